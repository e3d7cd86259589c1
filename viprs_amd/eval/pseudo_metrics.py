"""Pseudo-validation metrics from summary statistics (Mak et al. 2017; Yang and Zhou 2020): with ``r`` the standardized
marginal betas of a validation cohort, ``b`` the effects under test and ``R`` the LD matrix of the validation panel,

    Corr(PRS, y) ~ r'b / sqrt(b'Rb),        R^2 ~ (r'b)^2 / (b'Rb).

``R b`` is the LD product of the device-resident plan (``LDPlan.dot``, ``viprs_plan_dot``): all columns of ``b`` -- the
models of a grid -- in one pass over the LD.

Arrays are taken as ALREADY MATCHED: ``std_beta[c]`` and ``beta[c]`` are in the SNP order of ``ld[c]``.  Matching SNPs and
alleles between panels is the caller's job (out of scope here).
"""
import numpy as np

__all__ = ["pseudo_pearson_r", "pseudo_r2", "_streamlined_pseudo_r2"]


def _default_dq_scale(plan):
    dt = np.dtype(plan.ld_dtype)
    return 1.0 / float(np.iinfo(dt).max) if np.issubdtype(dt, np.integer) else 1.0


def _ld_product(ld, B, dot_fn, dq_scale):
    if dot_fn is not None:
        return np.asarray(dot_fn(ld, B))
    from ..plan import LDPlan                            # (the native library is only needed when a plan is handed in)
    if isinstance(ld, LDPlan):                           # integer LD is stored unscaled
        return ld.dot(B, dq_scale=_default_dq_scale(ld) if dq_scale is None else dq_scale)
    return np.asarray(ld.dot(B))


def _sums(ld, std_beta, beta, dot_fn=None, dq_scale=None):
    """(rb, bsb) = (sum r b, sum b (R b)) per column over the chromosomes of `beta`, accumulated in float64."""
    if not isinstance(beta, dict):
        ld, std_beta, beta = {0: ld}, {0: std_beta}, {0: beta}
    rb = bsb = None
    for c in sorted(beta):
        if c not in std_beta or c not in ld:
            raise ValueError(f"chromosome {c} of the effects has no " + ("validation betas" if c not in std_beta else "LD"))
        b = np.asarray(beta[c])
        r = np.asarray(std_beta[c], dtype=np.float64)
        if b.shape[0] != r.shape[0]:
            raise ValueError(f"chromosome {c}: {b.shape[0]} effects against {r.shape[0]} validation betas "
                             "(the arrays must be matched to the LD panel's SNPs)")
        Rb = np.asarray(_ld_product(ld[c], b, dot_fn, dq_scale), dtype=np.float64)
        b64 = b.astype(np.float64)
        rb_c = np.sum((b64.T * r).T, axis=0)
        bsb_c = np.sum(b64 * Rb, axis=0)
        rb = rb_c if rb is None else rb + rb_c
        bsb = bsb_c if bsb is None else bsb + bsb_c
    if rb is None:
        raise ValueError("no effects were given")
    return rb, bsb


def pseudo_pearson_r(ld, std_beta, beta, dot_fn=None, dq_scale=None):
    """``r'b / sqrt(b'Rb)`` per column of `beta`.

    `ld`, `std_beta`, `beta`: ``{chromosome: ...}`` dicts (or one chromosome's objects).  ``ld[c]`` is an ``LDPlan`` or any
    object with ``.dot(B)``; ``dot_fn(ld_c, B)``, when given, computes the product instead.  ``beta[c]`` is ``(m,)`` or
    ``(m, n_models)``.  `dq_scale` (plans only) defaults to 1 for float LD and to 1 / the quantisation maximum for integer
    LD.  Every chromosome of `beta` must be in `std_beta` and `ld` (ValueError otherwise; chromosomes only they hold are not
    scored).  A column of zeros gives ``nan`` (0 / 0).  The arrays are taken as already matched to the panel's SNPs."""
    rb, bsb = _sums(ld, std_beta, beta, dot_fn, dq_scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        return rb / np.sqrt(bsb)


def pseudo_r2(ld, std_beta, beta, dot_fn=None, dq_scale=None):
    """The square of `pseudo_pearson_r` (the proxy the reference uses for the proportion of variance explained)."""
    return pseudo_pearson_r(ld, std_beta, beta, dot_fn, dq_scale) ** 2


def _streamlined_pseudo_r2(validation_beta, prs_beta, ldw_prs_beta):
    """``(r'b)^2 / (b'(Rb))`` with the LD-weighted effects ``Rb`` given (training and validation share the LD matrix, so a
    fitted model's ``q + b`` serves).  Matched, concatenated arrays."""
    prs_beta = np.asarray(prs_beta)
    rb = np.sum((prs_beta.T * np.asarray(validation_beta)).T, axis=0)
    bsb = np.sum(prs_beta * np.asarray(ldw_prs_beta), axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return rb ** 2 / bsb
