"""LD scores on the device and the LD-score heritability estimate the models start from.

The reference takes both from magenpy: ``LDMatrix.ld_score`` / ``compute_ld_scores(annotation_matrix=...)`` and
``magenpy.stats.h2.ldsc.simple_ldsc`` (viprs/model/LDPredInf.py:32-33, VIPRS.py:279-292, VIPRSMix.py:134).  magenpy is not
part of the reference tree, so nothing here claims parity with it; the definitions are stated in full:

* the LD score of SNP j under the annotation column a is ``l_j = sum_k a_k r2_jk`` over every stored entry of row j of the
  symmetric LD matrix, the diagonal (``r_jj = 1``) included; with the sample-size correction every OFF-diagonal ``r^2`` is
  replaced by the adjusted ``r^2 - (1 - r^2) c``, ``c = 1 / (n_LD - 2)`` (Bulik-Sullivan et al. 2015);
* ``simple_ldsc`` is the intercept-free moment estimate ``h2 = (mean(chi2) - 1) M / (mean(l) mean(N))`` with
  ``chi2_j = N_j beta_hat_j^2`` from the standardised marginal effects.

* ``ld_scores_host``      plain NumPy in float64, written from the definition: the CPU fallback and the base of the tests;
* ``ld_scores``           the scores of one LD matrix or of every chromosome of a data loader (`LDPlan.ld_scores`);
* ``annotate_ld_scores``  computes the unstratified scores and attaches them to the LD objects (``ld_mat.ld_score``);
* ``simple_ldsc``         the heritability estimate of a data loader.
"""
import numpy as np

from .spectrum import _ld_matrices


def ld_scores_host(lb, ip, data, low_memory, weights=None, correction=None, dq_scale=1.0):
    """LD scores of the matrix the arrays stand for (the layout of `LDPlan`), in float64: ``(m,)`` without `weights` (one
    column of ones) or for ``(m,)`` weights, ``(m, G)`` for ``(m, G)`` weights.  `correction`: None or ``(m,)`` values
    ``c_j``.  Off-diagonal entries are ``dq_scale * stored``; the diagonal counts as 1 and is never corrected."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    A = np.ones((m, 1)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(m, -1)
    r2 = (float(dq_scale) * np.asarray(data, dtype=np.float64)) ** 2
    S2, S0 = np.zeros(A.shape), np.zeros(A.shape)
    for j in range(m):
        s, e = int(ip[j]), int(ip[j + 1])
        if e == s:
            continue
        cols = int(lb[j]) + np.arange(e - s)
        p = r2[s:e]
        if not low_memory:                                 # symmetric form: the stored diagonal entry is no entry
            keep = cols != j
            cols, p = cols[keep], p[keep]
        S2[j] += p @ A[cols]
        S0[j] += A[cols].sum(axis=0)
        if low_memory:                                     # upper form: the transposed entries (i, j) of the rows i < j
            S2[cols] += p[:, None] * A[j]
            S0[cols] += A[j]
    score = S2 + A
    if correction is not None:
        score = score + np.asarray(correction, dtype=np.float64)[:, None] * (S2 - S0)
    return score[:, 0] if weights is None or np.ndim(weights) == 1 else score


def ld_correction(ld_mat, m, where="the LD matrix"):
    """``(m,)`` values ``c = 1 / (n_LD - 2)`` from the LD object's ``sample_size``."""
    n = getattr(ld_mat, "sample_size", None)
    if n is None or not float(n) > 2.0:
        raise ValueError(f"{where}: corrected LD scores need the sample size of the LD reference panel (found "
                         f"{n!r}).  Remedy: set `sample_size` on the LD object (LDArrays(..., sample_size=n); the "
                         "'Sample size' attribute of a store), or ask for corrected=False.")
    return np.full(int(m), 1.0 / (float(n) - 2.0))


def ld_scores(ld_mat_or_gdl, annotation=None, corrected=True, low_memory=True, dequantize_on_the_fly=False, device=0,
              float_precision="float32", score_fn=None):
    """LD scores of one LD matrix object, of a ``{chromosome: LD matrix}`` dict or of every chromosome of a data loader:
    ``{chromosome: array}``, ``(m_c,)`` or -- with `annotation`, an ``(m_c, G)`` array or a ``{chromosome: array}`` dict --
    ``(m_c, G)``.  The LD is loaded as the models load it (`load_chromosome_ld`), with two decisions of this function's own:
    `dequantize_on_the_fly` is decided per matrix, and a matrix that holds only the upper-triangular store is scored in
    that form with ``low_memory=False`` too, not mirrored (the scores of both forms are those of the same matrix).
    `corrected`: the adjusted r^2 with ``c = 1 / (n_LD - 2)`` from the LD object's ``sample_size`` (ValueError when it has
    none).  On HIP device `device` (`LDPlan.ld_scores`); without a device, or with `score_fn` (a callable with
    `ld_scores_host`'s signature), on the host in float64."""
    from .. import _lib
    from ..model._ld_loading import dequantize_scale, load_chromosome_ld, open_plan
    on_host = score_fn is not None or _lib.device_count() < 1
    score_fn = score_fn or ld_scores_host
    out = {}
    for c, ld_mat in _ld_matrices(ld_mat_or_gdl).items():
        ld = load_chromosome_ld(ld_mat, low_memory, dequantize_on_the_fly, float_precision).as_stored()
        A = annotation[c] if isinstance(annotation, dict) else annotation
        corr = ld_correction(ld_mat, ld.left_bound.shape[0], where=f"chromosome {c}") if corrected else None
        dq = dequantize_scale(ld_mat, ld.dequantize)
        if on_host:
            out[c] = score_fn(ld.left_bound, ld.indptr, ld.data, ld.form == "upper", A, corr, dq)
            continue
        plan = open_plan(ld, device)
        try:
            A = None if A is None else np.asarray(A, dtype=float_precision)
            out[c] = plan.ld_scores(A, corr, dq_scale=dq, float_precision=float_precision)
        finally:
            plan.close()
    return out


_compute_ld_scores = ld_scores          # (`simple_ldsc` has a parameter of that name)


def annotate_ld_scores(gdl, **kw):
    """`ld_scores(gdl, **kw)` without annotations, attached to every LD object of the loader (`set_ld_score`): afterwards
    ``ld_mat.ld_score`` answers and `simple_ldsc` uses it.  Returns the scores."""
    if kw.get("annotation") is not None:
        raise ValueError("annotate_ld_scores attaches the unstratified scores: no `annotation`")
    scores = ld_scores(gdl, **kw)
    mats = _ld_matrices(gdl)
    for c, s in scores.items():
        if not hasattr(mats[c], "set_ld_score"):
            raise TypeError(f"{type(mats[c]).__name__}: no `set_ld_score` to attach the LD scores to")
        mats[c].set_ld_score(s)
    return scores


def chisq_statistic(ss):
    """chi2_j of one chromosome's summary statistics: its own `get_chisq_statistic()`, else N_j beta_hat_j^2."""
    if hasattr(ss, "get_chisq_statistic"):
        return np.asarray(ss.get_chisq_statistic(), dtype=np.float64)
    return np.asarray(ss.n_per_snp, dtype=np.float64) * np.asarray(ss.get_snp_pseudo_corr(), dtype=np.float64) ** 2


def ldsc_estimate(chisq, ld_score, n_per_snp):
    """``(mean(chi2) - 1) M / (mean(l) mean(N))`` over the SNPs given (float64)."""
    chisq, ld_score = np.asarray(chisq, dtype=np.float64), np.asarray(ld_score, dtype=np.float64)
    n = np.asarray(n_per_snp, dtype=np.float64)
    return float((chisq.mean() - 1.0) * chisq.shape[0] / (ld_score.mean() * n.mean()))


def ldsc_estimate_over(sumstats_table, scores, chroms):
    """`ldsc_estimate` over the SNPs of the chromosomes `chroms`, concatenated in that order: chi2 and N from
    ``sumstats_table[c]``, the LD scores from ``scores[c]``.  What `simple_ldsc`, `VIPRS(h2_init="ldsc")` and
    `LDPredInf(h2=None)` report."""
    return ldsc_estimate(np.concatenate([chisq_statistic(sumstats_table[c]) for c in chroms]),
                         np.concatenate([np.asarray(scores[c], dtype=np.float64) for c in chroms]),
                         np.concatenate([np.asarray(sumstats_table[c].n_per_snp, dtype=np.float64).ravel() for c in chroms]))


def simple_ldsc(gdl, ld_scores=None, **kw):
    """The LD-score regression estimate of the SNP heritability without an intercept, over all chromosomes of the loader.
    `ld_scores`: ``{chromosome: (m_c,) array}``; else the scores attached to the LD objects where present, else they are
    computed (`ld_scores(gdl, **kw)`, module function)."""
    mats = _ld_matrices(gdl)
    chroms = sorted(gdl.sumstats_table)
    if ld_scores is None:
        ld_scores = {}
        for c in chroms:
            try:
                ld_scores[c] = mats[c].ld_score
            except (AttributeError, ValueError):
                ld_scores = None
                break
        if ld_scores is None:
            ld_scores = _compute_ld_scores(gdl, **kw)
    return ldsc_estimate_over(gdl.sumstats_table, ld_scores, chroms)
