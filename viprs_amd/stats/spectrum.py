"""Extremal eigenvalues of LD matrices on the device, and the ridge penalty ``lambda_min`` the models derive from them.

The reference's CLI fits with ``lambda_min='infer'``: the model asks the LD matrix for ``get_lambda_min(min_max_ratio=1e-3)``
(viprs/model/VIPRS.py:174-191) and magenpy answers from the extremal eigenvalues it computed per LD block (ARPACK, on the
CPU) when the store was built.  LD that has no stored spectrum -- arrays, stores written without one, LD built on the
device -- gets it here: ``LDPlan.extremal_eigenvalues`` runs one Lanczos recurrence per LD block, all blocks in lock step,
and the extremes of a chromosome are the extremes over its blocks (the matrix is block diagonal).

* ``lambda_min_from_extremes``  the penalty from the two extremes (what ``ZarrLDMatrix.get_lambda_min`` applies);
* ``ld_spectrum``               the spectrum of one LD matrix or of every chromosome of a data loader;
* ``annotate_spectrum``         computes it and attaches it to the LD objects, so that ``lambda_min='infer'`` finds it.
"""
import json
import os

FORMULAS = ("one_plus_r", "one_minus_r")


class UnpinnedLambdaMinError(NotImplementedError):
    """`lambda_min='infer'` with a min / max ratio on LD that carries extremal eigenvalues: the formula is unverified
    (`lambda_min_from_extremes`)."""


def lambda_min_from_extremes(lam_min, lam_max, min_max_ratio=0.0, formula=None, where="the LD matrix"):
    """The ridge penalty from the extremal eigenvalues of an LD matrix.

    * ``r = min_max_ratio == 0`` (or no ``lam_max``): ``|min(lam_min, 0)|`` -- no formula involved, 0 for a positive
      definite matrix;
    * ``r > 0``: PARITY UNPINNED.  magenpy (not in the reference tree) defines what ``get_lambda_min(min_max_ratio)``
      applies; the two candidates
          "one_plus_r"  : max((r lam_max - lam_min) / (1 + r), 0)   (as recalled from magenpy 0.1.x)
          "one_minus_r" : max((r lam_max - lam_min) / (1 - r), 0)   (the algebraic solution of
                          (lam_min + x) = r (lam_max + x))
      differ by (1 - r) / (1 + r) (0.2 % at VIPRS's r = 1e-3) and nothing here decides between them.  Rather than hand
      ``fit()`` an unverified ridge this RAISES `UnpinnedLambdaMinError` unless `formula` names one
      (``tools/check_store.py`` tells which one a magenpy installation agrees with)."""
    lam_min = float(lam_min)
    r = float(min_max_ratio or 0.0)
    if r > 0.0 and lam_max is not None:
        lam_max = float(lam_max)
        if formula not in FORMULAS:
            raise UnpinnedLambdaMinError(
                f"{where}: the store carries extremal eigenvalues (min {lam_min}, max {lam_max}) but the formula "
                "magenpy's LDMatrix.get_lambda_min(min_max_ratio) applies to them could not be verified (magenpy is "
                "not available where this reader was written).  Pass a numeric lambda_min to VIPRS(...), or choose "
                "ZarrLDMatrix.lambda_min_formula = 'one_plus_r' | 'one_minus_r' (tools/check_store.py tells which one "
                "a magenpy installation agrees with).")
        den = 1.0 + r if formula == "one_plus_r" else 1.0 - r
        return max((r * lam_max - lam_min) / den, 0.0)
    return abs(min(lam_min, 0.0))


def _ld_matrices(ld_mat_or_gdl):
    if hasattr(ld_mat_or_gdl, "get_ld_matrices"):
        return dict(ld_mat_or_gdl.get_ld_matrices())
    if isinstance(ld_mat_or_gdl, dict):
        return dict(ld_mat_or_gdl)
    return {getattr(ld_mat_or_gdl, "chromosome", None): ld_mat_or_gdl}


def plan_spectrum(plan, segments=None, **kw):
    """`plan.extremal_eigenvalues(**kw)` summarised: ``{key: {"min", "max", "per_block"}}`` for every ``key: (start, end)``
    SNP range of `segments` (ranges made of whole LD blocks: the chromosomes of a merged plan); one entry under None
    without `segments`.  A range without SNPs has the spectrum of the empty matrix's identity: 1, 1."""
    from ..plan import SpectrumInfo
    info = plan.extremal_eigenvalues(**kw)
    starts = plan.blocks()[0][:-1]
    out = {}
    for key, (a, e) in (segments or {None: (0, plan.m)}).items():
        sel = (starts >= a) & (starts < e)
        part = SpectrumInfo(info.lambda_min[sel], info.lambda_max[sel], info.resid_min[sel], info.resid_max[sel],
                            info.iterations[sel], info.status[sel], info.ms, info.host_ms)
        out[key] = {"min": float(part.lambda_min.min()) if sel.any() else 1.0,
                    "max": float(part.lambda_max.max()) if sel.any() else 1.0, "per_block": part}
    return out


def ld_spectrum(ld_mat_or_gdl, low_memory=True, dequantize_on_the_fly=False, device=0, float_precision="float32", **kw):
    """Extremal eigenvalues of one LD matrix object, of a ``{chromosome: LD matrix}`` dict or of every chromosome of a data
    loader, on HIP device `device`: ``{chromosome: {"min": ..., "max": ..., "per_block": SpectrumInfo}}``.  The LD is
    loaded as the models load it (`low_memory`: the upper-triangular form; `dequantize_on_the_fly`: integer LD stays in
    its stored dtype on the device, decided per matrix) -- the spectrum is that of the matrix the E-step multiplies with.
    With ``low_memory=False`` a matrix that holds only the upper-triangular store is mirrored on the device, as `VIPRS`
    does by default.  `kw`: ``rtol``, ``maxiter`` of `LDPlan.extremal_eigenvalues`."""
    from .. import _lib
    from ..model._ld_loading import dequantize_scale, load_chromosome_ld, open_plan
    if _lib.device_count() < 1:
        raise RuntimeError("ld_spectrum needs a HIP device: the Lanczos recurrence has no CPU fallback")
    out = {}
    for c, ld_mat in _ld_matrices(ld_mat_or_gdl).items():
        ld = load_chromosome_ld(ld_mat, low_memory, dequantize_on_the_fly, float_precision)
        plan = open_plan(ld, device)
        try:
            out[c] = plan_spectrum(plan, dq_scale=dequantize_scale(ld_mat, ld.dequantize), float_precision=float_precision,
                                   **kw)[None]
        finally:
            plan.close()
    return out


def attach_extremal(ld_mat, lam_min, lam_max, write=False):
    """Hands the extremes to one LD object: `set_extremal` where it has one (`LDArrays`), else the in-memory attributes
    ``attrs["Spectral properties"]["Extremal"]`` that `ZarrLDMatrix.get_lambda_min` reads (magenpy's layout); `write`: into
    the store's ``.zattrs`` as well."""
    if hasattr(ld_mat, "set_extremal"):
        ld_mat.set_extremal(lam_min, lam_max)
    elif isinstance(getattr(ld_mat, "attrs", None), dict):
        sp = ld_mat.attrs.get("Spectral properties")
        if not isinstance(sp, dict):
            sp = ld_mat.attrs["Spectral properties"] = {}
        sp["Extremal"] = {"min": float(lam_min), "max": float(lam_max)}
    else:
        raise TypeError(f"{type(ld_mat).__name__}: no `set_extremal` and no `attrs` to attach the extremal eigenvalues to")
    if write:
        path = getattr(ld_mat, "path", None)
        if path is None or not os.path.isdir(path):
            raise ValueError(f"write=True: {type(ld_mat).__name__} is not backed by a store directory")
        za = os.path.join(path, ".zattrs")
        attrs = {}
        if os.path.exists(za):
            with open(za) as f:
                attrs = json.load(f)
        sp = attrs.get("Spectral properties")
        if not isinstance(sp, dict):
            sp = attrs["Spectral properties"] = {}
        sp["Extremal"] = {"min": float(lam_min), "max": float(lam_max)}
        tmp = za + ".tmp"
        with open(tmp, "w") as f:
            json.dump(attrs, f)
        os.replace(tmp, za)


def annotate_spectrum(gdl, write=False, **kw):
    """`ld_spectrum(gdl, **kw)`, attached to every LD object of the loader (`attach_extremal`): afterwards
    ``lambda_min='infer'`` works in every model class, the per-chromosome ones included.  Returns the spectrum."""
    spectrum = ld_spectrum(gdl, **kw)
    mats = _ld_matrices(gdl)
    for c, s in spectrum.items():
        attach_extremal(mats[c], s["min"], s["max"], write=write)
    return spectrum
