"""The one path from a data loader's LD matrix object to arrays in host memory and from those to an `LDPlan` on the device
(the reference's "load LD matrices to memory", viprs/model/VIPRS.py:151-172, 203-207).

* ``load_chromosome_ld``  LD matrix object -> `LoadedLD`: which dtype to ask for, which form, whether the entries are read
  at all.  The only caller of ``ld_mat.load(...)`` in the package.
* ``load_ld_in_order``    the model classes' loop over it: ``dequantize_on_the_fly`` threaded through the chromosomes.
* ``open_plan``           `LoadedLD` -> `LDPlan`: the only place outside `viprs_amd.plan` that chooses between
  ``LDPlan(...)`` and ``LDPlan.from_upper(...)``.
* ``empty_ld``            the arrays of a rank that holds no LD block.
* ``dequantize_scale``    the scale that turns stored integers into correlations.

Merging several chromosomes into one plan stays `viprs_amd.data.merge_ld_arrays`.

Who calls what, and the differences between the entry points -- decisions, each an argument here:

=====================================  =========================  ===========================================================
caller                                 ``expand_ld_on_device``    an upper-only store with ``low_memory=False``
=====================================  =========================  ===========================================================
`VIPRS.__init__` (`_load_ld`)          None / True / False        None, True: mirrored on the device; False: the ValueError
`MergedPlanModel._load` (7 models)     False                      the matrix's ValueError (never expands)
`stats.ldsc.ld_scores`                 None                       scored in the upper form (`LoadedLD.as_stored`)
`stats.spectrum.ld_spectrum`           None                       mirrored on the device
`model.VIPRS._pseudo_r2_external`      -- (arrays handed in)      --
=====================================  =========================  ===========================================================

``dequantize_on_the_fly``: every matrix decides for itself (`LoadedLD.dequantize`).  `VIPRS` and the models on a merged
plan (`_merged_plan`) thread the decision through the chromosomes in sorted order (`load_ld_in_order`) -- the first
float-stored chromosome turns it off for all later ones -- and take `dequantize_scale` from the FIRST chromosome's matrix;
the two `stats` functions decide per matrix.  Whether these differences should be unified is not decided here; they are
only visible in one place now.
"""
from collections import namedtuple

import numpy as np


class LoadedLD(namedtuple("LoadedLD", "left_bound indptr data form dtype ld_mat dequantize",
                          defaults=(None, None, False))):
    """One chromosome's LD in host memory: `left_bound` (int32), `indptr`, `data`, C-contiguous.  `form`: "upper",
    "symmetric", or "upper_to_expand" -- the compact upper store was loaded although the symmetric form was wanted (it is
    mirrored on the device, `LDPlan.from_upper`).  `dtype`: what ``load`` was asked for.  `ld_mat`: the matrix object when
    only the index was read (`data` is None then), else None.  `dequantize`: the matrix's own ``dequantize_on_the_fly``."""
    __slots__ = ()

    @classmethod
    def from_arrays(cls, left_bound, indptr, data, form, *rest):
        """The record of arrays as a loader hands them out: made C-contiguous, the window starts int32 (what `LDPlan`
        takes; arrays that already are come through as they are)."""
        return cls(np.ascontiguousarray(left_bound, dtype=np.int32), np.ascontiguousarray(indptr),
                   np.ascontiguousarray(data), form, *rest)

    def as_stored(self):
        """The arrays in the form they are stored in: an "upper_to_expand" store as "upper"."""
        return self._replace(form="upper") if self.form == "upper_to_expand" else self


def ld_form(low_memory, expanded=False):
    """The `LoadedLD.form` of arrays loaded for `low_memory`; `expanded`: the upper store, although symmetric was wanted."""
    return "upper_to_expand" if expanded else "upper" if low_memory else "symmetric"


def load_chromosome_ld(ld_mat, low_memory, dequantize_on_the_fly, float_precision, expand_ld_on_device=None,
                       index_only=False):
    """`LoadedLD` of one LD matrix object.

    * dtype: integer LD stays in its stored dtype when it is dequantised on the fly, everything else is loaded in
      `float_precision` -- and then nothing is left to dequantise (VIPRS.py:158-165).
    * form: upper-triangular (`low_memory`) or symmetric.  `expand_ld_on_device` (``low_memory=False`` only) True: the
      compact upper store is loaded instead; None: only when the matrix cannot hand out the symmetric form (its
      ValueError); False: never, the matrix's ValueError passes.
    * `index_only`: a store that can hand out row ranges (``load_rows``, `viprs_amd.io.zarr_ld.ZarrLDMatrix`) is not read
      beyond its index -- unless the symmetric form is wanted and `expand_ld_on_device` is False, which such a read
      cannot serve.  The upper store's windows are implied: row j starts at column j + 1."""
    if dequantize_on_the_fly and np.issubdtype(ld_mat.stored_dtype, np.integer):
        dtype, dequantize = ld_mat.stored_dtype, dequantize_on_the_fly
    else:
        dtype, dequantize = float_precision, False
    if index_only and hasattr(ld_mat, "load_rows") and (low_memory or expand_ld_on_device is not False):
        indptr = np.ascontiguousarray(ld_mat.indptr())
        return LoadedLD(np.arange(1, indptr.shape[0], dtype=np.int32), indptr, None, ld_form(low_memory, not low_memory),
                        dtype, ld_mat, dequantize)
    expanded = bool(expand_ld_on_device) and not low_memory
    if not expanded:
        try:
            lop = ld_mat.load(return_symmetric=not low_memory, dtype=dtype)
        except ValueError:
            if low_memory or expand_ld_on_device is False:
                raise
            expanded = True
    if expanded:
        lop = ld_mat.load(return_symmetric=False, dtype=dtype)
    return LoadedLD.from_arrays(lop.leftmost_idx, lop.ld_indptr, lop.ld_data, ld_form(low_memory, expanded), dtype, None,
                                dequantize)


def load_ld_in_order(ld_mats, chroms, low_memory, dequantize_on_the_fly, float_precision, **kw):
    """The model classes' loop over `load_chromosome_ld`: ``({chromosome: LoadedLD}, dequantize_on_the_fly,
    dequantize_scale)``.  `dequantize_on_the_fly` is threaded through `chroms` in the order given (sorted, in both models):
    every matrix gets what the one before it decided, so the first float-stored chromosome turns it off for all later
    ones; what comes out is the last decision.  `dequantize_scale` comes from the FIRST chromosome's matrix
    (VIPRS.py:203-207)."""
    loaded = {}
    for c in chroms:
        loaded[c] = load_chromosome_ld(ld_mats[c], low_memory, dequantize_on_the_fly, float_precision, **kw)
        dequantize_on_the_fly = loaded[c].dequantize
    return loaded, dequantize_on_the_fly, dequantize_scale(ld_mats[chroms[0]], dequantize_on_the_fly)


def empty_ld(dtype, form):
    """The LD of no SNP at all: what a rank without any LD block makes its plan from (it still takes part in the
    reductions)."""
    return LoadedLD(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, dtype), form)


def open_plan(ld, device, math_mode="exact"):
    """The `LDPlan` of a `LoadedLD` on HIP device `device`: mirrored on the device from an "upper_to_expand" store, else
    from the arrays as they are.  (`LDPlan` is looked up when this is called: tests replace it on `viprs_amd.plan`.)"""
    from .. import plan
    if ld.form == "upper_to_expand":
        return plan.LDPlan.from_upper(ld.indptr, ld.data, device=device, math_mode=math_mode)
    return plan.LDPlan(ld.left_bound, ld.indptr, ld.data, ld.form == "upper", device=device, math_mode=math_mode)


def dequantize_scale(ld_mat, dequantize_on_the_fly):
    """1 / (largest stored integer) for LD that is dequantised on the fly, else 1 (VIPRS.py:203-207)."""
    return 1.0 / np.iinfo(ld_mat.stored_dtype).max if dequantize_on_the_fly else 1.0
