"""Loading a chromosome's LD the way the reference's constructors do (viprs/model/VIPRS.py:151-172, 203-207): which dtype
to ask the LD matrix for, which form, and the scale that turns stored integers into correlations.  Shared by the model
classes; merging the chromosomes into one plan is `viprs_amd.data.merge_ld_arrays`."""
import numpy as np


def ld_load_dtype(ld_mat, dequantize_on_the_fly, float_precision):
    """`(dtype, dequantize_on_the_fly)`: integer LD stays in its stored dtype when it is dequantised on the fly, everything
    else is loaded in the model's float precision -- and then nothing is left to dequantise (VIPRS.py:158-165)."""
    if dequantize_on_the_fly and np.issubdtype(ld_mat.stored_dtype, np.integer):
        return ld_mat.stored_dtype, dequantize_on_the_fly
    return float_precision, False


def load_ld_arrays(ld_mat, low_memory, dtype, expand=False, expand_ld_on_device=None):
    """`(loaded, expanded)`: the LD arrays (`.ld_data / .ld_indptr / .leftmost_idx`) in the upper-triangular form
    (`low_memory`) or the symmetric one.  `expand`: load the compact upper-triangular store although the symmetric form is
    wanted (it is mirrored on the device); a matrix that cannot hand out the symmetric form is loaded that way too unless
    `expand_ld_on_device` is False.  `expanded` tells which happened."""
    if not expand:
        try:
            return ld_mat.load(return_symmetric=not low_memory, dtype=dtype), False
        except ValueError:
            if low_memory or expand_ld_on_device is False:
                raise
    return ld_mat.load(return_symmetric=False, dtype=dtype), True


def dequantize_scale(ld_mat, dequantize_on_the_fly):
    """1 / (largest stored integer) for LD that is dequantised on the fly, else 1 (VIPRS.py:203-207)."""
    return 1.0 / np.iinfo(ld_mat.stored_dtype).max if dequantize_on_the_fly else 1.0
