"""The C ABI of the LD from genotypes (include/viprs_hip.h): the two entry points are declared with the documented argument
lists, exported by the built library and bound in viprs_amd/_lib.py; argument checks that need no device; the Python
signatures."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "viprs_hip.h")

DECLARED = {
    "viprs_genotypes_ld": "viprs_genotypes* g, int64_t row0, int64_t row1, const int64_t* right_end /* m */, "
                          "const double* w /* m */, int out_dtype, void* data_host /* rows [row0,row1) of the store */",
    "viprs_genotypes_last_ld_ms": "viprs_genotypes* g, double* ms",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_documented_argument_lists():
    text = open(HEADER).read()
    for name, args in DECLARED.items():
        # (up to the first ");": a comment inside the list holds the half-open range "[row0,row1)")
        mt = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name
    # the definition sits with the declarations, in full
    flat = _norm(text.replace("\n *", " "))
    for piece in ("nn_j = c0 + c2 + c3", "a_j = 2 c0 + c2", "q_j = 4 c0 + c2", "d_j = nn_j q_j - a_j^2",
                  "w_j = sqrt((double)(nn_j d_j))", "ON THE HOST",
                  "num_ij = nn_i nn_j S_ij - nn_i a_j U_ij - nn_j a_i U_ji + a_i a_j N_ij",
                  "(w_i == 0 || w_j == 0) ? 0.0 : (double)num_ij / (w_i * w_j)", "rint(r 127) clamped to +-127",
                  "rint(r 32767) clamped to +-32767", "n <= 2^19", "4 n^3 4 < 2^63",
                  "indptr[j + 1] - indptr[j] = right_end[j] - j - 1", "non-decreasing"):
        assert piece in flat, piece


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, i64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    want = {"viprs_genotypes_ld": [vp, i64, i64, vp, vp, i, vp], "viprs_genotypes_last_ld_ms": [vp, ctypes.POINTER(d)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name


def test_bad_arguments_are_refused_before_any_device_work():
    """Every check of the arguments themselves comes before the object is touched: a null object reaches each of them without
    a device.  (What needs the object -- m, n -- is checked on the device box: tests/test_gpu_genotype_ld.py.)"""
    from viprs_amd import _lib as L
    out = np.full(4, 7.0, dtype=np.float32)
    re_ = np.array([4, 4, 4, 4], dtype=np.int64)
    w = np.ones(4, dtype=np.float64)
    po, pr, pw = (a.ctypes.data_as(ctypes.c_void_p) for a in (out, re_, w))
    for args, word in (((None, 0, 4, pr, pw, 7, po), "dtype"),
                       ((None, 0, 4, pr, pw, L.LD_I32, po), "dtype"),
                       ((None, 0, 4, pr, pw, L.LD_I64, po), "dtype"),
                       ((None, 3, 2, pr, pw, L.LD_F32, po), "row0"),
                       ((None, 0, 4, None, pw, L.LD_F32, po), "right_end"),
                       ((None, 0, 4, pr, None, L.LD_F32, po), "null w"),
                       ((None, 0, 4, pr, pw, L.LD_F32, None), "host buffer"),
                       ((None, 0, 4, pr, pw, L.LD_I8, po), "genotypes")):
        assert L.lib.viprs_genotypes_ld(*args) == L.EINVAL
        assert word in L.last_error(), (word, L.last_error())
    ms = ctypes.c_double(-1.0)
    assert L.lib.viprs_genotypes_last_ld_ms(None, ctypes.byref(ms)) == L.EINVAL
    assert np.all(out == 7.0) and ms.value == -1.0


def test_python_signatures():
    from viprs_amd import genotypes as G
    from viprs_amd.data import ArrayDataLoader
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert params(G.ld_host) == [("packed_rows", E), ("n", E), ("right_end", E), ("dtype", np.float32)]
    assert params(G.ld_windows) == [("estimator", E), ("m", E)]
    for cls in (G.HostGenotypes, G.DeviceGenotypes):
        assert params(cls.ld)[1:] == [("window", None), ("dtype", np.float32), ("max_bytes", 1 << 30)]
    assert callable(G.DeviceGenotypes.last_ld_ms) and callable(G.DeviceGenotypes.ld_rows)
    assert params(ArrayDataLoader.compute_ld)[1:] == [("estimator", ("sample",)), ("dtype", np.float32),
                                                      ("max_bytes", 1 << 30)]
    assert G.LD_MAX_SAMPLES == 1 << 19


def test_kernel_sources_are_built_into_the_library():
    mk = open(os.path.join(ROOT, "viprs_amd", "csrc", "Makefile")).read()
    assert "geno_ld.hip" in mk
    for f in ("geno_ld.h", "geno_ld.hip"):
        assert os.path.exists(os.path.join(ROOT, "viprs_amd", "csrc", f))
    src = open(os.path.join(ROOT, "viprs_amd", "csrc", "geno_ld.h")).read()
    assert "__builtin_amdgcn_mfma_i32_32x32x32_i8" in src and "atomic" not in src.replace("No atomics", "")
