"""The C ABI of the per-genotype-class column sums (include/viprs_hip.h): the two entry points are declared with the documented
argument lists, the header carries the definition, the built library exports them and viprs_amd/_lib.py binds them; argument
checks that need no device; the Python signatures."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "viprs_hip.h")

DECLARED = {
    "viprs_genotypes_class_sums": "viprs_genotypes* g, int64_t row0, int64_t row1, int n_cols, "
                                  "const double* y_host /* n x n_cols, row-major */, "
                                  "double* sums_host /* (row1-row0) x 3 x n_cols, row-major */",
    "viprs_genotypes_last_class_sums_ms": "viprs_genotypes* g, double* ms",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_documented_argument_lists_and_the_definition():
    text = open(HEADER).read()
    for name, args in DECLARED.items():
        # (up to the first ");": a comment inside the list holds "(row1-row0)")
        mt = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, re.S)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name
    assert re.search(r"#define\s+VIPRS_CLASS_SUM_SLOTS\s+64\b", text)
    flat = _norm(text.replace("\n *", " "))
    for piece in ("k = 0: code 0", "k = 1: code 2", "k = 2: code 3", "Code 1 (missing) belongs to no class",
                  "(class(i, j) == k) ? Y[i][c] : +0.0", "s(i) = (i >> 4) & 63", "ascending i", "__dadd_rn", "no fma",
                  "for d in 32, 16, 8, 4, 2, 1: P[s] <- P[s] + P[s ^ d]", "all 64 values are identical",
                  "not on n_cols, on the other columns, on row0 / row1, on m", "two calls give identical bits",
                  "never becomes -0", "either implementation is allowed", "a row that was never uploaded gives zeros",
                  "(16 ceil(n / 1024) + 6) 2^-53 sum|t|", "Derived, not measured", "outputs untouched",
                  "on error paths too"):
        assert piece in flat, piece


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, i64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    want = {"viprs_genotypes_class_sums": [vp, i64, i64, i, vp, vp],
            "viprs_genotypes_last_class_sums_ms": [vp, ctypes.POINTER(d)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name


def test_bad_arguments_are_refused_before_any_device_work():
    """Every check of the arguments themselves comes before the object is touched: a null object reaches each of them without
    a device.  (The row range against m needs the object: tests/test_gpu_genotype_gwas.py.)"""
    from viprs_amd import _lib as L
    out = np.full(12, 7.0)
    y = np.ones(8)
    po, py = (a.ctypes.data_as(ctypes.c_void_p) for a in (out, y))
    for args, word in (((None, 0, 2, 0, py, po), "n_cols"),
                       ((None, 0, 2, -3, py, po), "n_cols"),
                       ((None, 3, 2, 2, py, po), "row0"),
                       ((None, 0, 2, 2, None, po), "null Y"),
                       ((None, 0, 2, 2, py, None), "host buffer"),
                       ((None, 0, 2, 2, py, po), "genotypes")):
        assert L.lib.viprs_genotypes_class_sums(*args) == L.EINVAL
        assert word in L.last_error(), (word, L.last_error())
    ms = ctypes.c_double(-1.0)
    assert L.lib.viprs_genotypes_last_class_sums_ms(None, ctypes.byref(ms)) == L.EINVAL
    assert np.all(out == 7.0) and ms.value == -1.0


def test_python_signatures():
    from viprs_amd import genotypes as G
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model.gridsearch import grid_utils
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert params(G.class_sums_host) == [("packed_rows", E), ("n", E), ("Y", E)]
    for cls in (G.HostGenotypes, G.DeviceGenotypes):
        assert params(cls.class_sums)[1:] == [("Y", E), ("max_bytes", 1 << 30)]
        assert params(cls.association)[1:] == [("Y", E), ("keep", None)]
        assert cls.association is G._Genotypes.association
    assert callable(G.DeviceGenotypes.last_class_sums_ms)
    assert params(ArrayDataLoader.perform_gwas)[1:] == [("phenotype", None), ("keep", None)]
    assert params(grid_utils.pseudo_validation_std_beta) == [("validation_gdl", E), ("model_gdl", E)]
    assert G.CLASS_SUM_SLOTS == 64 and G.CLASS_CODES == (0, 2, 3)


def test_kernel_sources_are_built_into_the_library():
    mk = open(os.path.join(ROOT, "viprs_amd", "csrc", "Makefile")).read()
    assert "geno_class_sums.hip" in mk
    for f in ("geno_class_sums.h", "geno_class_sums.hip"):
        assert os.path.exists(os.path.join(ROOT, "viprs_amd", "csrc", f))
    src = open(os.path.join(ROOT, "viprs_amd", "csrc", "geno_class_sums.h")).read()
    assert "__dadd_rn" in src and "__shfl_xor" in src and "VIPRS_CLASS_SUM_SLOTS" in src
    assert "atomic" not in src.replace("no atomics", "") and "fma" not in src
