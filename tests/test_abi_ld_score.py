"""The C ABI of the LD scores (include/viprs_hip.h): the two entry points are declared with the documented argument lists,
exported by the built library and bound in viprs_amd/_lib.py; argument checks that need no device; the Python signatures."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_plan_ld_scores": "viprs_plan* plan, int float_dtype, int n_cols, const void* a_host, const double* corr_host, "
                            "void* scores_host, double dq_scale",
    "viprs_plan_last_ld_score_ms": "viprs_plan* plan, double* ms",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_documented_argument_lists():
    text = open(HEADER).read()
    for name, args in DECLARED.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name
    # the definition and the rounding bound sit with the declarations
    flat = _norm(text.replace("\n *", " "))
    for piece in ("p = fl(x x)", "fma(p, A[i, g], acc)", "d2 = fl(d d)", "score = fl(fl(U + fl(c fl(U - S0))) + A[j, g])",
                  "eps_T (D(L) + 1) sum p |A|", "eps_T D(L) sum |A|"):
        assert piece in flat, piece


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"viprs_plan_ld_scores": [vp, i, i, vp, vp, vp, d], "viprs_plan_last_ld_score_ms": [vp, ctypes.POINTER(d)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name


def test_bad_arguments_are_refused_before_any_device_work():
    """Every argument check comes before the plan is touched: a null plan reaches each of them without a device."""
    from viprs_amd import _lib as L
    y = np.full(4, 7.0, dtype=np.float32)
    a = np.ones(4, dtype=np.float32)
    py, pa = y.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p)
    for args, word in (((None, 7, 1, pa, None, py, 1.0), "dtype"),
                       ((None, L.F32, 0, pa, None, py, 1.0), "n_cols"),
                       ((None, L.F32, 2, None, None, py, 1.0), "unit weights"),
                       ((None, L.F32, 1, None, None, py, 1.0), "plan"),
                       ((None, L.F64, 1, pa, None, None, 1.0), "plan")):
        assert L.lib.viprs_plan_ld_scores(*args) == L.EINVAL
        assert word in L.last_error(), (word, L.last_error())
    ms = ctypes.c_double(-1.0)
    assert L.lib.viprs_plan_last_ld_score_ms(None, ctypes.byref(ms)) == L.EINVAL
    assert np.all(y == 7.0) and ms.value == -1.0


def test_python_signatures():
    from viprs_amd.model import LDPredInf, VIPRS
    from viprs_amd.plan import LDPlan
    from viprs_amd.stats import ldsc
    params = lambda f: list(inspect.signature(f).parameters.items())
    assert [(n, p.default) for n, p in params(LDPlan.ld_scores)[1:]] == [
        ("weights", None), ("correction", None), ("dq_scale", 1.0), ("float_precision", "float32")]
    assert callable(LDPlan.last_ld_score_ms)
    assert [(n, p.default) for n, p in params(ldsc.ld_scores_host)] == [
        ("lb", inspect.Parameter.empty), ("ip", inspect.Parameter.empty), ("data", inspect.Parameter.empty),
        ("low_memory", inspect.Parameter.empty), ("weights", None), ("correction", None), ("dq_scale", 1.0)]
    assert [(n, p.default) for n, p in params(ldsc.ld_scores)[:7]] == [
        ("ld_mat_or_gdl", inspect.Parameter.empty), ("annotation", None), ("corrected", True), ("low_memory", True),
        ("dequantize_on_the_fly", False), ("device", 0), ("float_precision", "float32")]
    assert [n for n, _ in params(ldsc.simple_ldsc)[:2]] == ["gdl", "ld_scores"] and callable(ldsc.annotate_ld_scores)
    # LDPredInf keeps its first eight constructor parameters; h2 has the reference's default
    assert [n for n, _ in params(LDPredInf.__init__)[1:9]] == [
        "gdl", "h2", "float_precision", "low_memory", "dequantize_on_the_fly", "device", "solve_fn", "comm"]
    assert inspect.signature(LDPredInf.__init__).parameters["h2"].default is None
    assert inspect.signature(VIPRS.__init__).parameters["h2_init"].default is None
