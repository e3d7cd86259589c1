"""The C ABI of LD clumping (include/viprs_hip.h): the two entry points are declared with the documented argument lists,
exported by the built library and bound in viprs_amd/_lib.py; argument checks that need no device; the Python signatures."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_plan_clump": "viprs_plan* plan, int64_t n_order, const int32_t* order_host, const uint8_t* member_host, "
                        "int n_cols, const double* r2_host, double dq_scale, int32_t* index_of_host",
    "viprs_plan_last_clump_ms": "viprs_plan* plan, double* ms",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_documented_argument_lists():
    text = open(HEADER).read()
    for name, args in DECLARED.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name
    # the definition sits with the declarations
    flat = _norm(text.replace("\n *", " "))
    for piece in ("(double)x * (double)x >= thr[g]", "thr[g] = r2[g] / s2", "s2 = dq_scale * dq_scale",
                  "avail = member, index_of[:, g] = -1", "index_of[j, g] = j and avail[j] = 0",
                  "index_of[k, g] = j and avail[k] = 0", "a stored zero is an entry",
                  "viprs_plan_set_active_blocks does NOT filter the call", "1 <= n_cols <= 32"):
        assert piece in flat, piece


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, i64, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    want = {"viprs_plan_clump": [vp, i64, vp, vp, i, vp, d, vp], "viprs_plan_last_clump_ms": [vp, ctypes.POINTER(d)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name


def test_bad_arguments_are_refused_before_any_device_work():
    """The checks of the thresholds, the column count and the scale come before the plan is touched: a null plan reaches
    each of them without a device."""
    from viprs_amd import _lib as L
    out = np.full(8, 7, dtype=np.int32)
    order = np.arange(4, dtype=np.int32)
    po, pout = order.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    r2 = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)
    many = np.full(33, 0.1)
    for args, word in (((None, 4, po, None, 0, r2(0.1), 1.0, pout), "n_cols"),
                       ((None, 4, po, None, 33, many.ctypes.data_as(ctypes.c_void_p), 1.0, pout), "n_cols"),
                       ((None, 4, po, None, 1, None, 1.0, pout), "r2"),
                       ((None, 4, po, None, 2, r2(0.1, -0.1), 1.0, pout), "thresholds"),
                       ((None, 4, po, None, 2, r2(np.nan, 0.1), 1.0, pout), "thresholds"),
                       ((None, 4, po, None, 1, r2(np.inf), 1.0, pout), "thresholds"),
                       ((None, 4, po, None, 1, r2(0.1), 0.0, pout), "dq_scale"),
                       ((None, 4, po, None, 1, r2(0.1), -1.0, pout), "dq_scale"),
                       ((None, 4, po, None, 1, r2(0.1), np.inf, pout), "dq_scale"),
                       ((None, 4, po, None, 1, r2(0.1), np.nan, pout), "dq_scale"),
                       ((None, 4, po, None, 2, r2(0.1, 0.2), 1.0, pout), "plan")):
        assert L.lib.viprs_plan_clump(*args) == L.EINVAL
        assert word in L.last_error(), (word, L.last_error())
    ms = ctypes.c_double(-1.0)
    assert L.lib.viprs_plan_last_clump_ms(None, ctypes.byref(ms)) == L.EINVAL
    assert np.all(out == 7) and ms.value == -1.0


def test_python_signatures():
    from viprs_amd.model import ClumpThreshold
    from viprs_amd.plan import LDPlan
    from viprs_amd.stats import clump as C
    E = inspect.Parameter.empty
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert params(LDPlan.clump)[1:] == [("order", E), ("r2", E), ("member", None), ("dq_scale", 1.0)]
    assert callable(LDPlan.last_clump_ms)
    assert params(C.clump_host) == [("lb", E), ("ip", E), ("data", E), ("low_memory", E), ("order", E), ("r2", E),
                                    ("member", None), ("dq_scale", 1.0)]
    assert params(C.clump_order) == [("chisq", E), ("min_chisq", 0.0)]
    assert params(C.clump)[:6] == [("ld_mat_or_gdl", E), ("chisq", None), ("r2", 0.1), ("p1", 1.0), ("p2", 1.0), ("order", None)]
    assert "clump_fn" in dict(params(C.clump)) and "pruning" in C.clump.__doc__.lower()
    got = dict(params(ClumpThreshold.__init__))
    assert got["r2"] == (0.1, 0.2, 0.5, 0.8)
    assert got["p_thresholds"] == (5e-8, 1e-6, 1e-4, 1e-3, 1e-2, 0.05, 0.1, 0.5, 1.0)
    assert {"low_memory", "dequantize_on_the_fly", "device", "clump_fn"} <= set(got)
    for name in ("fit", "predict", "pseudo_validate", "select_best", "to_table"):
        assert callable(getattr(ClumpThreshold, name))
    assert params(ClumpThreshold.pseudo_validate)[1:] == [("validation_std_beta", None), ("validation_ld", None)]
    assert params(ClumpThreshold.select_best)[1:] == [("validation_gdl", None), ("criterion", "validation")]
