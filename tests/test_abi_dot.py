"""The C ABI of the LD product (include/viprs_hip.h): the three entry points are declared with the documented argument lists,
exported by the built library and bound in viprs_amd/_lib.py; argument checks that need no device."""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_plan_dot": "viprs_plan* plan, int float_dtype, int n_cols, const void* b_host, void* y_host, "
                      "double dq_scale, int include_diagonal",
    "viprs_state_dot": "viprs_state* state, int field, double dq_scale, int include_diagonal, void* y_host",
    "viprs_plan_last_dot_ms": "viprs_plan* plan, double* ms",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_documented_argument_lists():
    text = open(HEADER).read()
    for name, args in DECLARED.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name
    # the order contract sits with the declarations
    assert "D(L) = ceil((L + 1) / (64 V)) + log2(V) + 6" in text


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"viprs_plan_dot": [vp, i, i, vp, vp, d, i], "viprs_state_dot": [vp, i, d, i, vp],
            "viprs_plan_last_dot_ms": [vp, ctypes.POINTER(d)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name


def test_null_arguments_are_refused_before_any_device_work():
    from viprs_amd import _lib as L
    y = np.full(4, 7.0, dtype=np.float32)
    ms = ctypes.c_double(-1.0)
    assert L.lib.viprs_plan_dot(None, L.F32, 1, y.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), 1.0, 1) == L.EINVAL
    assert "plan" in L.last_error()
    assert L.lib.viprs_state_dot(None, L.FIELD_ETA, 1.0, 1, y.ctypes.data_as(ctypes.c_void_p)) == L.EINVAL
    assert L.lib.viprs_plan_last_dot_ms(None, ctypes.byref(ms)) == L.EINVAL
    assert np.all(y == 7.0) and ms.value == -1.0


def test_python_handles_expose_the_product():
    from viprs_amd.plan import DeviceState, LDPlan
    assert callable(LDPlan.dot) and callable(LDPlan.last_dot_ms) and callable(DeviceState.dot)
