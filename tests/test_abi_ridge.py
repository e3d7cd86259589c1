"""The C ABI of the ridge solve (include/viprs_hip.h): the two entry points are declared with the documented argument lists,
exported by the built library and bound in viprs_amd/_lib.py; every argument check that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_plan_solve_ridge": "viprs_plan* plan, int float_dtype, const void* b_host, const double* shift_host, "
                              "const void* x0_host, void* x_host, double dq_scale, double rtol, int max_iter, "
                              "int check_every, int32_t* block_iters, double* block_relres, int32_t* block_status",
    "viprs_plan_last_solve_ms": "viprs_plan* plan, double* total_ms, int* iterations",
}


def _norm(s):
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", s)).strip()          # (a removed comment leaves its blank behind)


def test_header_declares_the_documented_argument_lists():
    text = open(HEADER).read()
    assert "Paige & Saunders 1975" in text and "phibar <= rtol" in text        # the contract sits with the declarations
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, args in DECLARED.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"viprs_plan_solve_ridge": [vp, i, vp, vp, vp, vp, d, d, i, i, vp, vp, vp],
            "viprs_plan_last_solve_ms": [vp, ctypes.POINTER(d), ctypes.POINTER(i)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name


class _FakePlan(ctypes.Structure):
    """Stands for a plan where the argument checks must return before they look at it."""
    _fields_ = [("bytes", ctypes.c_char * 64)]


def _call(L, plan, dtype, b, shift, x, rtol=1e-5, max_iter=10, check_every=4, out=None):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    it, rr, st = out if out is not None else (None, None, None)
    return L.lib.viprs_plan_solve_ridge(plan, dtype, p(b), p(shift), None, p(x), 1.0, rtol, max_iter, check_every,
                                        p(it), p(rr), p(st))


@pytest.mark.parametrize("what", ["plan", "dtype", "rtol_zero", "rtol_negative", "rtol_nan", "max_iter", "check_every",
                                  "b", "shift", "x"])
def test_bad_arguments_are_refused_before_any_device_work(what):
    from viprs_amd import _lib as L
    fake = _FakePlan()
    plan = ctypes.cast(ctypes.pointer(fake), ctypes.c_void_p)
    b = np.ones(4, dtype=np.float32)
    shift = np.ones(4, dtype=np.float64)
    x = np.full(4, 7.0, dtype=np.float32)
    out = (np.full(1, -5, np.int32), np.full(1, -5.0), np.full(1, -5, np.int32))
    kw = dict(plan=plan, dtype=L.F32, b=b, shift=shift, x=x, out=out)
    word = {"plan": "plan", "dtype": "dtype", "rtol_zero": "rtol", "rtol_negative": "rtol", "rtol_nan": "rtol",
            "max_iter": "max_iter", "check_every": "check_every", "b": "null", "shift": "null", "x": "null"}[what]
    if what == "plan":
        kw["plan"] = None
    elif what == "dtype":
        kw["dtype"] = 7
    elif what.startswith("rtol"):
        kw["rtol"] = {"rtol_zero": 0.0, "rtol_negative": -1e-5, "rtol_nan": float("nan")}[what]
    elif what == "max_iter":
        kw["max_iter"] = 0
    elif what == "check_every":
        kw["check_every"] = 0
    else:
        kw[what] = None
    assert _call(L, **kw) == L.EINVAL
    assert word in L.last_error()
    assert np.all(x == 7.0) and all(np.all(o == -5) for o in out)
    assert bytes(fake.bytes) == b""                    # (the stand-in was not written either)


def test_last_solve_ms_refuses_null_arguments():
    from viprs_amd import _lib as L
    ms, n = ctypes.c_double(-1.0), ctypes.c_int(-1)
    assert L.lib.viprs_plan_last_solve_ms(None, ctypes.byref(ms), ctypes.byref(n)) == L.EINVAL
    assert ms.value == -1.0 and n.value == -1


def test_python_handles_expose_the_solve():
    import inspect
    from viprs_amd.model import LDPredInf
    from viprs_amd.plan import LDPlan, RidgeInfo
    assert list(inspect.signature(LDPlan.solve_ridge).parameters) == [
        "self", "b", "shift", "dq_scale", "rtol", "maxiter", "x0", "check_every"]
    assert inspect.signature(LDPlan.solve_ridge).parameters["check_every"].default == 4
    assert list(inspect.signature(LDPredInf.__init__).parameters)[:8] == [
        "self", "gdl", "h2", "float_precision", "low_memory", "dequantize_on_the_fly", "device", "solve_fn"]
    info = RidgeInfo([3, 0, 9], [1e-6, 0.0, 0.5], [0, 2, 1], 1.5)
    assert not info.converged and info.ms == 1.5 and RidgeInfo([1], [0.0], [2]).converged
