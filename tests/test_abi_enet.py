"""The C ABI of the elastic-net sweep (include/viprs_hip.h): the entry points are declared with the documented argument
lists, the header states the update, the field aliases and the sums, the symbols are exported and bound in
viprs_amd/_lib.py; argument checks that need no device; the Python signatures."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_state_enet_sweep": "viprs_state* state, double dq_scale, const int32_t* active_model_idx, int n_active, int sync",
    "viprs_state_enet_sums": "viprs_state* state, int n, const int32_t* cols, double* out",
    "viprs_enet_route": "int grid, int ld_dtype, int dense, int ragged, int band_ok, int* route",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_documented_argument_lists():
    text = open(HEADER).read()
    for name, args in DECLARED.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name
    flat = _norm(text.replace("\n *", " "))
    for piece in ("t = fl(c_j * q_j)", "u = fl(std_beta_j - t)", "a = fl(|u| - pen_j)", "b = a > 0 ? copysign(a, u) : +0",
                  "d = fl(b - eta_old_j)", "var_gamma[j] = (b != 0) ? 1 : 0", "eta[j] = fl(eta_old_j + d)",
                  "q[k] = fma(R[j,k], dq_scale * d, q[k])", "There is no skip branch", "VIPRS_FIELD_U_LOGS is not read",
                  "VIPRS_FIELD_ENET_MULT = VIPRS_FIELD_MU_MULT", "VIPRS_FIELD_ENET_PENALTY = VIPRS_FIELD_SQRT_HALF_VAR_TAU",
                  "#define VIPRS_N_ENET_SUMS 6", "[0] max |eta_diff| (fmax: ignores NaN)", "[1] sum std_beta eta",
                  "[2] sum q eta", "[3] sum eta^2", "[4] sum pen |eta|", "[5] the number of eta != 0",
                  "a float64 state VIPRS_EUNSUPPORTED", "a mixture state VIPRS_EINVAL",
                  "never on the batched matrix-core kernel"):
        assert piece in flat, piece
    # the E-step's route keeps its arguments
    mt = re.search(r"\bint\s+viprs_sweep_route\s*\(([^)]*)\)\s*;", text)
    assert _norm(mt.group(1)) == ("int float_dtype, int model_kind, int width, int ld_dtype, int dense, int ragged, int band_ok, "
                                  "int grid_mfma, int f64_row_by_row, int* route")


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"viprs_state_enet_sweep": [vp, d, vp, i, i], "viprs_state_enet_sums": [vp, i, vp, vp],
            "viprs_enet_route": [i] * 5 + [ctypes.POINTER(i)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name
    assert L.N_ENET_SUMS == 6 and L.FIELD_ENET_MULT == L.FIELD_MU_MULT and L.FIELD_ENET_PENALTY == L.FIELD_SQRT_HALF_VAR_TAU


def test_bad_arguments_are_refused_before_any_device_work():
    from viprs_amd import _lib as L
    out = np.full(6, 7.0)
    pout = out.ctypes.data_as(ctypes.c_void_p)
    assert L.lib.viprs_state_enet_sweep(None, 1.0, None, 0, 1) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_enet_sums(None, 1, None, pout) == L.EINVAL and "null" in L.last_error()
    assert L.lib.viprs_enet_route(0, L.LD_F32, 1, 0, 1, None) == L.EINVAL and "null" in L.last_error()
    route = (ctypes.c_int * len(L.ROUTE_FIELDS))(*([-9] * len(L.ROUTE_FIELDS)))
    assert L.lib.viprs_enet_route(1, L.LD_F32, 0, 1, 0, route) == L.EUNSUPPORTED and "elastic-net" in L.last_error()
    assert L.lib.viprs_enet_route(1, L.LD_F64, 1, 0, 1, route) == L.EINVAL and "unsupported LD dtype" in L.last_error()
    assert list(route) == [-9] * len(L.ROUTE_FIELDS) and np.all(out == 7.0)


def test_python_signatures():
    from viprs_amd.model import ClumpThreshold, Lassosum
    from viprs_amd.plan import DeviceState
    from viprs_amd.stats import enet as EN
    E = inspect.Parameter.empty
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert params(DeviceState.enet_sweep)[1:] == [("dq_scale", 1.0), ("active_model_idx", None), ("sync", True)]
    assert params(DeviceState.enet_sums)[1:] == [("cols", None)]
    assert [n for n, _ in params(EN.enet_sweep_host)] == ["lb", "ip", "data", "low_memory", "std_beta", "mult", "penalty", "eta",
                                                          "q", "dq_scale"]
    assert params(EN.lambda_path) == [("lo", 0.001), ("hi", 0.1), ("n", 20)]
    assert params(EN.enet_objective) == [("sums", E), ("s", E)] and callable(EN.enet_sums_host)
    assert params(Lassosum.__init__)[1:] == [
        ("gdl", E), ("s", (0.2, 0.5, 0.9, 1.0)), ("lambdas", None), ("penalty_factor", None), ("tol", 1e-4), ("max_sweeps", 1000),
        ("float_precision", "float32"), ("low_memory", True), ("dequantize_on_the_fly", False), ("device", None),
        ("sweep_fn", None), ("comm", None)]
    for name in ("fit", "predict", "pseudo_validate", "select_best", "to_table"):
        assert callable(getattr(Lassosum, name))
    # shared with ClumpThreshold, not copied
    assert Lassosum.select_best is ClumpThreshold.select_best and Lassosum.predict is ClumpThreshold.predict
