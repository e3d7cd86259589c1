"""The C ABI of the LDpred2 Gibbs sweep (include/viprs_hip.h): the entry points are declared with the documented argument
lists, the header states the draws, the update, the refusals and what is not built, the symbols are exported and bound in
viprs_amd/_lib.py; argument checks that need no device; the Python signatures."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_state_gibbs_draws": "viprs_state* state, uint64_t seed, uint64_t draw_index, const int32_t* active_model_idx, int n_active",
    "viprs_state_gibbs_sweep": "viprs_state* state, double dq_scale, const int32_t* active_model_idx, int n_active, uint64_t seed, "
                               "uint64_t draw_index, int flags, int sync",
    "viprs_state_gibbs_upload": "viprs_state* state, int which, const void* host",
    "viprs_state_gibbs_download": "viprs_state* state, int which, void* host",
    "viprs_state_gibbs_accumulate": "viprs_state* state, const int32_t* active_model_idx, int n_active",
    "viprs_state_gibbs_reset_mean": "viprs_state* state",
    "viprs_gibbs_route": "int ld_dtype, int dense, int ragged, int band_ok, int* route",
    "viprs_plan_last_gibbs_draws_ms": "viprs_plan* plan, double* ms",
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
    for piece in ("0xD2511F53 and 0xCD9E8D57", "0x9E3779B9 and 0xBB67AE85", "10 rounds",
                  "key = (low 32 bits of seed, high 32 bits of seed)",
                  "counter = (j, g, low 32 bits of draw_index, high 32 bits of draw_index)",
                  "U = (2 (x0 >> 9) + 1) * 2^-24", "z = sqrtf(-2 logf(u1)) * cospif(2 u2)",
                  "noise = z * (1.0f / sqrtf(2.0f * half_var_tau[j, g]))",
                  "mu = fl(mu_mult_j * fl(std_beta_j - q_j))", "b = gamma > U_j ? fl(mu + noise_j) : +0",
                  "d = fl(b - eta_old_j)", "eta[j] = b", "There is no skip branch",
                  "enum viprs_gibbs_buffer { VIPRS_GIBBS_UNIF = 0, VIPRS_GIBBS_NOISE = 1, VIPRS_GIBBS_MEAN_SUM = 2",
                  "#define VIPRS_GIBBS_KEEP_DRAWS 1", "REFUSALS, each VIPRS_EINVAL before any launch",
                  "never on the batched matrix-core kernel", "NOT BUILT", "`sparse` option", "allow_jump_sign",
                  "mean_sum[j, g] += (double)var_gamma[j, g] * (double)var_mu[j, g]"):
        assert piece in flat, piece
    # the existing enums and routes keep their values and arguments
    assert "VIPRS_FIELD_COUNT = 10," in text
    mt = re.search(r"\bint\s+viprs_sweep_route\s*\(([^)]*)\)\s*;", text)
    assert _norm(mt.group(1)) == ("int float_dtype, int model_kind, int width, int ld_dtype, int dense, int ragged, int band_ok, "
                                  "int grid_mfma, int f64_row_by_row, int* route")
    mt = re.search(r"\bint\s+viprs_enet_route\s*\(([^)]*)\)\s*;", text)
    assert _norm(mt.group(1)) == "int grid, int ld_dtype, int dense, int ragged, int band_ok, int* route"


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
    want = {"viprs_state_gibbs_draws": [vp, u64, u64, vp, i], "viprs_state_gibbs_sweep": [vp, d, vp, i, u64, u64, i, i],
            "viprs_state_gibbs_upload": [vp, i, vp], "viprs_state_gibbs_download": [vp, i, vp],
            "viprs_state_gibbs_accumulate": [vp, vp, i], "viprs_state_gibbs_reset_mean": [vp],
            "viprs_gibbs_route": [i] * 4 + [ctypes.POINTER(i)], "viprs_plan_last_gibbs_draws_ms": [vp, ctypes.POINTER(d)]}
    assert set(want) == set(DECLARED)
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name
    assert (L.GIBBS_UNIF, L.GIBBS_NOISE, L.GIBBS_MEAN_SUM, L.GIBBS_KEEP_DRAWS) == (0, 1, 2, 1)
    assert (L.PANEL_GIBBS, L.BAND_GIBBS) == (5, 4)


def test_bad_arguments_are_refused_before_any_device_work():
    from viprs_amd import _lib as L
    buf = np.full(4, 7.0)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.lib.viprs_state_gibbs_sweep(None, 1.0, None, 0, 1, 2, 0, 1) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_gibbs_draws(None, 1, 2, None, 0) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_gibbs_accumulate(None, None, 0) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_gibbs_reset_mean(None) == L.EINVAL and "state" in L.last_error()
    for which in (L.GIBBS_UNIF, L.GIBBS_NOISE, L.GIBBS_MEAN_SUM):
        assert L.lib.viprs_state_gibbs_upload(None, which, p) == L.EINVAL and "state" in L.last_error()
        assert L.lib.viprs_state_gibbs_download(None, which, p) == L.EINVAL and "state" in L.last_error()
    ms = ctypes.c_double(-3.0)
    assert L.lib.viprs_plan_last_gibbs_draws_ms(None, ctypes.byref(ms)) == L.EINVAL and "null" in L.last_error()
    assert L.lib.viprs_gibbs_route(L.LD_F32, 1, 0, 1, None) == L.EINVAL and "null" in L.last_error()
    route = (ctypes.c_int * len(L.ROUTE_FIELDS))(*([-9] * len(L.ROUTE_FIELDS)))
    assert L.lib.viprs_gibbs_route(L.LD_F32, 0, 1, 0, route) == L.EINVAL and "Gibbs sweep" in L.last_error()
    assert L.lib.viprs_gibbs_route(L.LD_F64, 1, 0, 1, route) == L.EINVAL and "unsupported LD dtype" in L.last_error()
    assert list(route) == [-9] * len(L.ROUTE_FIELDS) and np.all(buf == 7.0) and ms.value == -3.0


def test_python_signatures():
    from viprs_amd.model import ClumpThreshold, LDpred2
    from viprs_amd.plan import DeviceState, LDPlan
    from viprs_amd.stats import gibbs as GB
    E = inspect.Parameter.empty
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert params(DeviceState.gibbs_sweep)[1:] == [("dq_scale", 1.0), ("active_model_idx", None), ("seed", 0), ("draw_index", 0),
                                                   ("keep_draws", False), ("sync", True)]
    assert params(DeviceState.gibbs_draws)[1:] == [("seed", E), ("draw_index", E), ("active_model_idx", None)]
    assert params(DeviceState.gibbs_accumulate)[1:] == [("active_model_idx", None)]
    assert params(DeviceState.gibbs_download)[1:] == [("which", E)] and params(DeviceState.gibbs_upload)[1:] == [("which", E),
                                                                                                              ("array", E)]
    assert callable(DeviceState.gibbs_reset_mean) and callable(LDPlan.last_gibbs_draws_ms)
    assert [n for n, _ in params(GB.gibbs_sweep_host)] == ["lb", "ip", "data", "low_memory", "std_beta", "mu_mult", "half_var_tau",
                                                           "u_logs", "unif", "noise", "eta", "q", "dq_scale"]
    assert params(GB.gibbs_draws_host) == [("seed", E), ("draw_index", E), ("half_var_tau", E), ("cols", None)]
    assert params(GB.philox4x32_10) == [("counter", E), ("key", E)] and callable(GB.gibbs_route)
    got = dict(params(LDpred2.__init__)[1:])
    for k, v in dict(gdl=E, mode="grid", p=None, h2=None, h2_init="ldsc", burn_in=None, num_iter=None, n_chains=30, seed=0,
                     float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, sweep_fn=None,
                     draws_fn=None, comm=None).items():
        assert got[k] is v or got[k] == v, k
    for name in ("fit", "predict", "pseudo_validate", "select_best", "to_table"):
        assert callable(getattr(LDpred2, name))
    # shared with ClumpThreshold, not copied
    assert LDpred2.select_best is ClumpThreshold.select_best and LDpred2.predict is ClumpThreshold.predict
