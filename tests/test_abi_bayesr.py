"""The C ABI of SBayesR (include/viprs_hip.h): the entry points are declared with the documented argument lists, the header
states the draws, the update, the sums, the refusals and what is not built, the symbols are exported and bound in
viprs_amd/_lib.py; argument checks that need no device; the Python signatures."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_state_bayesr_draws": "viprs_state* state, uint64_t seed, uint64_t draw_index",
    "viprs_state_bayesr_sweep": "viprs_state* state, double dq_scale, uint64_t seed, uint64_t draw_index, int flags, int sync",
    "viprs_state_bayesr_sums": "viprs_state* state, double* out",
    "viprs_state_bayesr_accumulate": "viprs_state* state",
    "viprs_state_bayesr_reset_mean": "viprs_state* state",
    "viprs_state_bayesr_upload": "viprs_state* state, int which, const void* host",
    "viprs_state_bayesr_download": "viprs_state* state, int which, void* host",
    "viprs_bayesr_route": "int ld_dtype, int dense, int ragged, int band_ok, int* route",
    "viprs_plan_last_bayesr_draws_ms": "viprs_plan* plan, double* ms",
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
    for piece in ("counter = (j, 2^30, low 32 bits of draw_index, high 32 bits of draw_index)",
                  "u_k = fma(t_k, t_k, u_logs_jk)", "(the null term last)", "gamma_k = fl(e_k / ssum)",
                  "sd_k = fl(0x1.6a09e6p-1f / sqrt_half_var_tau_jk)", "c_1 = gamma_1; c_k = fl(c_{k-1} + gamma_k)",
                  "k* = the smallest k in 1..K with U_j < c_k (strict), 0 if there is none", "b = k* ? fl(mu_{k*} + n_{k*}) : +0",
                  "eta[j] = b; kstar[j] = k*", "There is no skip branch", "in ONE allocation of the state",
                  "enum viprs_bayesr_buffer { VIPRS_BAYESR_UNIF = 0, VIPRS_BAYESR_Z = 1, VIPRS_BAYESR_KSTAR = 2, "
                  "VIPRS_BAYESR_MEAN_SUM = 3, VIPRS_BAYESR_PIP_SUM = 4, VIPRS_BAYESR_BUFFER_COUNT = 5 }",
                  "#define VIPRS_BAYESR_KEEP_DRAWS 1", "REFUSALS, each VIPRS_EINVAL before any launch", "NOT BUILT",
                  "robust parameterisation", "per-chromosome hyper-parameters"):
        assert piece in flat, piece
    # the existing enums keep their values
    assert "VIPRS_FIELD_COUNT = 10," in text
    assert "enum viprs_gibbs_buffer { VIPRS_GIBBS_UNIF = 0, VIPRS_GIBBS_NOISE = 1, VIPRS_GIBBS_MEAN_SUM = 2, VIPRS_GIBBS_BUFFER_COUNT = 3 }" in text
    assert "VIPRS_CS_BUFFER_COUNT = 6 }" in text


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
    want = {"viprs_state_bayesr_draws": [vp, u64, u64], "viprs_state_bayesr_sweep": [vp, d, u64, u64, i, i],
            "viprs_state_bayesr_sums": [vp, vp], "viprs_state_bayesr_accumulate": [vp], "viprs_state_bayesr_reset_mean": [vp],
            "viprs_state_bayesr_upload": [vp, i, vp], "viprs_state_bayesr_download": [vp, i, vp],
            "viprs_bayesr_route": [i] * 4 + [ctypes.POINTER(i)], "viprs_plan_last_bayesr_draws_ms": [vp, ctypes.POINTER(d)]}
    assert set(want) == set(DECLARED)
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name
    assert (L.BAYESR_UNIF, L.BAYESR_Z, L.BAYESR_KSTAR, L.BAYESR_MEAN_SUM, L.BAYESR_PIP_SUM) == (0, 1, 2, 3, 4)
    assert (L.BAYESR_KEEP_DRAWS, L.BAYESR_MAX_K, L.PANEL_BAYESR, L.BAND_BAYESR) == (1, 4, 6, 5)


def test_bad_arguments_are_refused_before_any_device_work():
    from viprs_amd import _lib as L
    buf = np.full(12, 7.0)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.lib.viprs_state_bayesr_sweep(None, 1.0, 1, 2, 0, 1) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_bayesr_draws(None, 1, 2) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_bayesr_sums(None, p) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_bayesr_accumulate(None) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_bayesr_reset_mean(None) == L.EINVAL and "state" in L.last_error()
    for which in range(5):
        assert L.lib.viprs_state_bayesr_upload(None, which, p) == L.EINVAL and "state" in L.last_error()
        assert L.lib.viprs_state_bayesr_download(None, which, p) == L.EINVAL and "state" in L.last_error()
    ms = ctypes.c_double(-3.0)
    assert L.lib.viprs_plan_last_bayesr_draws_ms(None, ctypes.byref(ms)) == L.EINVAL and "null" in L.last_error()
    assert L.lib.viprs_bayesr_route(L.LD_F32, 1, 0, 1, None) == L.EINVAL and "null" in L.last_error()
    route = (ctypes.c_int * len(L.ROUTE_FIELDS))(*([-9] * len(L.ROUTE_FIELDS)))
    assert L.lib.viprs_bayesr_route(L.LD_F32, 0, 1, 0, route) == L.EINVAL and "SBayesR sweep" in L.last_error()
    assert L.lib.viprs_bayesr_route(L.LD_F64, 1, 0, 1, route) == L.EINVAL and "unsupported LD dtype" in L.last_error()
    assert L.lib.viprs_bayesr_route(L.LD_I32, 0, 1, 1, route) == L.EINVAL and "unsupported LD dtype" in L.last_error()
    assert list(route) == [-9] * len(L.ROUTE_FIELDS) and np.all(buf == 7.0) and ms.value == -3.0


def test_python_signatures():
    from viprs_amd.model import ClumpThreshold, SBayesR
    from viprs_amd.plan import DeviceState, LDPlan
    from viprs_amd.stats import bayesr as BR
    E = inspect.Parameter.empty
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert params(DeviceState.bayesr_sweep)[1:] == [("dq_scale", 1.0), ("seed", 0), ("draw_index", 0), ("keep_draws", False),
                                                    ("sync", True)]
    assert params(DeviceState.bayesr_draws)[1:] == [("seed", E), ("draw_index", E)]
    assert params(DeviceState.bayesr_download)[1:] == [("which", E)]
    assert params(DeviceState.bayesr_upload)[1:] == [("which", E), ("array", E)]
    for name in ("bayesr_sums", "bayesr_accumulate", "bayesr_reset_mean"):
        assert callable(getattr(DeviceState, name))
    assert callable(LDPlan.last_bayesr_draws_ms)
    assert [n for n, _ in params(BR.bayesr_sweep_host)] == ["lb", "ip", "data", "low_memory", "std_beta", "mu_mult",
                                                            "sqrt_half_var_tau", "u_logs", "log_null_pi", "unif", "z", "eta", "q",
                                                            "dq_scale"]
    assert params(BR.bayesr_draws_host) == [("seed", E), ("draw_index", E), ("m", E)]
    assert callable(BR.bayesr_sums_host) and callable(SBayesR.from_plan)
    got = dict(params(SBayesR.__init__)[1:])
    for k, v in dict(gdl=E, gamma=(0.01, 0.1, 1.0), pi=(0.95, 0.02, 0.02, 0.01), h2_init="ldsc", n_iter=1000, n_burnin=250, thin=1,
                     n_chains=1, seed=0, float_precision="float32", low_memory=True, device=None, backend=None, sweep_fn=None,
                     draws_fn=None, comm=None).items():
        assert got[k] is v or got[k] == v, k
    for name in ("fit", "predict", "pseudo_validate", "to_table"):
        assert callable(getattr(SBayesR, name))
    assert SBayesR.predict is ClumpThreshold.predict
