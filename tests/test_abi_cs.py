"""The C ABI of PRS-CS (include/viprs_hip.h): the entry points are declared with the documented argument lists, the header
states the variates, the update, the sums, the refusals and what is not built, the symbols are exported and bound in
viprs_amd/_lib.py; argument checks that need no device; the Python signatures; the sweep's sources are untouched."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "viprs_hip.h")

DECLARED = {
    "viprs_state_cs_variates": "viprs_state* state, uint64_t seed, uint64_t draw_index, const int32_t* active_model_idx, int n_active",
    "viprs_state_cs_update": "viprs_state* state, int n, const double* params, double psi_max, uint64_t seed, uint64_t draw_index, "
                             "int flags, int sync",
    "viprs_state_cs_sums": "viprs_state* state, int n, const int32_t* cols, double* out",
    "viprs_state_cs_upload": "viprs_state* state, int which, const void* host",
    "viprs_state_cs_download": "viprs_state* state, int which, void* host",
    "viprs_plan_last_cs_ms": "viprs_plan* plan, double* variates_ms, double* update_ms",
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
    for piece in ("counter = (j, g + 2^31, low 32 bits of draw_index, high 32 bits of draw_index)",
                  "ub = (2 (x0 >> 9) + 1) * 2^-24", "r = sqrtf(-2 logf(u1))", "z1 = r * cospif(2 u2); z2 = r * sinpif(2 u2)",
                  "e = -logf(u3)", "g15 = 0.5 z2 z2 + e", "delta = g15 / (psi_old + phi)", "lam = 2 delta",
                  "s = |eta| sqrt(n_j / (lam sigma2))", "y = z1 z1", "A = s + (y + sqrt(y (4 lam s + y))) / (2 lam)",
                  "psi = (ub (A + s) <= A) ? A : s s / A", "psi32 = (float)psi; delta32 = (float)delta; p = (double)psi32",
                  "mu_mult = (float)(p / (1 + p)); half_var_tau = (float)(n_j (1 + 1 / p) / (2 sigma2)); u_logs = 32.0f",
                  "[0] sum eta^2 / psi [1] sum n_j eta^2 / psi [2] sum delta [3] sum psi",
                  "enum viprs_cs_buffer { VIPRS_CS_PSI = 0, VIPRS_CS_DELTA = 1, VIPRS_CS_UB = 2, VIPRS_CS_Z1 = 3, VIPRS_CS_Z2 = 4, "
                  "VIPRS_CS_E = 5, VIPRS_CS_BUFFER_COUNT = 6 }",
                  "#define VIPRS_CS_KEEP_VARIATES 1", "#define VIPRS_CS_PREPARE_ONLY 2", "#define VIPRS_N_CS_SUMS 4",
                  "REFUSALS, each VIPRS_EINVAL before any launch, outputs untouched", "NOT BUILT: a != 1 or b != 1/2",
                  "cap 256 workgroups", "without LDS or atomics"):
        assert piece in flat, piece
    # the LDpred2 section keeps its declarations
    assert "enum viprs_gibbs_buffer { VIPRS_GIBBS_UNIF = 0, VIPRS_GIBBS_NOISE = 1, VIPRS_GIBBS_MEAN_SUM = 2" in flat
    assert "VIPRS_FIELD_COUNT = 10," in text and "#define VIPRS_N_ENET_SUMS 6" in text


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
    pd = ctypes.POINTER(d)
    want = {"viprs_state_cs_variates": [vp, u64, u64, vp, i], "viprs_state_cs_update": [vp, i, vp, d, u64, u64, i, i],
            "viprs_state_cs_sums": [vp, i, vp, vp], "viprs_state_cs_upload": [vp, i, vp], "viprs_state_cs_download": [vp, i, vp],
            "viprs_plan_last_cs_ms": [vp, pd, pd]}
    assert set(want) == set(DECLARED)
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name
    assert (L.CS_PSI, L.CS_DELTA, L.CS_UB, L.CS_Z1, L.CS_Z2, L.CS_E) == (0, 1, 2, 3, 4, 5)
    assert (L.CS_KEEP_VARIATES, L.CS_PREPARE_ONLY, L.N_CS_SUMS) == (1, 2, 4)


def test_bad_arguments_are_refused_before_any_device_work():
    from viprs_amd import _lib as L
    buf = np.full(4, 7.0)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    params = np.array([0.0, 1.0, 1.0])
    pp = params.ctypes.data_as(ctypes.c_void_p)
    assert L.lib.viprs_state_cs_variates(None, 1, 2, None, 0) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_cs_update(None, 1, pp, 1.0, 1, 2, 0, 1) == L.EINVAL and "state" in L.last_error()
    assert L.lib.viprs_state_cs_sums(None, 1, None, p) == L.EINVAL and "state" in L.last_error()
    for which in range(6):
        assert L.lib.viprs_state_cs_upload(None, which, p) == L.EINVAL and "state" in L.last_error()
        assert L.lib.viprs_state_cs_download(None, which, p) == L.EINVAL and "state" in L.last_error()
    v, u = ctypes.c_double(-3.0), ctypes.c_double(-4.0)
    assert L.lib.viprs_plan_last_cs_ms(None, ctypes.byref(v), ctypes.byref(u)) == L.EINVAL and "null" in L.last_error()
    assert np.all(buf == 7.0) and (v.value, u.value) == (-3.0, -4.0) and params.tolist() == [0.0, 1.0, 1.0]


def test_python_signatures():
    from viprs_amd.model import ClumpThreshold, PRSCS
    from viprs_amd.plan import DeviceState, LDPlan
    from viprs_amd.stats import cs as CS
    E = inspect.Parameter.empty
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert params(DeviceState.cs_variates)[1:] == [("seed", E), ("draw_index", E), ("active_model_idx", None)]
    assert params(DeviceState.cs_update)[1:] == [("params", E), ("psi_max", 1.0), ("seed", 0), ("draw_index", 0),
                                                 ("keep_variates", False), ("prepare_only", False), ("sync", True)]
    assert params(DeviceState.cs_sums)[1:] == [("cols", None)]
    assert params(DeviceState.cs_download)[1:] == [("which", E)] and params(DeviceState.cs_upload)[1:] == [("which", E), ("array", E)]
    assert callable(LDPlan.last_cs_ms)
    assert params(CS.cs_variates_host) == [("seed", E), ("draw_index", E), ("m", E), ("cols", E)]
    assert params(CS.gig_half_from_variates) == [("a", E), ("b", E), ("z", E), ("u", E)]
    assert [n for n, _ in params(CS.cs_update_host)] == ["n_per_snp", "eta", "psi", "delta", "mu_mult", "half_var_tau", "u_logs",
                                                        "params", "psi_max", "variates", "prepare_only"]
    assert [n for n, _ in params(CS.cs_sums_host)] == ["n_per_snp", "eta", "psi", "delta", "cols"]
    assert callable(CS.cs_sigma2_draw) and callable(CS.cs_phi_draw)
    got = dict(params(PRSCS.__init__)[1:])
    for k, v in dict(gdl=E, phi=None, a=1.0, b=0.5, n_iter=1000, n_burnin=500, thin=5, seed=0, psi_max=1.0,
                     float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, sweep_fn=None,
                     comm=None).items():
        assert got[k] is v or got[k] == v, k
    for name in ("fit", "predict", "pseudo_validate", "select_best", "to_table"):
        assert callable(getattr(PRSCS, name))
    assert PRSCS.select_best is ClumpThreshold.select_best and PRSCS.predict is ClumpThreshold.predict


def test_the_sweep_sources_are_untouched():
    """PRS-CS adds no sweep kernel: the translation units of the Gibbs policy do not mention it, and the Makefile builds
    the new one."""
    csrc = os.path.join(ROOT, "viprs_amd", "csrc")
    for name in ("panel_gibbs.h", "estep_panel.h", "panel_models.h", "kernels_common.h", "launch_panel_gibbs.inc",
                 "launch_band_gibbs.inc"):
        text = open(os.path.join(csrc, name)).read()
        assert "PRS-CS" not in text and "VIPRS_CS_" not in text, name
    assert re.search(r"\babi_cs\.hip\b", open(os.path.join(csrc, "Makefile")).read())
    gibbs = open(os.path.join(csrc, "abi_gibbs.hip")).read()
    assert '#include "philox.h"' in gibbs and "0xD2511F53" not in gibbs          # one Philox for both streams
