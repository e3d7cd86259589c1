"""The C ABI of PRS-CSx (include/viprs_hip.h): the entry points are declared with the documented argument lists, the header
states the update in full, the symbols are exported and bound in viprs_amd/_lib.py; every refusal that needs no device; the
Python signatures; the sweep's and PRS-CS's sources are untouched."""
import ctypes
import inspect
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "viprs_hip.h")

DECLARED = {
    "viprs_csx_create": "viprs_csx** out, int n_pop, viprs_state* const* states, int64_t m_union, const int64_t* row_of",
    "viprs_csx_destroy": "viprs_csx* x",
    "viprs_csx_update": "viprs_csx* x, int n, const double* params, double psi_max, uint64_t seed, uint64_t draw_index, "
                        "int flags, int sync",
    "viprs_csx_sums": "viprs_csx* x, int n, const int32_t* cols, double* out",
    "viprs_csx_upload": "viprs_csx* x, int which, const void* host",
    "viprs_csx_download": "viprs_csx* x, int which, void* host",
    "viprs_csx_last": "viprs_csx* x, double* ms, int64_t* n_capped",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_documented_argument_lists_and_states_the_update():
    text = open(HEADER).read()
    for name, args in DECLARED.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name
    flat = _norm(text.replace("\n *", " "))
    for piece in ("psi_u ~ GIG(p = 1 - K_u / 2, 2 delta_u, B_u)", "g15 = 0.5 z2 z2 + e; delta = g15 / (psi_old + phi); lam = 2 delta",
                  "B = B + n_kr eta_kr eta_kr / sigma2_k", "A = s + (y + sqrt(y (4 lam s + y))) / (2 lam)",
                  "K >= 2 and B == 0: psi = 2^-40", "psi(x) = -alpha (cosh(x) - 1) - lambda (exp(x) - x - 1)",
                  "dpsi(x) = -alpha sinh(x) - lambda (exp(x) - 1)",
                  "lambda = 0.5 K - 1; omega = sqrt(lam B); alpha = sqrt(omega omega + lambda lambda) - lambda",
                  "sqrt(2 / (alpha + lambda)) if x > 2", "log(4 / (alpha + 2 lambda)) if x < 0.5",
                  "sqrt(4 / (alpha C1 + lambda)) if x > 2", "s = log(1 + ia + sqrt(ia ia + 2 ia))",
                  "only if lambda > 0: s = fmin(1 / lambda, s)", "no 1 / lambda is formed",
                  "td = t - re eta'; sd = s - pe theta; q = td + sd; norm = pe + q + re; cut1 = q / norm; cut2 = (q + re) / norm",
                  "counter = (u, g + 2^31 + (a + 1) 2^16, low 32 bits of draw_index, high 32 bits of draw_index)",
                  "x = -sd + q V if U < cut1; td - re log(V) if U < cut2; -sd + pe log(V) otherwise",
                  "accept when W gx <= exp(psi(x))", "THE ATTEMPT CAP IS 32", "0.177", "a global atomic add",
                  "lo = lambda / omega; psi = exp(x) (lo + sqrt(1 + lo lo)); if K > 2 (p < 0): psi = 1 / psi; psi = psi / sqrt(lam / B)",
                  "psi = psi < 2^-40 ? 2^-40 : psi; psi = psi > psi_max ? psi_max : psi",
                  "mu_mult = (float)(p / (1 + p)); half_var_tau = (float)(n_kr (1 + 1 / p) / (2 sigma2_k)); u_logs = 32.0f",
                  "gives the bits of viprs_state_cs_update", "ORDER ACROSS STREAMS", "[0] sum delta [1] sum psi",
                  "cap 256 workgroups", "at most 8192 workgroups of 256, no LDS",
                  "REFUSALS of viprs_csx_create, each VIPRS_EINVAL before any allocation: n_pop outside 1..8",
                  "G >= 2^16", "a union row carried by no population",
                  "enum viprs_csx_buffer { VIPRS_CSX_PSI = 0, VIPRS_CSX_DELTA = 1, VIPRS_CSX_ATTEMPTS = 2, VIPRS_CSX_BUFFER_COUNT = 3 }",
                  "#define VIPRS_CSX_MAX_POP 8", "#define VIPRS_CSX_MAX_ATTEMPTS 32", "#define VIPRS_N_CSX_SUMS 2",
                  "NOT BUILT: a != 1 or b != 1/2; joint-block draws; float64 states; several ranks; a math_mode = fast variant; "
                  "populations on different devices"):
        assert piece in flat, piece
    # the PRS-CS section keeps its declarations
    assert "#define VIPRS_CS_KEEP_VARIATES 1" in text and "#define VIPRS_N_CS_SUMS 4" in text


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, i64, d, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_uint64
    want = {"viprs_csx_create": [ctypes.POINTER(vp), i, ctypes.POINTER(vp), i64, vp], "viprs_csx_destroy": [vp],
            "viprs_csx_update": [vp, i, vp, d, u64, u64, i, i], "viprs_csx_sums": [vp, i, vp, vp],
            "viprs_csx_upload": [vp, i, vp], "viprs_csx_download": [vp, i, vp],
            "viprs_csx_last": [vp, ctypes.POINTER(d), ctypes.POINTER(i64)]}
    assert set(want) == set(DECLARED)
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name
    assert (L.CSX_PSI, L.CSX_DELTA, L.CSX_ATTEMPTS) == (0, 1, 2)
    assert (L.CSX_MAX_POP, L.CSX_MAX_ATTEMPTS, L.N_CSX_SUMS) == (8, 32, 2)


def test_bad_arguments_are_refused_before_any_device_work():
    from viprs_amd import _lib as L
    buf = np.full(4, 7.0)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    params = np.array([0.0, 1.0, 1.0])
    pp = params.ctypes.data_as(ctypes.c_void_p)
    row_of = np.zeros(4, dtype=np.int64)
    pr = row_of.ctypes.data_as(ctypes.c_void_p)
    states = (ctypes.c_void_p * 9)()
    h = ctypes.c_void_p(12345)
    for n_pop in (0, -1, 9, 1 << 20):
        assert L.lib.viprs_csx_create(ctypes.byref(h), n_pop, states, 4, pr) == L.EINVAL and "1..8" in L.last_error()
        assert h.value is None                                       # the output is cleared, nothing was created
        h = ctypes.c_void_p(12345)
    assert L.lib.viprs_csx_create(None, 1, states, 4, pr) == L.EINVAL and "null" in L.last_error()
    assert L.lib.viprs_csx_create(ctypes.byref(h), 1, None, 4, pr) == L.EINVAL and "null" in L.last_error()
    assert L.lib.viprs_csx_create(ctypes.byref(h), 1, states, 4, None) == L.EINVAL and "null" in L.last_error()
    assert L.lib.viprs_csx_create(ctypes.byref(h), 1, states, -1, pr) == L.EINVAL and "m_union" in L.last_error()
    assert L.lib.viprs_csx_create(ctypes.byref(h), 2, states, 4, pr) == L.EINVAL and "state" in L.last_error()   # null states
    assert L.lib.viprs_csx_update(None, 1, pp, 1.0, 1, 2, 0, 1) == L.EINVAL and "handle" in L.last_error()
    assert L.lib.viprs_csx_sums(None, 1, None, p) == L.EINVAL and "handle" in L.last_error()
    for which in range(3):
        assert L.lib.viprs_csx_upload(None, which, p) == L.EINVAL and "handle" in L.last_error()
        assert L.lib.viprs_csx_download(None, which, p) == L.EINVAL and "handle" in L.last_error()
    ms, nc = ctypes.c_double(-3.0), ctypes.c_int64(-4)
    assert L.lib.viprs_csx_last(None, ctypes.byref(ms), ctypes.byref(nc)) == L.EINVAL and "handle" in L.last_error()
    assert L.lib.viprs_csx_destroy(None) == L.OK
    assert np.all(buf == 7.0) and (ms.value, nc.value) == (-3.0, -4) and params.tolist() == [0.0, 1.0, 1.0]


def test_python_signatures():
    from viprs_amd.model import PRSCSx
    from viprs_amd.plan import DeviceCoupling
    from viprs_amd.stats import csx as CX
    E = inspect.Parameter.empty
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert params(DeviceCoupling.__init__)[1:] == [("states", E), ("row_of", E)]
    assert params(DeviceCoupling.update)[1:] == [("params", E), ("psi_max", 1.0), ("seed", 0), ("draw_index", 0),
                                                 ("keep_variates", False), ("prepare_only", False), ("sync", True)]
    assert params(DeviceCoupling.sums)[1:] == [("cols", None)] and params(DeviceCoupling.download)[1:] == [("which", E)]
    assert params(DeviceCoupling.upload)[1:] == [("which", E), ("array", E)] and callable(DeviceCoupling.last)
    assert params(CX.gig_host) == [("p", E), ("a", E), ("b", E), ("uniforms", E)]
    assert [n for n, _ in params(CX.csx_update_host)] == ["row_of", "n_per_snp", "eta", "psi", "delta", "members", "params",
                                                         "psi_max", "variates", "seed", "draw_index", "prepare_only"]
    assert [n for n, _ in params(CX.csx_sums_host)] == ["psi", "delta", "cols"]
    got = dict(params(PRSCSx.__init__)[1:])
    for k, v in dict(gdls=E, phi=None, a=1.0, b=0.5, n_iter=1000, n_burnin=500, thin=5, seed=0, psi_max=1.0,
                     float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, sweep_fn=None,
                     draws_fn=None, coupled_fn=None, keep_draws_log=False, comm=None).items():
        assert got[k] is v or got[k] == v, k
    for name in ("fit", "predict", "to_table", "meta_beta"):
        assert callable(getattr(PRSCSx, name))
    for words in ("single-site", "genome-wide scalars", "Rao-Blackwellised", "a = 1, b = 1/2", "--meta"):
        assert words in inspect.getdoc(inspect.getmodule(PRSCSx)), words


def test_the_sweep_and_prs_cs_sources_are_untouched():
    """PRS-CSx adds no sweep kernel and leaves the PRS-CS translation unit alone: one new translation unit, built by the
    Makefile with the library's -ffp-contract=off, on the library's one Philox."""
    csrc = os.path.join(ROOT, "viprs_amd", "csrc")
    for name in ("panel_gibbs.h", "estep_panel.h", "panel_models.h", "kernels_common.h", "launch_panel_gibbs.inc",
                 "launch_band_gibbs.inc", "abi_cs.hip", "abi_gibbs.hip", "estep_band.h"):
        text = open(os.path.join(csrc, name)).read()
        assert "PRS-CSx" not in text and "csx" not in text, name
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"\babi_csx\.hip\b", make) and "-ffp-contract=off" in make
    csx = open(os.path.join(csrc, "abi_csx.hip")).read()
    assert '#include "philox.h"' in csx and "0xD2511F53" not in csx and "__shared__ double red" in csx
    assert "cs_ensure_buffers" in csx and "hipStreamWaitEvent" in csx
