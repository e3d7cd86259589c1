"""The C ABI of SuSiE fine-mapping (include/viprs_hip.h): the two entry points are declared with the documented argument
lists, exported by the built library and bound in viprs_amd/_lib.py; every argument check that needs no device.  (The checks
of the VALUES of z, log_prior and a prior-variance array read the plan's size and blocks: tests/test_gpu_susie.py holds them,
with the empty plan.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viprs_hip.h")

DECLARED = {
    "viprs_plan_susie": "viprs_plan* plan, int float_dtype, int L, const double* z_host, const double* log_prior_host, "
                        "const double* prior_variance_host, double prior_variance0, int estimate_prior_variance, "
                        "double dq_scale, double tol, int max_iter, int check_every, void* alpha_host, void* mu_host, "
                        "double* prior_variance_out, double* post_var_out, int32_t* block_iters, double* block_delta, "
                        "int32_t* block_status",
    "viprs_plan_last_susie_ms": "viprs_plan* plan, double* total_ms, int* steps, double* step_kernel_ms",
}


def _norm(s):
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", s)).strip()          # (a removed comment leaves its blank behind)


def test_header_declares_the_documented_argument_lists():
    text = open(HEADER).read()
    for phrase in ("Wang et al. 2020", "w_j = (0.5 * (r_j * r_j)) * s + log pi_j", "delta_it < tol", "NOT BUILT"):
        assert phrase in text                                             # the contract sits with the declarations
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, args in DECLARED.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in include/viprs_hip.h"
        assert _norm(mt.group(1)) == _norm(args), name


def test_library_exports_and_binds_the_symbols():
    from viprs_amd import _lib as L
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {"viprs_plan_susie": [vp, i, i, vp, vp, vp, d, i, d, d, i, i] + [vp] * 7,
            "viprs_plan_last_susie_ms": [vp, ctypes.POINTER(d), ctypes.POINTER(i), ctypes.POINTER(d)]}
    for name, args in want.items():
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is i and list(fn.argtypes) == args, name


class _FakePlan(ctypes.Structure):
    """Stands for a plan where the argument checks must return before they look at it."""
    _fields_ = [("bytes", ctypes.c_char * 64)]


CASES = {
    "plan": (dict(plan=None), "plan"), "dtype": (dict(dtype=7), "dtype"),
    "L_zero": (dict(L=0), "L must"), "L_33": (dict(L=33), "L must"),
    "tol_zero": (dict(tol=0.0), "tol"), "tol_negative": (dict(tol=-1e-4), "tol"), "tol_nan": (dict(tol=float("nan")), "tol"),
    "max_iter": (dict(max_iter=0), "max_iter"), "check_every": (dict(check_every=0), "check_every"),
    "dq_zero": (dict(dq=0.0), "dq_scale"), "dq_negative": (dict(dq=-1.0), "dq_scale"),
    "dq_inf": (dict(dq=float("inf")), "dq_scale"), "dq_nan": (dict(dq=float("nan")), "dq_scale"),
    "v0_negative": (dict(v0=-1.0), "prior variance"), "v0_inf": (dict(v0=float("inf")), "prior variance"),
    "v0_nan": (dict(v0=float("nan")), "prior variance"),
    "z": (dict(z=None), "null"), "alpha": (dict(alpha=None), "null"), "mu": (dict(mu=None), "null"),
}


@pytest.mark.parametrize("what", sorted(CASES))
def test_bad_arguments_are_refused_before_any_device_work(what):
    from viprs_amd import _lib as L
    fake = _FakePlan()
    z = np.ones(4)
    alpha, mu = np.full((4, 2), 7.0, dtype=np.float32, order="F"), np.full((4, 2), 7.0, dtype=np.float32, order="F")
    out = (np.full(2, -5.0), np.full(2, -5.0), np.full(1, -5, np.int32), np.full(1, -5.0), np.full(1, -5, np.int32))
    kw = dict(plan=ctypes.cast(ctypes.pointer(fake), ctypes.c_void_p), dtype=L.F32, L=2, z=z, v0=50.0, dq=1.0, tol=1e-4,
              max_iter=10, check_every=4, alpha=alpha, mu=mu)
    change, word = CASES[what]
    kw.update(change)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    rc = L.lib.viprs_plan_susie(kw["plan"], kw["dtype"], kw["L"], p(kw["z"]), None, None, kw["v0"], 1, kw["dq"], kw["tol"],
                                kw["max_iter"], kw["check_every"], p(kw["alpha"]), p(kw["mu"]), *(p(o) for o in out))
    assert rc == L.EINVAL
    assert word in L.last_error(), L.last_error()
    assert np.all(alpha == 7.0) and np.all(mu == 7.0) and all(np.all(o == -5) for o in out)
    assert bytes(fake.bytes) == b""                    # (the stand-in was not written either)


def test_last_susie_ms_refuses_null_arguments():
    from viprs_amd import _lib as L
    ms, n, step = ctypes.c_double(-1.0), ctypes.c_int(-1), ctypes.c_double(-1.0)
    assert L.lib.viprs_plan_last_susie_ms(None, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(step)) == L.EINVAL
    assert ms.value == -1.0 and n.value == -1 and step.value == -1.0


def test_python_handles_expose_the_fit():
    from viprs_amd.model import SuSiE
    from viprs_amd.plan import LDPlan, SusieInfo
    from viprs_amd.stats import susie as S
    E = inspect.Parameter.empty
    params = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    common = [("z", E), ("L", 10), ("prior_variance", 50.0), ("estimate_prior_variance", True), ("log_prior", None),
              ("dq_scale", 1.0), ("tol", 1e-4), ("max_iter", 100)]
    assert params(LDPlan.susie)[1:] == common + [("check_every", 4), ("float_precision", "float32")]
    assert params(S.susie_host) == [("lb", E), ("ip", E), ("data", E), ("low_memory", E)] + common + [
        ("float_precision", "float64"), ("callback", None)]
    assert callable(LDPlan.last_susie_ms)
    assert params(SuSiE.__init__)[1:] == [("gdl", E), ("L", 10), ("prior_variance", 50.0), ("estimate_prior_variance", True),
                                          ("prior_weights", None), ("float_precision", "float32"), ("low_memory", True),
                                          ("dequantize_on_the_fly", False), ("device", None), ("fit_fn", None)]
    assert params(SuSiE.fit)[1:] == [("tol", 1e-4), ("max_iter", 100)]
    assert params(SuSiE.credible_sets)[1:] == [("coverage", 0.95), ("min_abs_corr", 0.5), ("n_purity", 100), ("seed", 0)]
    for name in ("get_pip", "get_posterior_mean_beta", "elbo", "to_table", "predict"):
        assert callable(getattr(SuSiE, name))
    info = SusieInfo(np.zeros((3, 2)), np.zeros((3, 2)), [[1.0, 1.0]] * 2, [[0.5, 0.5]] * 2, [3, 9], [1e-6, 0.5], [0, 1],
                     [0, 2, 3], 1.5)
    assert not info.converged and info.ms == 1.5 and "L=2" in repr(info)
