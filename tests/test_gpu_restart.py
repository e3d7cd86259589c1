"""The negative-MSE restart of ONE chromosome of a per-chromosome batch fit (VIPRS.py:1025-1037) on the device path, where the
chromosome's state goes device -> host -> standard start -> device (`_pull_state` / `_push_state`), and the pieces around it
that need no GPU.

GPU: `VIPRSPerChromosome` (both LD forms) and `VIPRSMixPerChromosome` (both host forms) with one chromosome's marginal effects
blown up must be `==` the per-chromosome `VIPRS` / `VIPRSMix` fits run one after the other on the device, the restarted one
included.  The blow-up factor starts at the one of the CPU tests (x5 / x6, found with the oracle's kernel); the device
trajectory differs from the oracle's in the last bits, so if that factor does not make the SEQUENTIAL device fit restart the
next larger one of `FACTORS` is taken -- the batch fit is never consulted for the choice.

CPU: `VIPRSMixPerChromosome._restart_state` around a recording stand-in for `DeviceState` whose `upload` checks shapes as the
real one does (the restart used to push one chromosome's arrays into the merged state); `_lockstep._close` against `np.isclose`.
"""
import numpy as np
import pytest

from tests import test_per_chromosome as PC
from tests import test_per_chromosome_mix as PM
from tests.test_fit import loader_from_fixture

FACTORS = (5.0, 6.0, 8.0, 12.0, 20.0, 40.0)


def _blown_up(fx, bad, factor):
    from viprs_amd.data import ArrayDataLoader, SumstatsArrays
    gdl = loader_from_fixture(fx)
    ss = dict(gdl.sumstats_table)
    ss[bad] = SumstatsArrays(ss[bad].get_snp_pseudo_corr() * np.float32(factor), ss[bad].n_per_snp)
    return ArrayDataLoader(gdl.ld, ss)


def _restarting_input(fx, bad, first, fit_one):
    """The loader with the smallest factor of FACTORS (from `first` on) at which chromosome `bad` fitted ALONE restarts."""
    for factor in (f for f in FACTORS if f >= first):
        gdl = _blown_up(fx, bad, factor)
        one = fit_one(gdl.split_by_chromosome()[bad])
        if one.fix_params.get("sigma_epsilon") == 0.95:
            return gdl, factor
    raise AssertionError(f"no factor of {FACTORS} makes the sequential device fit of chromosome {bad} restart")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("low_memory", [True, False])
def test_restart_on_the_device_spike_slab(gpu, low_memory):
    from viprs_amd.model import VIPRS, VIPRSPerChromosome
    fx = np.load(PC.FX4)
    bad = int(fx["chroms"][1])
    kw = PC.model_kwargs(fx, e_step="hip")
    kw["low_memory"] = low_memory
    fit_one = lambda sub: VIPRS(sub, **kw).fit(max_iter=40, theta_0=PC.theta_of(fx))
    gdl, factor = _restarting_input(fx, bad, 5.0, fit_one)
    print(f"[restart, spike-and-slab, low_memory={low_memory}] factor {factor}")
    seq = {c: fit_one(sub) for c, sub in gdl.split_by_chromosome().items()}
    assert seq[bad].fix_params.get("sigma_epsilon") == 0.95, "the test input does not trigger the restart"
    assert all(seq[c].fix_params.get("sigma_epsilon") != 0.95 for c in seq if c != bad)
    model = VIPRSPerChromosome(gdl, **kw).fit(max_iter=40, theta_0=PC.theta_of(fx))
    assert list(model._plans) == ["*"]
    PC.check_identical_to_sequential(model, seq)
    assert model.sigma_epsilon[bad] == 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("host", ["vector", "scalar"])
def test_restart_on_the_device_mixture(gpu, host):
    from viprs_amd.model import VIPRSMix, VIPRSMixPerChromosome
    fx = np.load(PM.FXM)
    bad = int(fx["chroms"][1])
    kw = PM.model_kwargs(fx, e_step="hip")
    fit_one = lambda sub: VIPRSMix(sub, **kw).fit(max_iter=30, theta_0=PM.theta_of(fx))
    gdl, factor = _restarting_input(fx, bad, 6.0, fit_one)
    print(f"[restart, mixture, host={host}] factor {factor}")
    seq = {c: fit_one(sub) for c, sub in gdl.split_by_chromosome().items()}
    assert seq[bad].fix_params.get("sigma_epsilon") == 0.95, "the test input does not trigger the restart"
    assert all(seq[c].fix_params.get("sigma_epsilon") != 0.95 for c in seq if c != bad)
    model = VIPRSMixPerChromosome(gdl, host=host, **kw).fit(max_iter=30, theta_0=PM.theta_of(fx))
    assert list(model._plans) == ["*"]
    PM.check_identical_to_sequential(model, seq)
    assert model.sigma_epsilon[bad] == 0.95


# ---- CPU: the restart's round trip through a stand-in for the device state --------------------------------------------------
class RecordingState:
    """What `_pull_state` / `_push_state` / `_upload_log_var_tau` use of `DeviceState`: arrays of the MERGED plan, `upload`
    refusing any other shape or dtype (plan.py `DeviceState.upload`)."""

    def __init__(self, arrays, K):
        self.arrays = {k: np.array(v) for k, v in arrays.items()}
        self.m, self.K = self.arrays["eta"].shape[0], K
        self.uploads, self.log_var_tau = [], None

    def upload(self, name, array):
        want = self.arrays[name]
        if array.dtype != want.dtype:
            raise ValueError(f"Buffer dtype mismatch for {name}: expected {want.dtype}, got {array.dtype}")
        if tuple(array.shape) != want.shape:
            raise ValueError(f"{name}: expected shape {want.shape}, got {array.shape}")
        self.arrays[name] = np.array(array)
        self.uploads.append(name)

    def download(self, name, out=None):
        return self.arrays[name].copy()

    def set_log_var_tau(self, a):
        if a.shape != (self.m, self.K):
            raise ValueError(f"log_var_tau: expected shape ({self.m}, {self.K}), got {a.shape}")
        self.log_var_tau = np.array(a)


STATE = ("var_gamma", "var_mu", "eta", "q", "eta_diff")


@pytest.mark.parametrize("holds_it", [True, False])
def test_mixture_restart_pushes_the_whole_merged_state(holds_it):
    """`_restart_state` of chromosome c, with c's model swapped in, must upload the state of EVERY chromosome this rank holds:
    c at the standard start, the others as they were -- also on a rank that does not hold c at all (nothing of its own changes)."""
    fx = np.load(PM.FXM)
    model = PM.build(fx).fit(max_iter=3, theta_0=PM.theta_of(fx))
    chroms = sorted(model.shapes)
    g = 1
    c = model.groups[g]
    if not holds_it:                                  # this rank's share: every chromosome but c
        model.shapes = {k: v for k, v in model.shapes.items() if k != c}
    held = sorted(model.shapes)
    assert (c in held) == holds_it and len(held) >= 2 and len(chroms) == 3
    seg, off = {}, 0
    for k in held:
        seg[k] = (off, off + model.shapes[k])
        off += model.shapes[k]
    dev = RecordingState({n: np.concatenate([getattr(model, n)[k] for k in held]) for n in STATE}, model.K)
    before = {n: dev.arrays[n].copy() for n in STATE}
    # the device path: no CPU kernel hook, one merged plan
    model._e_step_fn, model._merged, model._seg, model._dstate = None, True, seg, {"*": dev}
    with model._as_model(g):
        model._restart_state(PM.theta_of(fx), None)
        pi = np.asarray(model.pi)
    assert model._cur is None
    assert sorted(dev.uploads) == sorted(STATE) and dev.log_var_tau is not None
    for k in held:
        a, b = seg[k]
        if k == c:
            assert np.array_equal(dev.arrays["var_gamma"][a:b], np.broadcast_to(pi.astype(dev.arrays["var_gamma"].dtype), (b - a, model.K)))
            for n in ("var_mu", "eta", "q", "eta_diff"):
                assert not dev.arrays[n][a:b].any(), n
            assert before["var_mu"][a:b].any()                                  # (it had moved: the restart is visible)
        else:
            for n in STATE:
                assert np.array_equal(dev.arrays[n][a:b], before[n][a:b]), (k, n)
        assert np.array_equal(dev.log_var_tau[a:b], np.asarray(model._log_var_tau[k], dtype=np.float64) * np.ones((b - a, model.K)))


# ---- CPU: the stopping rules' isclose ---------------------------------------------------------------------------------------
def test_lockstep_close_is_isclose():
    from viprs_amd.model._lockstep import _close
    vals = np.array([0.0, 1.0, 1.0 + 5e-7, -1.0, 1e8, 1e8 + 1.0, -3.5e5, np.inf, -np.inf, np.nan])
    a, b = (x.ravel() for x in np.meshgrid(vals, vals))
    for atol, rtol in ((1e-6, 0.0), (1e-3, 1e-4), (0.0, 1e-4), (0.0, 0.0)):
        got = _close(a, b, atol, rtol)
        assert got.dtype == np.bool_
        want = np.isclose(a, b, atol=atol, rtol=rtol)
        assert np.array_equal(got, want), (atol, rtol, a[got != want], b[got != want])
    # the case the stopping rule meets: the first ELBO against prev_elbo = -inf, rtol > 0
    assert not _close(np.array([-1234.5]), np.array([-np.inf]), 1e-3, 1e-4)[0]
    assert _close(np.array([-np.inf]), np.array([-np.inf]), 1e-3, 1e-4)[0]
