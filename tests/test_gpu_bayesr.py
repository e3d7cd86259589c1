"""GPU: the SBayesR sweep (viprs_state_bayesr_sweep: panel_bayesr.h in the panel sweep and the band kernel, the kernels of
abi_bayesr.hip) against the host definition -- the uniforms `==` the host's Philox, the normals within the bound measured
for the LDpred2 normals, the sweep `==` the C replay (tests/bayesr_replay.c) fed the draws the device used, for every role
of the panel sweep and windowed LD, with inputs that differ from SNP to SNP; the sums, the accumulators, determinism,
`SBayesR.fit()` against the same fit on the host; the refusals."""
import ctypes
import functools

import numpy as np
import pytest

from tests import bayesr_replay as R
from tests.test_band import _inputs as band_inputs, banded_ld, dense_beside_banded
from tests.test_gpu_enet import _too_wide_a_band
from tests.test_gpu_gibbs import Z_TOL
from viprs_amd.stats import bayesr as B
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
SIZES = [2370, 1601, 130, 64, 1]         # tests/test_gpu_panel_roles.py: large team, medium team, partial panel, one panel, one row
FIELDS = ("eta", "q", "eta_diff", "var_mu", "var_gamma")
INPUTS = ("mu_mult", "sqrt_half_var_tau", "u_logs", "log_null_pi")
SEED = 0x5DEECE66D1234567


@functools.lru_cache(maxsize=None)
def _problem(low_memory, ld_dtype, sizes=tuple(SIZES)):
    ld, ss, inp = syn.make_problem(sizes=list(sizes), low_memory=low_memory, ld_dtype=ld_dtype, seed=53, kind="longrange")
    return ld, inp.std_beta, ss.n_per_snp


def _start(m, K):
    """The inputs of tests/bayesr_replay.py (they differ from SNP to SNP) and a state: eta = q = 0, junk in the outputs."""
    rng = np.random.default_rng(17)
    inputs = dict(zip(INPUTS, R.spread_inputs(m, K)))
    st = dict(eta=np.zeros(m, np.float32), q=np.zeros(m, np.float32), eta_diff=rng.standard_normal(m).astype(np.float32),
              var_mu=rng.standard_normal((m, K)).astype(np.float32), var_gamma=rng.standard_normal((m, K)).astype(np.float32))
    return inputs, st


def _open(ld, std_beta, inputs, st0, math_mode="exact"):
    from viprs_amd.plan import DeviceState, LDPlan
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, math_mode=math_mode)
    st = DeviceState(plan, "float32", model="mixture", width=st0["var_mu"].shape[1], placement="off")
    st.upload("std_beta", std_beta)
    st.set_n_per_snp(np.full(ld.m, 1e5))
    for k, a in inputs.items():
        st.upload(k, a)
    for k in FIELDS:
        st.upload(k, st0[k])
    return plan, st


def _device(ld, std_beta, inputs, st0, sweeps, seed=SEED, math_mode="exact"):
    """`sweeps` sweeps with draw_index 0, 1, ...: the final fields + k*, and the draws every sweep used."""
    plan, st = _open(ld, std_beta, inputs, st0, math_mode)
    try:
        draws = []
        for i in range(sweeps):
            st.bayesr_sweep(ld.dq_scale, seed=seed, draw_index=i)
            draws.append((st.bayesr_download("unif"), st.bayesr_download("z")))
        assert plan.effective_math_mode() == "exact"
        out = {k: st.download(k) for k in FIELDS}
        out["kstar"] = st.bayesr_download("kstar")
        st.close()
        return out, draws
    finally:
        plan.close()


def _replay(ld, std_beta, inputs, st0, draws):
    eta, q = st0["eta"].copy(), st0["q"].copy()
    for unif, z in draws:
        ed, mu, gam, ks = R.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, std_beta,
                                         *[inputs[k] for k in INPUTS], unif, z, eta, q, ld.dq_scale)
    return dict(eta=eta, q=q, eta_diff=ed, var_mu=mu, var_gamma=gam, kstar=ks)


def _assert_equal(got, want):
    for k in FIELDS + ("kstar",):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def _assert_draws_are_the_hosts(draws, m, seed=SEED):
    for i, (unif, z) in enumerate(draws):
        hu, hz = B.bayesr_draws_host(seed, i, m)
        assert np.array_equal(unif, hu), i
        assert np.all(np.abs(z.astype(np.float64) - hz.astype(np.float64)) <= Z_TOL), i


def test_draws_against_the_host(gpu):
    """2^20 SNPs: U `==` the host's, z within the bound EXPERIMENTS.md 6.28 records for the Gibbs normals (the same formula
    on the same device functions), its sign the sign the integers give cos(2 pi u2)."""
    from viprs_amd.plan import DeviceState, LDPlan
    m = 2 ** 20
    idx = 2 ** 40 + 5
    plan = LDPlan(np.arange(m, dtype=np.int32), np.arange(m + 1, dtype=np.int64), np.ones(m, dtype=np.float32), False)
    try:
        st = DeviceState(plan, "float32", model="mixture", width=3, placement="off")
        st.set_n_per_snp(np.full(m, 1e5))
        st.bayesr_draws(SEED, idx)
        assert plan.last_bayesr_draws_ms() > 0
        unif, z = st.bayesr_download("unif"), st.bayesr_download("z")
        assert not st.bayesr_download("kstar").any()                       # created zeroed, no sweep yet
        st.close()
    finally:
        plan.close()
    hu, hz = B.bayesr_draws_host(SEED, idx, m)
    assert np.array_equal(unif, hu)
    k2 = 2 * (B.bayesr_words_host(SEED, idx, m)[:, 2].astype(np.int64) >> 9) + 1
    assert np.array_equal(z > 0, (k2 < 2 ** 22) | (k2 > 3 * 2 ** 22)) and np.all(z != 0)
    err = float(np.abs(z.astype(np.float64) - hz.astype(np.float64)).max())
    print(f"max |z_dev - z_host| over 2^20 draws: {err:.3e} (bound {Z_TOL:.3e})")
    assert err <= Z_TOL


@pytest.mark.parametrize("K", [1, 3], ids=["K1", "K3"])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8, np.int16], ids=["f32", "i8", "i16"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_every_role_of_the_sweep(gpu, low_memory, ld_dtype, K, monkeypatch):
    """Two sweeps (the second starts from the eta, q the first stored) over the five panel roles with per-SNP inputs; every
    outcome k* = 0 .. K occurs in every block of 64 or more SNPs in both sweeps."""
    ld, std_beta, _ = _problem(low_memory, ld_dtype)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")      # teams of 8: the large class takes the narrow team strips
    inputs, st0 = _start(ld.m, K)
    got, draws = _device(ld, std_beta, inputs, st0, 2)
    _assert_draws_are_the_hosts(draws, ld.m)
    first = _replay(ld, std_beta, inputs, st0, draws[:1])
    want = _replay(ld, std_beta, inputs, st0, draws)
    for w in (first, want):
        assert R.every_outcome_in_every_block(w["kstar"], ld.block_start, K)
    assert not np.array_equal(first["eta"], want["eta"])
    _assert_equal(got, want)


def test_first_sweep_alone(gpu):
    """One sweep from eta = q = 0 (what the two-sweep test cannot tell from a wrong eta store)."""
    ld, std_beta, _ = _problem(True, np.int8)
    inputs, st0 = _start(ld.m, 3)
    got, draws = _device(ld, std_beta, inputs, st0, 1)
    _assert_equal(got, _replay(ld, std_beta, inputs, st0, draws))


@pytest.mark.parametrize("K", [1, 3], ids=["K1", "K3"])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8, np.int16], ids=["f32", "i8", "i16"])
@pytest.mark.parametrize("m, wl, wr, jitter, seed", [(900, 40, 40, 0, 8), (2500, 90, 140, 60, 5)], ids=["band", "ragged"])
def test_windowed_ld(gpu, m, wl, wr, jitter, seed, ld_dtype, K):
    """The band kernel (symmetric form: the upper form's instantiation is not shipped, see test_refusals_launch_nothing)."""
    ld = banded_ld(m, wl, wr, False, ld_dtype, seed=seed, jitter=jitter)
    ss, _ = band_inputs(m, seed=4)
    inputs, st0 = _start(m, K)
    got, draws = _device(ld, ss.std_beta, inputs, st0, 2)
    want = _replay(ld, ss.std_beta, inputs, st0, draws)
    assert set(np.unique(want["kstar"])) == set(range(K + 1))
    _assert_equal(got, want)


def test_dense_blocks_beside_a_band(gpu):
    """One plan with a dense block (panel sweep) and a windowed component (band kernel): the prologue launch in front of
    both.  The plan is in math_mode = fast: the sweep is the exact kernel and says so."""
    ld = dense_beside_banded([90], 300, 20, False)
    ss, _ = band_inputs(ld.m, seed=16)
    inputs, st0 = _start(ld.m, 3)
    got, draws = _device(ld, ss.std_beta, inputs, st0, 2, math_mode="fast")
    want = _replay(ld, ss.std_beta, inputs, st0, draws)
    assert set(np.unique(want["kstar"][:90])) == set(range(4)) and set(np.unique(want["kstar"][90:])) == set(range(4))
    _assert_equal(got, want)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 2370])
def test_sums_in_the_order(gpu, m):
    from viprs_amd.plan import DeviceState, LDPlan
    rng = np.random.default_rng(m)
    K = 3
    ks = rng.integers(0, K + 1, m).astype(np.int32)
    eta = np.where(ks > 0, 0.01 * rng.standard_normal(m), 0).astype(np.float32)
    q, beta = (0.01 * rng.standard_normal(m)).astype(np.float32), (0.01 * rng.standard_normal(m)).astype(np.float32)
    plan = LDPlan(np.arange(m, dtype=np.int32), np.arange(m + 1, dtype=np.int64), np.ones(m, dtype=np.float32), False)
    try:
        st = DeviceState(plan, "float32", model="mixture", width=K, placement="off")
        st.set_n_per_snp(np.full(m, 1e5))
        st.upload("std_beta", beta)
        st.upload("eta", eta)
        st.upload("q", q)
        st.bayesr_upload("kstar", ks)
        got = st.bayesr_sums()
        st.close()
    finally:
        plan.close()
    want = B.bayesr_sums_host(ks, eta, q, beta, K)
    assert got.dtype == np.float64 and np.array_equal(got, want), (got, want)
    assert np.array_equal(got[:K + 1], np.bincount(ks, minlength=K + 1))


def test_accumulate_and_reset_mean(gpu):
    ld, std_beta, _ = _problem(True, np.int8, (1601, 130, 64, 1))
    inputs, st0 = _start(ld.m, 3)
    plan, st = _open(ld, std_beta, inputs, st0)
    try:
        rng = np.random.default_rng(2)
        mean, pip = rng.standard_normal(ld.m), rng.random(ld.m)
        st.bayesr_upload("mean_sum", mean)
        st.bayesr_upload("pip_sum", pip)
        for i in range(3):
            st.bayesr_sweep(ld.dq_scale, seed=SEED, draw_index=i)
            st.bayesr_accumulate()
            B.bayesr_accumulate_host(st.download("var_gamma"), st.download("var_mu"), mean, pip)
        for name, want in (("mean_sum", mean), ("pip_sum", pip)):
            got = st.bayesr_download(name)
            assert got.dtype == np.float64 and np.array_equal(got, want), name
        st.bayesr_reset_mean()
        assert not st.bayesr_download("mean_sum").any() and not st.bayesr_download("pip_sum").any()
        st.close()
    finally:
        plan.close()


def test_determinism_and_keep_draws(gpu):
    """Two states, same seed: identical bits after 3 sweeps.  Another seed: another eta.  A sweep under KEEP_DRAWS from the
    same start, with the draws a sweep left behind: that sweep again."""
    ld, std_beta, _ = _problem(True, np.float32)
    inputs, st0 = _start(ld.m, 3)
    a, da = _device(ld, std_beta, inputs, st0, 3)
    b, db = _device(ld, std_beta, inputs, st0, 3)
    for k in FIELDS + ("kstar",):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for (u1, z1), (u2, z2) in zip(da, db):
        assert np.array_equal(u1, u2) and np.array_equal(z1.view(np.uint32), z2.view(np.uint32))
    c, _ = _device(ld, std_beta, inputs, st0, 3, seed=SEED + 1)
    assert not np.array_equal(a["eta"], c["eta"])
    plan, st = _open(ld, std_beta, inputs, st0)
    try:
        st.bayesr_sweep(ld.dq_scale, seed=SEED, draw_index=4)
        one = {k: st.download(k) for k in FIELDS}
        one["kstar"] = st.bayesr_download("kstar")
        for k in FIELDS:
            st.upload(k, st0[k])
        st.bayesr_upload("kstar", np.full(ld.m, -1, dtype=np.int32))
        st.bayesr_sweep(ld.dq_scale, seed=99, draw_index=7, keep_draws=True)          # (seed and index are not used)
        two = {k: st.download(k) for k in FIELDS}
        two["kstar"] = st.bayesr_download("kstar")
        for k in FIELDS + ("kstar",):
            assert np.array_equal(one[k].view(np.uint32), two[k].view(np.uint32)), k
        # uploaded draws are what a KEEP_DRAWS sweep uses
        unif, z = B.bayesr_draws_host(3, 0, ld.m)
        for k in FIELDS:
            st.upload(k, st0[k])
        st.bayesr_upload("unif", unif)
        st.bayesr_upload("z", z)
        st.bayesr_sweep(ld.dq_scale, keep_draws=True)
        got = {k: st.download(k) for k in FIELDS}
        got["kstar"] = st.bayesr_download("kstar")
        _assert_equal(got, _replay(ld, std_beta, inputs, st0, [(unif, z)]))
        st.close()
    finally:
        plan.close()


E2E_CHROMS = {1: [300, 130], 2: [200, 64, 1]}           # 695 SNPs: the host sweep walks them in a fraction of a second


def test_sbayesr_fit_equals_the_host_fit(gpu):
    """20 iterations, two chains.  What differs between the device and the host backend by construction is z alone: the
    device forms it in float32 with its logf and cospif, the host in float64 (within Z_TOL of each other, as for LDpred2).
    Everything behind the draws -- the sweep, the sums in THE ORDER, the accumulators, the hyper-parameter draws of the host
    generator -- is defined bit for bit.  So the host fit is fed the draws the device used, and the tolerance that remains
    is none: the two fits are `==`."""
    from viprs_amd.model import SBayesR
    kw = dict(h2_init=0.3, n_iter=20, n_burnin=5, n_chains=2, seed=11, dequantize_on_the_fly=True)
    dev = SBayesR(R.model_gdl(E2E_CHROMS), keep_draws_log=True, **kw).fit()
    assert sorted(dev.draws_log) == list(range(20)) + [(1 << 32) + i for i in range(20)]
    for i, (unif, z) in dev.draws_log.items():
        hu, hz = B.bayesr_draws_host(11, i, dev.m)
        assert np.array_equal(unif, hu) and np.all(np.abs(z.astype(np.float64) - hz) <= Z_TOL)
    host = SBayesR(R.model_gdl(E2E_CHROMS), backend="host", draws_fn=lambda seed, i, m: dev.draws_log[i], **kw).fit()
    assert not dev.diverged.any() and not host.diverged.any()
    for c in host.post_mean_beta:
        assert np.array_equal(dev.post_mean_beta[c], host.post_mean_beta[c]), c
        assert np.array_equal(dev.pip[c], host.pip[c]), c
        assert dev.post_mean_beta[c].any() and np.all((dev.pip[c] > 0) & (dev.pip[c] <= 1.0 + 1e-6))
    assert dev.grid_table.equals(host.grid_table)
    for a, b in zip(dev.pi_history + dev.h2_history, host.pi_history + host.h2_history):
        assert np.array_equal(a, b)
    assert "PIP" in dev.to_table().columns


def test_from_plan_equals_the_loader_fit(gpu):
    """`SBayesR.from_plan` on the plan a loader-built model made: the same fit."""
    from viprs_amd.model import SBayesR
    kw = dict(n_iter=12, n_burnin=4, seed=5)
    a = SBayesR(R.model_gdl({1: [300, 130, 1]}), h2_init=0.3, dequantize_on_the_fly=True, **kw)
    b = SBayesR.from_plan(a._plan, a.std_beta[1], a._n_per_snp, a.dequantize_scale, 0.3, **kw)
    a.fit()
    b.fit()
    assert np.array_equal(a.post_mean_beta[1], b.post_mean_beta[1]) and np.array_equal(a.pip[1], b.pip[1])
    assert a.grid_table.equals(b.grid_table) and b.n_sweeps.tolist() == [12] and a.post_mean_beta[1].any()


CASES = ["float64", "spike_slab", "grid", "wide_mixture", "groups", "comm", "no_n_per_snp", "wide_band", "upper_band", "ld_i32",
         "keep_draws_first", "unknown_flag", "sums_first"]


@pytest.mark.parametrize("case", CASES)
def test_refusals_launch_nothing(gpu, case):
    """Each refusal is a ValueError (VIPRS_EINVAL) before any launch: the timing record does not move, the state's fields
    keep their bits."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, LDPlan
    if case == "wide_band":
        ld = _too_wide_a_band()
    elif case == "upper_band":
        ld = banded_ld(900, 40, 40, True, np.float32, seed=8)
    elif case == "ld_i32":
        ld, _, _ = _problem(False, np.int32, (130, 64, 1))
    else:
        ld, _, _ = _problem(False, np.float32, (130, 64, 1))
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)
    comm = None
    try:
        if case == "comm":                                   # (before the timed sweep: starting RCCL is no part of the check)
            from viprs_amd.parallel import RcclComm
            comm = RcclComm(rank=0, world_size=1, device=0)
        ok = DeviceState(plan, "float32", model="mixture", width=2, placement="off")
        if case in ("wide_band", "upper_band"):
            assert plan.info(L.INFO_N_RAGGED) == 1
        ok.e_step(1.0)                                       # one timed sweep first: the record must not move afterwards
        ms = plan.last_kernel_ms(0)
        n = len(plan.timing_history())
        kind = {"float64": dict(float_precision="float64", model="mixture", width=3), "spike_slab": {},
                "grid": dict(model="grid", width=2), "wide_mixture": dict(model="mixture", width=5)}.get(
                    case, dict(model="mixture", width=3))
        st = DeviceState(plan, placement="off", **kind)
        if case != "no_n_per_snp":
            st.set_n_per_snp(np.full(ld.m, 1e5))
        if case == "groups":
            st.set_groups([0, 130, ld.m])
        if case == "comm":
            st.set_comm(comm)
        rng = np.random.default_rng(5)
        names = [k for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult") + FIELDS]
        before = {}
        for k in names:
            a = rng.standard_normal(st._shape(k)).astype(st.dtype)
            before[k] = np.asfortranarray(a) if st.model == "grid" and a.ndim == 2 else a
            st.upload(k, before[k])
        if case == "unknown_flag":
            assert L.lib.viprs_state_bayesr_sweep(st._h, 1.0, 1, 2, 2, 1) == L.EINVAL and "unknown flag" in L.last_error()
        elif case == "sums_first":
            with pytest.raises(ValueError, match="SBayesR sums"):
                st.bayesr_sums()
            out = np.full(10, 7.0)                               # a refused call leaves the caller's buffer alone
            assert L.lib.viprs_state_bayesr_sums(st._h, out.ctypes.data_as(ctypes.c_void_p)) == L.EINVAL and np.all(out == 7.0)
        else:
            with pytest.raises(ValueError, match="SBayesR|unsupported LD dtype"):
                st.bayesr_sweep(1.0, keep_draws=case == "keep_draws_first")
        if case in ("float64", "spike_slab", "grid", "wide_mixture", "groups", "comm", "no_n_per_snp"):
            buf = np.zeros(ld.m * 8)
            for call in (lambda: st.bayesr_draws(1, 2), st.bayesr_sums, st.bayesr_accumulate, st.bayesr_reset_mean,
                         lambda: st.bayesr_download("unif")):
                with pytest.raises(ValueError, match="SBayesR"):
                    call()
            assert L.lib.viprs_state_bayesr_upload(st._h, 0, buf.ctypes.data_as(ctypes.c_void_p)) == L.EINVAL
        assert plan.last_kernel_ms(0) == ms and len(plan.timing_history()) == n
        for k in names:
            u = f"u{st.dtype.itemsize}"
            assert np.array_equal(st.download(k).view(u), before[k].view(u)), k
        if case == "comm":
            st.set_comm(None)
        st.close()
        ok.close()
    finally:
        plan.close()
        if comm is not None and hasattr(comm, "close"):
            comm.close()


def test_null_pointers_and_buffer_codes(gpu):
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState
    ld, std_beta, _ = _problem(False, np.float32, (130, 64, 1))
    inputs, st0 = _start(ld.m, 3)
    plan, st = _open(ld, std_beta, inputs, st0)
    try:
        buf = np.zeros(ld.m)
        p = buf.ctypes.data_as(ctypes.c_void_p)
        assert L.lib.viprs_state_bayesr_sums(st._h, None) == L.EINVAL and "null" in L.last_error()
        for which in (-1, 5):
            assert L.lib.viprs_state_bayesr_upload(st._h, which, p) == L.EINVAL and "buffer code" in L.last_error()
            assert L.lib.viprs_state_bayesr_download(st._h, which, p) == L.EINVAL and "buffer code" in L.last_error()
        assert L.lib.viprs_state_bayesr_upload(st._h, 0, None) == L.EINVAL and "null" in L.last_error()
        assert L.lib.viprs_state_bayesr_download(st._h, 0, None) == L.EINVAL and "null" in L.last_error()
        # states of other users do not grow, and their Gibbs / PRS-CS buffers are not this model's
        other = DeviceState(plan, "float32", model="grid", width=2, placement="off")
        with pytest.raises(ValueError, match="SBayesR"):
            other.bayesr_download("unif")
        other.close()
        st.close()
    finally:
        plan.close()
