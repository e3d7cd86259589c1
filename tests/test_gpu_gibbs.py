"""GPU: the LDpred2 Gibbs sweep (viprs_state_gibbs_sweep: panel_gibbs.h in the panel sweep and the band kernel, the draws
kernel of abi_gibbs.hip) against the host definition -- the uniforms `==` the host's Philox, the normals within a measured
bound, the sweep `==` the C replay (tests/gibbs_replay.c) fed the draws the device used, for every role of the panel sweep,
windowed LD and grid states; the strict comparison, the accumulator, determinism, `LDpred2.fit()` against the same fit on the
host; the refusals."""
import functools

import numpy as np
import pytest

from tests import gibbs_replay as GR
from tests.test_band import _inputs as band_inputs, banded_ld, dense_beside_banded
from tests.test_gpu_enet import _too_wide_a_band
from viprs_amd.stats import gibbs as GB
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
SIZES = [2370, 1601, 130, 64, 1]         # tests/test_gpu_panel_roles.py: large team, medium team, partial panel, one panel, one row
FIELDS = ("eta", "q", "eta_diff", "var_mu", "var_gamma")
PAIRS = ((0.5, 0.2), (0.01, 0.2), (0.9, 0.4))           # (p, h2) of the three columns; column 1 is the one nobody sweeps
ACTIVE = [2, 0]
SEED = 0x5DEECE66D1234567

# The largest |z_dev - z_host| over the 2^20 draws of test_draws_against_the_host (z_host: float64 Box-Muller rounded to
# float32; z_dev: ocml's logf and cospif in float32), measured on an MI355X (EXPERIMENTS.md 6.28).  The bound of the test is
# four times that: logf and cospif are a few ulp each and the product compounds them.  It may not exceed 1e-5: |z| <= 5.9, a
# wrong formula is off by O(1).
Z_MEASURED = 4.768e-7
Z_TOL = 4 * Z_MEASURED
assert Z_TOL <= 1e-5


@functools.lru_cache(maxsize=None)
def _problem(low_memory, ld_dtype, sizes=tuple(SIZES)):
    ld, ss, inp = syn.make_problem(sizes=list(sizes), low_memory=low_memory, ld_dtype=ld_dtype, seed=53, kind="longrange")
    return ld, inp.std_beta, ss.n_per_snp


def _start(n_per_snp, pairs, junk_cols=()):
    """The chains' inputs and a state: eta = q = 0 (junk in `junk_cols`: columns nobody sweeps), junk in the three outputs."""
    m, G = n_per_snp.shape[0], len(pairs)
    rng = np.random.default_rng(17)
    inputs = dict(zip(("mu_mult", "half_var_tau", "u_logs"), GR.chain_inputs(n_per_snp, pairs)))
    st = {k: np.asfortranarray(rng.standard_normal((m, G)).astype(np.float32)) for k in FIELDS}
    for k in ("eta", "q"):
        keep = st[k].copy()
        st[k][...] = 0
        for g in junk_cols:
            st[k][:, g] = 0.01 * keep[:, g]
    return inputs, st


def _open(ld, std_beta, inputs, st0, math_mode="exact"):
    from viprs_amd.plan import DeviceState, LDPlan
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, math_mode=math_mode)
    st = DeviceState(plan, "float32", model="grid", width=st0["eta"].shape[1], placement="off")
    st.upload("std_beta", std_beta)
    for k, a in inputs.items():
        st.upload(k, a)
    for k in FIELDS:
        st.upload(k, st0[k])
    return plan, st


def _device(ld, std_beta, inputs, st0, sweeps, active=None, seed=SEED, math_mode="exact"):
    """`sweeps` sweeps with draw_index 0, 1, ...: the final fields and the draws every sweep used."""
    plan, st = _open(ld, std_beta, inputs, st0, math_mode)
    try:
        draws = []
        for i in range(sweeps):
            st.gibbs_sweep(ld.dq_scale, active_model_idx=active, seed=seed, draw_index=i)
            draws.append((st.gibbs_download("unif"), st.gibbs_download("noise")))
        assert plan.effective_math_mode() == "exact"
        out = {k: st.download(k) for k in FIELDS}
        st.close()
        return out, draws
    finally:
        plan.close()


def _replay(ld, std_beta, inputs, st0, draws, active=None):
    st = {k: v.copy(order="F") for k, v in st0.items()}
    for g in (active if active is not None else range(st0["eta"].shape[1])):
        eta, q = st["eta"][:, g].copy(), st["q"][:, g].copy()
        for unif, noise in draws:
            ed, mu, gam = GR.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, std_beta,
                                          inputs["mu_mult"][:, g], inputs["half_var_tau"][:, g], inputs["u_logs"][:, g],
                                          unif[:, g].copy(), noise[:, g].copy(), eta, q, ld.dq_scale)
        for k, v in zip(FIELDS, (eta, q, ed, mu, gam)):
            st[k][:, g] = v
    return st


def _assert_equal(got, want):
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def _assert_draws_are_the_hosts(draws, hvt, cols, seed=SEED):
    """U `==` the host's; the sign of the noise is the sign the integers give cos(2 pi u2); the noise within the bound."""
    m = hvt.shape[0]
    for i, (unif, noise) in enumerate(draws):
        w = GB.gibbs_words_host(seed, i, m, cols)
        hu, hn = GB.gibbs_draws_host(seed, i, hvt, cols)
        k2 = 2 * (w[..., 2].astype(np.int64) >> 9) + 1
        positive = (k2 < 2 ** 22) | (k2 > 3 * 2 ** 22)               # (k2 is odd: never on a zero of the cosine)
        for a, g in enumerate(cols):
            assert np.array_equal(unif[:, g], hu[:, g]), (i, g)
            assert np.array_equal(noise[:, g] > 0, positive[:, a]) and np.all(noise[:, g] != 0), (i, g)
            sd = np.float32(1.0) / np.sqrt(np.float32(2.0) * hvt[:, g])
            assert np.all(np.abs(noise[:, g].astype(np.float64) - hn[:, g]) <= Z_TOL * sd), (i, g)


def test_draws_against_the_host(gpu):
    """2^20 SNPs, one column, half_var_tau = 0.5: the noise is z itself."""
    from viprs_amd.plan import DeviceState, LDPlan
    m = 2 ** 20
    plan = LDPlan(np.arange(m, dtype=np.int32), np.arange(m + 1, dtype=np.int64), np.ones(m, dtype=np.float32), False)
    try:
        st = DeviceState(plan, "float32", model="grid", width=1, placement="off")
        hvt = np.full((m, 1), 0.5, dtype=np.float32, order="F")
        st.upload("half_var_tau", hvt)
        st.gibbs_draws(SEED, 2 ** 40 + 5)
        assert plan.last_gibbs_draws_ms() > 0
        unif, noise = st.gibbs_download("unif"), st.gibbs_download("noise")
        st.close()
    finally:
        plan.close()
    hu, hz = GB.gibbs_normals_host(SEED, 2 ** 40 + 5, m, [0])
    assert np.array_equal(unif, hu)
    k = unif.astype(np.float64) * 2.0 ** 24
    assert np.all((unif > 0) & (unif < 1)) and np.array_equal(k, np.round(k)) and np.all(k.astype(np.int64) % 2 == 1)
    k2 = 2 * (GB.gibbs_words_host(SEED, 2 ** 40 + 5, m, [0])[:, 0, 2].astype(np.int64) >> 9) + 1
    assert np.array_equal(noise[:, 0] > 0, (k2 < 2 ** 22) | (k2 > 3 * 2 ** 22)) and np.all(noise != 0)
    err = float(np.abs(noise.astype(np.float64) - hz.astype(np.float64)).max())
    print(f"max |z_dev - z_host| over 2^20 draws: {err:.3e} (bound {Z_TOL:.3e})")
    assert err <= Z_TOL
    z = noise[:, 0].astype(np.float64)
    assert abs(z.mean()) < 4.9e-3 and abs(z.var() - 1.0) < 6.9e-3           # (five standard errors, as for the host's)


def test_draws_of_a_column_depend_on_nothing_else(gpu):
    """Not on the other columns listed, not on the call that generated them (gibbs_draws or gibbs_sweep), not on the state."""
    ld, std_beta, n = _problem(True, np.float32, (1601, 130, 64, 1))
    inputs, st0 = _start(n, PAIRS, junk_cols=(1,))
    plan, st = _open(ld, std_beta, inputs, st0)
    try:
        st.gibbs_draws(SEED, 7, [2, 0])
        both = st.gibbs_download("unif"), st.gibbs_download("noise")
        assert not both[0][:, 1].any() and not both[1][:, 1].any()              # (created zeroed, column 1 never listed)
        st.gibbs_draws(SEED, 8, [0])                                             # column 2 keeps the draws of index 7
        st.gibbs_draws(SEED, 7, [0])
        for a, b in zip(both, (st.gibbs_download("unif"), st.gibbs_download("noise"))):
            assert np.array_equal(a, b)
        st.gibbs_sweep(ld.dq_scale, active_model_idx=[0], seed=SEED, draw_index=7)
        for a, b in zip(both, (st.gibbs_download("unif"), st.gibbs_download("noise"))):
            assert np.array_equal(a, b)
        assert np.array_equal(both[0], GB.gibbs_draws_host(SEED, 7, inputs["half_var_tau"], [2, 0])[0])
        st.close()
    finally:
        plan.close()


@pytest.mark.parametrize("width", [1, 3], ids=["width1", "grid3"])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8, np.int16], ids=["f32", "i8", "i16"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_every_role_of_the_sweep(gpu, low_memory, ld_dtype, width, monkeypatch):
    ld, std_beta, n = _problem(low_memory, ld_dtype)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")      # teams of 8: the large class takes the narrow team strips
    pairs, active, swept = ((PAIRS[0],), None, [0]) if width == 1 else (PAIRS, ACTIVE, ACTIVE)
    inputs, st0 = _start(n, pairs, junk_cols=() if width == 1 else (1,))
    got, draws = _device(ld, std_beta, inputs, st0, 3, None if active is None else np.array(active, dtype=np.int32))
    _assert_draws_are_the_hosts(draws, inputs["half_var_tau"], swept)
    want = _replay(ld, std_beta, inputs, st0, draws, swept)
    # the chain is exercised: every swept column ends neither empty nor full
    for g in swept:
        frac = np.count_nonzero(want["eta"][:, g]) / ld.m
        assert 0.10 <= frac <= 0.90, (g, frac)
    _assert_equal(got, want)
    if width > 1:
        for k in FIELDS:                             # column 1 keeps its uploaded bits
            assert np.array_equal(got[k][:, 1].view(np.uint32), st0[k][:, 1].view(np.uint32)), k
        for unif, noise in draws:
            assert not unif[:, 1].any() and not noise[:, 1].any()


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("m, wl, wr, jitter, seed", [(900, 40, 40, 0, 8), (2500, 90, 140, 60, 5)], ids=["band", "ragged"])
def test_windowed_ld(gpu, m, wl, wr, jitter, seed, low_memory, ld_dtype):
    ld = banded_ld(m, wl, wr, low_memory, ld_dtype, seed=seed, jitter=jitter)
    ss, _ = band_inputs(m, seed=4)
    inputs, st0 = _start(ss.n_per_snp, (PAIRS[0],))
    got, draws = _device(ld, ss.std_beta, inputs, st0, 2)
    want = _replay(ld, ss.std_beta, inputs, st0, draws)
    assert 0 < np.count_nonzero(want["eta"]) < m
    _assert_equal(got, want)


@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_dense_blocks_beside_a_band(gpu, low_memory):
    """One plan with a dense block (panel sweep) and a windowed component (band kernel), a grid state: the prologue launch
    with granules per model in front of both.  The plan is in math_mode = fast: the sweep is the exact kernel and says so."""
    ld = dense_beside_banded([90], 300, 20, low_memory)
    ss, _ = band_inputs(ld.m, seed=16)
    inputs, st0 = _start(ss.n_per_snp, PAIRS, junk_cols=(1,))
    got, draws = _device(ld, ss.std_beta, inputs, st0, 2, np.array(ACTIVE, dtype=np.int32), math_mode="fast")
    want = _replay(ld, ss.std_beta, inputs, st0, draws, ACTIVE)
    assert 0 < np.count_nonzero(want["eta"][:, 0]) < ld.m
    _assert_equal(got, want)


def test_strict_comparison(gpu):
    """Uploaded draws under KEEP_DRAWS: U_j == gamma_j leaves SNP j out, the next float below includes it."""
    ld, std_beta, n = _problem(False, np.float32, (130, 64, 1))
    inputs, st0 = _start(n, (PAIRS[0],))
    j = 150                                          # (inside the second block: its gamma depends on the draws in front of it)
    unif, noise = GB.gibbs_draws_host(3, 0, inputs["half_var_tau"])
    gamma = _replay(ld, std_beta, inputs, st0, [(unif, noise)])["var_gamma"][j, 0]
    assert 0 < gamma < 1
    plan, st = _open(ld, std_beta, inputs, st0)
    try:
        for u, included in ((gamma, False), (np.nextafter(gamma, np.float32(0)), True)):
            unif[j, 0] = u
            for k in FIELDS:
                st.upload(k, st0[k])
            st.gibbs_upload("unif", unif)
            st.gibbs_upload("noise", noise)
            st.gibbs_sweep(ld.dq_scale, seed=99, draw_index=5, keep_draws=True)
            assert np.array_equal(st.gibbs_download("unif"), unif) and np.array_equal(st.gibbs_download("noise"), noise)
            got = {k: st.download(k) for k in FIELDS}
            want = _replay(ld, std_beta, inputs, st0, [(unif, noise)])
            assert want["var_gamma"][j, 0] == gamma and (want["eta"][j, 0] != 0) == included
            _assert_equal(got, want)
        st.close()
    finally:
        plan.close()


def test_accumulate_and_reset_mean(gpu):
    ld, std_beta, n = _problem(True, np.int8, (1601, 130, 64, 1))
    inputs, st0 = _start(n, PAIRS, junk_cols=(1,))
    plan, st = _open(ld, std_beta, inputs, st0)
    try:
        junk = np.asfortranarray(np.random.default_rng(2).standard_normal((ld.m, 3)))
        junk[:, ACTIVE] = 0
        st.gibbs_upload("mean_sum", junk)
        want = junk.copy(order="F")
        for i in range(3):
            st.gibbs_sweep(ld.dq_scale, active_model_idx=ACTIVE, seed=SEED, draw_index=i)
            st.gibbs_accumulate(ACTIVE)
            gam, mu = st.download("var_gamma"), st.download("var_mu")
            for g in ACTIVE:
                want[:, g] += gam[:, g].astype(np.float64) * mu[:, g].astype(np.float64)
        got = st.gibbs_download("mean_sum")
        assert got.dtype == np.float64 and np.array_equal(got, want) and want[:, ACTIVE].any(axis=0).all()
        assert np.array_equal(got[:, 1].view(np.uint64), junk[:, 1].view(np.uint64))          # unlisted: untouched
        st.gibbs_reset_mean()
        assert not st.gibbs_download("mean_sum").any()
        st.close()
    finally:
        plan.close()


def test_determinism(gpu):
    """Two states, same seed: identical bits after 3 sweeps.  Another seed: another eta."""
    ld, std_beta, n = _problem(True, np.float32)
    inputs, st0 = _start(n, PAIRS, junk_cols=(1,))
    active = np.array(ACTIVE, dtype=np.int32)
    a, da = _device(ld, std_beta, inputs, st0, 3, active)
    b, db = _device(ld, std_beta, inputs, st0, 3, active)
    for k in FIELDS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for (u1, n1), (u2, n2) in zip(da, db):
        assert np.array_equal(u1, u2) and np.array_equal(n1.view(np.uint32), n2.view(np.uint32))
    c, _ = _device(ld, std_beta, inputs, st0, 3, active, seed=SEED + 1)
    assert not np.array_equal(a["eta"][:, 0], c["eta"][:, 0]) and not np.array_equal(a["eta"][:, 2], c["eta"][:, 2])


E2E_CHROMS = {1: [400, 330, 300], 2: [330, 300, 270, 64, 1]}     # 1 995 SNPs; blocks of a size the host sweep walks quickly


@pytest.mark.parametrize("mode", ["grid", "auto"])
def test_ldpred2_fit_equals_the_host_fit(gpu, mode):
    """Short chains, 3 columns, 1 995 SNPs: the device fit against the same fit driven by `gibbs_sweep_host`, fed the draws
    the device used (the normals of the two differ within the bound above; everything behind them is `==`)."""
    from viprs_amd.model import LDpred2
    kw = dict(mode=mode, h2_init=0.3, burn_in=5, num_iter=10, seed=11, dequantize_on_the_fly=True)
    kw.update(dict(p=(0.05, 0.5, 1.0), h2=(0.3,)) if mode == "grid" else dict(n_chains=3))
    dev = LDpred2(GR.model_gdl(E2E_CHROMS), keep_draws_log=True, **kw).fit()
    assert len(dev.draws_log) == 15
    host = LDpred2(GR.model_gdl(E2E_CHROMS), sweep_fn=GB.gibbs_sweep_host,
                   draws_fn=lambda seed, i, hvt, cols: dev.draws_log[i], **kw).fit()
    for c in host.post_mean_beta:
        assert np.array_equal(dev.post_mean_beta[c], host.post_mean_beta[c]), c
        assert dev.post_mean_beta[c].any()
    assert dev.grid_table.equals(host.grid_table)
    assert np.array_equal(dev.p_history, host.p_history) and np.array_equal(dev.h2_history, host.h2_history)
    if mode == "grid":
        rng = np.random.default_rng(11)
        vb = {c: np.asarray(b, dtype=np.float64) + 0.002 * rng.normal(size=b.shape[0]) for c, b in dev.std_beta.items()}
        dev.select_best(validation_gdl=vb, criterion="pseudo_validation")
        r = np.asarray(dev.validation_result["Pseudo_Validation_R2"])
        assert r.shape == (3,) and dev.best_model_idx == int(np.argmax(r)) and r.max() > 0


def test_from_plan_equals_the_loader_fit(gpu):
    """`LDpred2.from_plan` on the plan a loader-built model made (one chromosome of [130, 64] SNPs, int8 LD): the same fit."""
    from viprs_amd.model import LDpred2
    kw = dict(mode="auto", n_chains=3, burn_in=4, num_iter=4, seed=5)
    a = LDpred2(GR.model_gdl({1: [130, 64]}), h2_init=0.3, dequantize_on_the_fly=True, **kw)
    b = LDpred2.from_plan(a._plan, a.std_beta[1], a._n_per_snp, a.dequantize_scale, 0.3, **kw)
    a.fit()
    b.fit()
    assert np.array_equal(a.post_mean_beta[1], b.post_mean_beta[1], equal_nan=True) and a.post_mean_beta[1].any()
    assert list(a.grid_table.columns) == list(b.grid_table.columns) == ["p", "h2", "diverged", "n_nonzero", "kept"]
    for k in a.grid_table.columns:
        assert np.array_equal(a.grid_table[k].to_numpy(), b.grid_table[k].to_numpy(), equal_nan=k in ("p", "h2")), k
    assert np.array_equal(a.p_history, b.p_history, equal_nan=True) and b.p_history.shape == (8, 3)


@pytest.mark.parametrize("case", ["float64", "spike_slab", "mixture", "masked_grid", "wide_band", "keep_draws_first"])
def test_refusals_launch_nothing(gpu, case):
    """Each refusal is a ValueError (VIPRS_EINVAL) before any launch: the timing record does not move, the state's fields
    keep their bits."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, LDPlan
    if case == "wide_band":
        ld = _too_wide_a_band()
        std_beta = np.zeros(ld.m, dtype=np.float32)
    else:
        ld, std_beta, _ = _problem(False, np.float32, (130, 64, 1))
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)
    try:
        ok = DeviceState(plan, "float32", model="grid", width=2, placement="off")
        if case == "wide_band":
            assert plan.info(L.INFO_N_RAGGED) == 1
        ok.e_step(1.0)                                       # one timed sweep first: the record must not move afterwards
        ms = plan.last_kernel_ms(0)
        n = len(plan.timing_history())
        kind = {"float64": dict(float_precision="float64", model="grid", width=2), "spike_slab": {},
                "mixture": dict(model="mixture", width=3), "masked_grid": dict(model="grid", width=2),
                "wide_band": dict(model="grid", width=2), "keep_draws_first": dict(model="grid", width=2)}[case]
        st = DeviceState(plan, placement="off", **kind)
        if case == "masked_grid":
            st.set_groups([0, 130, ld.m])
            st.set_group_columns(np.array([[1, 0], [1, 1]], dtype=np.uint8))
        rng = np.random.default_rng(5)
        names = [k for k in ("std_beta", "u_logs", "half_var_tau", "mu_mult") + FIELDS]
        before = {}
        for k in names:
            a = rng.standard_normal(st._shape(k)).astype(st.dtype)
            before[k] = np.asfortranarray(a) if st.model == "grid" and a.ndim == 2 else a
            st.upload(k, before[k])
        with pytest.raises(ValueError, match="Gibbs"):
            st.gibbs_sweep(1.0, keep_draws=case == "keep_draws_first")
        assert plan.last_kernel_ms(0) == ms and len(plan.timing_history()) == n
        for k in names:
            u = f"u{st.dtype.itemsize}"
            assert np.array_equal(st.download(k).view(u), before[k].view(u)), k
        st.close()
        ok.close()
    finally:
        plan.close()
