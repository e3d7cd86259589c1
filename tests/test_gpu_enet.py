"""GPU: the elastic-net sweep (viprs_state_enet_sweep: panel_enet.h in the panel sweep and the band kernel) against the host
replay of its definition (tests/enet_replay.c), `==` on eta, q, eta_diff, var_mu and var_gamma; the sums against
`enet_sums_host`; `Lassosum.fit()` against the same fit driven by `enet_sweep_host`; the refusals."""
import functools

import numpy as np
import pytest

from tests import enet_replay as ER
from tests.test_band import _inputs as band_inputs, banded_ld, dense_beside_banded
from viprs_amd.stats import enet as EN
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
SIZES = [2370, 1601, 130, 64, 1]         # tests/test_gpu_panel_roles.py: large team, medium team, partial panel, one panel, one row
FIELDS = ("eta", "q", "eta_diff", "var_mu", "var_gamma")
GRID = ((0.2, 0.005), (0.5, 0.002), (0.9, 0.005))
ACTIVE = [2, 0]


@functools.lru_cache(maxsize=None)
def _problem(low_memory, ld_dtype, sizes=tuple(SIZES)):
    ld, ss, inp = syn.make_problem(sizes=list(sizes), low_memory=low_memory, ld_dtype=ld_dtype, seed=53, kind="longrange")
    return ld, inp.std_beta


def _start(m, pairs, junk_cols=()):
    """mult, penalty and a state: eta = q = 0 (junk in `junk_cols`: columns nobody sweeps), junk in the three outputs."""
    rng = np.random.default_rng(17)
    G = len(pairs)
    shape = (m,) if G == 1 else (m, G)
    col = lambda v: np.asfortranarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (m, G)).reshape(shape))
    mult = col([np.float32(1.0 - s) for s, _ in pairs])
    pen = col([np.float32(lam) for _, lam in pairs])
    st = {k: np.asfortranarray(rng.standard_normal((m, G)).astype(np.float32).reshape(shape)) for k in FIELDS}
    for k in ("eta", "q"):
        keep = st[k].copy()
        st[k][...] = 0
        for g in junk_cols:
            st[k][:, g] = 0.01 * keep[:, g]
    return mult, pen, st


def _device(ld, std_beta, mult, pen, st0, sweeps, active=None, each=None, math_mode="exact"):
    from viprs_amd.plan import DeviceState, LDPlan
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, math_mode=math_mode)
    try:
        grid = mult.ndim == 2
        st = DeviceState(plan, "float32", model="grid" if grid else "spike_slab", width=mult.shape[1] if grid else 1,
                         placement="off")
        st.upload("std_beta", std_beta)
        st.upload("mu_mult", mult)
        st.upload("half_var_tau" if grid else "sqrt_half_var_tau", pen)
        st.upload("u_logs", np.full_like(mult, np.nan))          # not read
        for k in FIELDS:
            st.upload(k, st0[k])
        for i in range(sweeps):
            st.enet_sweep(ld.dq_scale, active_model_idx=active)
            if each is not None and each(i, st):
                break
        assert plan.effective_math_mode() == "exact"             # the one kernel, whatever the plan's math_mode
        out = {k: st.download(k) for k in FIELDS}
        st.close()
        return out
    finally:
        plan.close()


def _replay(ld, std_beta, mult, pen, st0, sweeps, active=None):
    st = {k: v.copy(order="F") for k, v in st0.items()}
    cols = [None] if mult.ndim == 1 else list(active if active is not None else range(mult.shape[1]))
    for g in cols:
        pick = (lambda a: a) if g is None else (lambda a: a[:, g])
        eta, q = pick(st["eta"]).copy(), pick(st["q"]).copy()
        for _ in range(sweeps):
            ed, mu, gam = ER.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, std_beta, pick(mult),
                                          pick(pen), eta, q, ld.dq_scale)
        for k, v in zip(FIELDS, (eta, q, ed, mu, gam)):
            pick(st[k])[...] = v
    return st


def _assert_equal(got, want):
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("width", [1, 3], ids=["width1", "grid3"])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8, np.int16], ids=["f32", "i8", "i16"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_every_role_of_the_sweep(gpu, low_memory, ld_dtype, width, monkeypatch):
    ld, std_beta = _problem(low_memory, ld_dtype)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")      # teams of 8: the large class takes the narrow team strips
    pairs, active, swept = (((0.5, 0.002),), None, [0]) if width == 1 else (GRID, ACTIVE, ACTIVE)
    mult, pen, st0 = _start(ld.m, pairs, junk_cols=() if width == 1 else (1,))
    want = _replay(ld, std_beta, mult, pen, st0, 3, active)
    # the chain is exercised: every swept column ends neither empty nor full
    for g in swept:
        frac = np.count_nonzero(want["eta"].reshape(ld.m, -1)[:, g]) / ld.m
        assert 0.10 <= frac <= 0.90, (g, frac)
    got = _device(ld, std_beta, mult, pen, st0, 3, None if active is None else np.array(active, dtype=np.int32))
    _assert_equal(got, want)
    if width > 1:
        for k in FIELDS:                             # column 1 keeps its uploaded bits
            assert np.array_equal(got[k][:, 1].view(np.uint32), st0[k][:, 1].view(np.uint32)), k


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("m, wl, wr, jitter, seed", [(900, 40, 40, 0, 8), (2500, 90, 140, 60, 5)], ids=["band", "ragged"])
def test_windowed_ld(gpu, m, wl, wr, jitter, seed, low_memory, ld_dtype):
    ld = banded_ld(m, wl, wr, low_memory, ld_dtype, seed=seed, jitter=jitter)
    ss, _ = band_inputs(m, seed=4)
    mult, pen, st0 = _start(m, ((0.5, 0.002),))
    want = _replay(ld, ss.std_beta, mult, pen, st0, 2)
    assert 0 < np.count_nonzero(want["eta"]) < m
    _assert_equal(_device(ld, ss.std_beta, mult, pen, st0, 2), want)


@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_dense_blocks_beside_a_band(gpu, low_memory):
    """One plan with a dense block (panel sweep) and a windowed component (band kernel), a grid state: the prologue launch
    with granules per model in front of both.  The plan is in math_mode = fast: the sweep is the same kernel and says so."""
    ld = dense_beside_banded([90], 300, 20, low_memory)
    ss, _ = band_inputs(ld.m, seed=16)
    mult, pen, st0 = _start(ld.m, GRID, junk_cols=(1,))
    active = np.array(ACTIVE, dtype=np.int32)
    want = _replay(ld, ss.std_beta, mult, pen, st0, 2, ACTIVE)
    assert 0 < np.count_nonzero(want["eta"][:, 0]) < ld.m
    _assert_equal(_device(ld, ss.std_beta, mult, pen, st0, 2, active, math_mode="fast"), want)


def test_fixed_point_on_the_device(gpu):
    """Swept until a sweep changes nothing: as many sweeps as the replay needs, the sums `==` the host's at every sweep."""
    ld, std_beta = _problem(False, np.float32, (1601, 130, 64, 1))
    s, lam = 0.9, 0.005
    mult, pen, st0 = _start(ld.m, ((s, lam),))
    eta, q = st0["eta"].copy(), st0["q"].copy()
    want_sums = []
    for k in range(1, 401):
        ed, _, _ = ER.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False, std_beta, mult, pen, eta, q, ld.dq_scale)
        want_sums.append(EN.enet_sums_host(std_beta, pen, eta, q, ed)[0])
        if want_sums[-1][0] == 0:
            break
    assert want_sums[-1][0] == 0 and 2 < len(want_sums) < 400
    got_sums = []

    def each(i, st):
        got_sums.append(st.enet_sums()[0])
        return got_sums[-1][0] == 0 or i + 1 >= len(want_sums) + 5

    got = _device(ld, std_beta, mult, pen, st0, 400, each=each)
    assert len(got_sums) == len(want_sums)
    assert np.array_equal(np.array(got_sums), np.array(want_sums))
    assert np.array_equal(got["eta"], eta) and np.array_equal(got["q"], q)
    R = ER.dense_matrix(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    assert ER.kkt_violation(R, std_beta, got["eta"], 1.0 - float(mult[0]), float(pen[0])) < ER.KKT_BOUND[(s, lam)]


def test_grid_sums_equal_the_host(gpu):
    """The rows of a grid state (256 workgroups at most) and a column list, on a plan long enough for several workgroups."""
    ld, std_beta = _problem(True, np.int8)
    mult, pen, st0 = _start(ld.m, GRID, junk_cols=(1,))
    from viprs_amd.plan import DeviceState, LDPlan
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    try:
        st = DeviceState(plan, "float32", model="grid", width=3, placement="off")
        st.upload("std_beta", std_beta)
        st.upload("half_var_tau", pen)
        for k in FIELDS:
            st.upload(k, st0[k])
        want = EN.enet_sums_host(std_beta, pen, st0["eta"], st0["q"], st0["eta_diff"])
        assert np.array_equal(st.enet_sums(), want)
        assert np.array_equal(st.enet_sums([2, 0]), want[[2, 0]])
        st.close()
    finally:
        plan.close()


@pytest.mark.parametrize("model", ["spike_slab", "grid"])
def test_sums_of_a_row_longer_than_256_workgroups(gpu, model):
    """70 001 SNPs: 274 workgroups for the row of a spike-and-slab state, the cap of 256 (two passes per thread, five
    partials per lane of the final pass) for the rows of a grid state."""
    from viprs_amd.plan import DeviceState, LDPlan
    m = 70001
    rng = np.random.default_rng(23)
    shape = (m,) if model == "spike_slab" else (m, 2)
    v = {k: np.asfortranarray(rng.standard_normal(shape).astype(np.float32)) for k in ("eta", "q", "eta_diff", "pen")}
    v["eta"][rng.random(shape) < 0.3] = 0
    v["pen"] = np.abs(v["pen"])
    std_beta = rng.standard_normal(m).astype(np.float32)
    plan = LDPlan(np.arange(m, dtype=np.int32), np.arange(m + 1, dtype=np.int64), np.ones(m, dtype=np.float32), False)
    try:
        st = DeviceState(plan, "float32", model=model, width=1 if model == "spike_slab" else 2, placement="off")
        st.upload("std_beta", std_beta)
        st.upload("sqrt_half_var_tau" if model == "spike_slab" else "half_var_tau", v["pen"])
        for k in ("eta", "q", "eta_diff"):
            st.upload(k, v[k])
        want = EN.enet_sums_host(std_beta, v["pen"], v["eta"], v["q"], v["eta_diff"], grid=model == "grid")
        other = EN.enet_sums_host(std_beta, v["pen"], v["eta"], v["q"], v["eta_diff"], grid=model != "grid")
        assert np.array_equal(st.enet_sums(), want) and not np.array_equal(want, other)
        st.close()
    finally:
        plan.close()


def test_lassosum_fit_equals_the_host_fit(gpu):
    got = ER.model_fit(device=True)
    want = ER.model_fit(device=False)
    for c in want.post_mean_beta:
        assert np.array_equal(got.post_mean_beta[c], want.post_mean_beta[c]), c
    assert got.grid_table.equals(want.grid_table)
    rng = np.random.default_rng(11)
    vb = {c: np.asarray(b, dtype=np.float64) + 0.002 * rng.normal(size=b.shape[0]) for c, b in got.std_beta.items()}
    got.select_best(validation_gdl=vb, criterion="pseudo_validation")
    r = np.asarray(got.validation_result["Pseudo_Validation_R2"])
    assert r.shape == (6,) and got.best_model_idx == int(np.argmax(r)) and r.max() > 0
    assert {c: b.shape for c, b in got.post_mean_beta.items()} == {c: (n,) for c, n in got.shapes.items()}


def test_from_plan_equals_the_loader_fit(gpu):
    """`Lassosum.from_plan` on the plan a loader-built model made (one chromosome of [130, 64] SNPs, int8 LD): the same fit."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import Lassosum
    kw = dict(s=ER.MODEL_S, lambdas=ER.MODEL_LAMBDAS, tol=ER.MODEL_TOL)
    gdl = ArrayDataLoader.synthetic({1: [130, 64]}, ld_dtype=np.int8, n=5e4, kind="longrange", h2=0.5)
    a = Lassosum(gdl, dequantize_on_the_fly=True, **kw)
    b = Lassosum.from_plan(a._plan, a.std_beta[1], a.dequantize_scale, **kw)
    a.fit()
    b.fit()
    assert np.array_equal(a.post_mean_beta[1], b.post_mean_beta[1], equal_nan=True)
    assert a.post_mean_beta[1].shape == (194, 6) and a.post_mean_beta[1].any()
    assert list(a.grid_table.columns) == list(b.grid_table.columns)
    for k in a.grid_table.columns:
        assert np.array_equal(a.grid_table[k].to_numpy(), b.grid_table[k].to_numpy(), equal_nan=k == "objective"), k


def _too_wide_a_band():
    """One windowed component whose first row reaches 16 400 SNPs: 257 panels to the right, more than the q ring holds."""
    m, reach = 16500, 16400
    j = np.arange(m)
    lo = np.maximum(j - 1, 0)
    hi = np.minimum(j + 2, m)
    hi[0] = reach
    length = hi - lo
    ip = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    data = np.full(int(ip[-1]), 0.01, dtype=np.float32)
    data[ip[:-1] + (j - lo)] = 1.0
    return syn.SyntheticLD(lo.astype(np.int32), ip, data, np.array([0, m]), np.zeros(1), False, 1.0)


@pytest.mark.parametrize("case", ["float64", "mixture", "masked_grid", "wide_band"])
def test_refusals_launch_nothing(gpu, case):
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, LDPlan
    if case == "wide_band":
        ld = _too_wide_a_band()
        std_beta = np.zeros(ld.m, dtype=np.float32)
    else:
        ld, std_beta = _problem(False, np.float32, (130, 64, 1))
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)
    try:
        # one timed sweep first: the record must not move afterwards
        ok = DeviceState(plan, "float32", placement="off")
        if case == "wide_band":
            assert plan.info(L.INFO_N_RAGGED) == 1
            ok.e_step(1.0)                                   # (the E-step has a row-by-row kernel for it)
        else:
            ok.enet_sweep(1.0)
        ms = plan.last_kernel_ms(0)
        n = len(plan.timing_history())
        kind, exc = {"float64": (dict(float_precision="float64"), NotImplementedError),
                     "mixture": (dict(model="mixture", width=3), ValueError),
                     "masked_grid": (dict(model="grid", width=2), NotImplementedError),
                     "wide_band": ({}, NotImplementedError)}[case]
        st = DeviceState(plan, placement="off", **kind)
        if case == "masked_grid":
            st.set_groups([0, 130, ld.m])
            st.set_group_columns(np.array([[1, 0], [1, 1]], dtype=np.uint8))
        before = st.download("eta")
        with pytest.raises(exc, match="elastic-net"):
            st.enet_sweep(1.0)
        assert plan.last_kernel_ms(0) == ms and len(plan.timing_history()) == n
        assert np.array_equal(st.download("eta"), before, equal_nan=True)
        st.close()
        ok.close()
    finally:
        plan.close()
