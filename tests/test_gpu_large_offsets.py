"""GPU: every kernel family that reads LD, on plans whose LD offsets need more than 31 and more than 32 bits
(tests/large_offset_plans.py), bit for bit against the family's existing reference run on a small host-built LD that holds
only the group of blocks placed behind the mark.

The largest plan of every other test keeps element offsets below 2^31 and byte offsets below 2^32: one `(int)` or `unsigned`
in an LD address would leave all of them green and give wrong posteriors on the largest inputs only.  tests/
test_large_offset_plans.py shows on the CPU that on these plans a row read at its offset truncated to 32 or 31 bits holds other
entries, for every row of every group.  A failure here names the group, the block of the plan and the row.

Device memory (INFO_LD_BYTES_DEVICE, printed by test_plan_is_what_the_block_list_implies): i8-sym 9.5 GB, i8-upper 7.0 GB,
f32-upper 14.4 GB, i16-sym 9.7 GB; the widest state (float32 grid, 32 columns, 383 k SNPs: nine arrays) adds 0.45 GB and the
one-block plans of the filler test 0.6 GB -- every case stays below 16 GB.  One big plan is alive at a time: one test class
per plan, the class-scoped fixture `big` makes the plan of the class's `KEY` and closes it when the class is done (a fixture
parametrised over the plans would be ordered by parameter INDEX, which differs from case to case, and remake the plans many
times).  Nothing here skips: a plan that cannot be allocated fails its cases with the library's message."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import large_offset_plans as LO
from tests import ld_dot_reference as DR
from tests import ld_score_reference as SR
from tests import order_replay as OR
from tests import per_snp_inputs as P
from tests.test_gpu_models import _run_grid, _run_mix
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
SWEEPS = 2


@pytest.fixture(scope="class")
def big(request, gpu):
    """The device-generated plan of the test class: `KEY` = (layout name, VIPRS_GRID_MFMA -- read when a plan is made).  One
    plan per class, closed when the class is done: at most one big plan is alive."""
    from viprs_amd.plan import LDPlan
    name, mfma = request.cls.KEY
    mp = pytest.MonkeyPatch()
    mp.setenv("VIPRS_GRID_MFMA", mfma)
    try:
        plan = LDPlan.synthetic(LO.skeleton(name))
    finally:
        mp.undo()
    full = LO.skeleton(name)
    yield SimpleNamespace(name=name, plan=plan, lay=LO.layout(name), full=full, dq=full.dq_scale, mfma=mfma)
    plan.close()


def _slice_inputs(inp, s, e):
    """`EStepInputs` of the SNPs [s, e)."""
    per_snp = ("std_beta", "var_gamma", "var_mu", "eta", "q", "eta_diff", "u_logs", "sqrt_half_var_tau", "mu_mult")
    return syn.EStepInputs(**{k: getattr(inp, k)[s:e].copy() for k in per_snp}, pi=inp.pi, sigma_epsilon=inp.sigma_epsilon,
                           tau_beta=inp.tau_beta)


def _rows(a, s, e):
    return np.array(a[s:e], order="F" if (a.ndim == 2 and a.flags.f_contiguous and not a.flags.c_contiguous) else "C")


def _sweeps_on_plan(plan, model, width, inputs, st0, dq, active=None, sweeps=SWEEPS):
    """`sweeps` calls of `DeviceState.e_step` on a state of the plan holding `inputs` and the start `st0`: the five state
    arrays afterwards.  (No placement probe: it would sweep the whole plan dozens of times.)"""
    from viprs_amd.plan import DeviceState
    st = DeviceState(plan, st0["eta"].dtype.name, model=model, width=width, placement="off")
    try:
        for k, a in inputs.items():
            st.upload(k, a)
        for k in H.STATE:
            st.upload(k, st0[k])
        for _ in range(sweeps):
            st.e_step(dq, active_model_idx=active)
        return {k: st.download(k) for k in H.STATE}
    finally:
        st.close()


def _spike_slab_on_plan(plan, inp, dq):
    return _sweeps_on_plan(plan, "spike_slab", 1, {k: getattr(inp, k) for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult")},
                           inp.state_copy(), dq)


def _check_spike_slab(big, inp, got, what):
    LO.assert_all_finite(got, f"{what} {big.name}")
    for g, blocks in big.lay.groups.items():
        s, e = big.lay.snps(blocks)
        sub = LO.sub_ld(big.name, g)
        part = _slice_inputs(inp, s, e)
        ref = H.run_oracle(sub, part, part.state_copy(), sweeps=SWEEPS)
        assert 0 < int((ref["eta_diff"] == 0).sum()) < sub.m                 # both branches of the update
        LO.assert_group_equal(got, ref, big.lay, g, H.STATE, what)


# ---- the plans --------------------------------------------------------------------------------------------------------------------
def plan_is_what_the_block_list_implies(self, big):
    from viprs_amd import _lib as L
    plan, lay, full = big.plan, big.lay, big.full
    assert plan.info(L.INFO_NNZ) == int(full.ld_indptr[-1]) == full.nnz
    assert plan.info(L.INFO_N_DENSE) == lay.n_dense and plan.info(L.INFO_N_RAGGED) == lay.n_ragged == 1
    assert plan.info(L.INFO_M) == lay.m and plan.n_blocks == len(lay.sizes)
    assert np.array_equal(plan.blocks()[0], lay.block_start)
    lb, ip = plan.windows()
    assert np.array_equal(ip, full.ld_indptr) and np.array_equal(lb, full.ld_left_bound)
    # the raw buffer (kept: one block is ragged) and the repacked squares with their slack
    es = lay.ld_dtype.itemsize
    dense_elems = LO.dense_layout(lay.sizes)[2]
    want = full.nnz * es + 64 + (dense_elems + 4 * 256 + 64 * int(LO.dense_layout(lay.sizes)[1].max())) * es
    got = plan.info(L.INFO_LD_BYTES_DEVICE)
    print(f"{big.name}: {got / 1e9:.2f} GB of LD on the device, m = {lay.m}")
    assert abs(got - want) <= 4096 * es and got < 16e9


# ---- the LD product and the LD scores (ld_rows.h) -----------------------------------------------------------------------------------
def _check_product_and_scores(big, what):
    plan, lay = big.plan, big.lay
    rng = np.random.default_rng(71)
    B = np.asfortranarray(rng.standard_normal((lay.m, 3)).astype(np.float32))
    y = plan.dot(B, dq_scale=big.dq)
    scores = plan.ld_scores(B, None, dq_scale=big.dq)
    LO.assert_all_finite({"dot": y, "ld_scores": scores}, f"{what} {big.name}")
    for g, blocks in lay.groups.items():
        s, e = lay.snps(blocks)
        sub = LO.sub_ld(big.name, g)
        Bg = _rows(B, s, e)
        arrays = (sub.ld_left_bound, sub.ld_indptr, sub.ld_data, sub.low_memory)
        want = {"dot": DR.finish(OR.replay_dot(*arrays, Bg), Bg, big.dq, True, np.float32)}
        S2, S0 = OR.replay_scores(*arrays, Bg, np.float32)
        want["ld_scores"] = SR.finish(S2, S0, Bg, None, big.dq, np.float32)
        assert np.any(want["dot"] != Bg)
        LO.assert_group_equal({"dot": y, "ld_scores": scores}, want, lay, g, ("dot", "ld_scores"), what)
    return B, y, scores


def ld_product_and_ld_scores(self, big):
    _check_product_and_scores(big, "product as created")


# ---- clumping (ld_clump.h) ------------------------------------------------------------------------------------------------------
def clump(self, big):
    from tests.test_clump_reference import chisq_draw
    from tests.test_gpu_clump import R2_5
    from viprs_amd.stats.clump import clump_host, clump_order
    plan, lay = big.plan, big.lay
    chisq = chisq_draw(lay.m, 7)
    order, member = clump_order(chisq, 1.0), chisq >= 0.3
    got = plan.clump(order, R2_5, member=member, dq_scale=big.dq)
    assert got.shape == (lay.m, 5) and got.min() >= -1 and got.max() < lay.m
    # a clump never leaves its LD block
    blk = np.searchsorted(lay.block_start, np.arange(lay.m), side="right") - 1
    claimed = got >= 0
    assert np.array_equal(np.searchsorted(lay.block_start, got[claimed], side="right") - 1,
                          np.broadcast_to(blk[:, None], got.shape)[claimed])
    for g, blocks in lay.groups.items():
        s, e = lay.snps(blocks)
        sub = LO.sub_ld(big.name, g)
        og = order[(order >= s) & (order < e)] - s
        r = clump_host(sub.ld_left_bound, sub.ld_indptr, sub.ld_data, sub.low_memory, og, R2_5, member[s:e], big.dq)
        want = np.where(r >= 0, r + s, -1).astype(np.int32)
        assert ((r >= 0) & (r != np.arange(e - s)[:, None])).sum(axis=0)[0] > 0.05 * (e - s)      # SNPs are claimed
        LO.assert_group_equal({"index_of": got}, {"index_of": want}, lay, g, ("index_of",), "clump")


# ---- the panel sweep: spike-and-slab, mixture of 4, grid columns as panel items ---------------------------------------------------
_whole_plan_spike_slab = {}              # plan -> (inputs, result of the whole plan): shared with the filler test


def _spike_slab_whole_plan(big):
    key = (big.name, big.mfma)
    if key not in _whole_plan_spike_slab:
        inp = P.spike_slab(LO.sumstats(big.name).std_beta)
        _whole_plan_spike_slab[key] = (inp, _spike_slab_on_plan(big.plan, inp, big.dq))
    return _whole_plan_spike_slab[key]


@pytest.mark.parametrize("model", ["spike_slab", "mix4", "grid"])
def panel_sweep_three_models(self, big, model):
    _panel_sweep(big, model)


def panel_sweep_spike_slab(self, big):
    _panel_sweep(big, "spike_slab")


def _panel_sweep(big, model):
    plan, lay = big.plan, big.lay
    std_beta = LO.sumstats(big.name).std_beta
    if model == "spike_slab":
        inp, got = _spike_slab_whole_plan(big)
        _check_spike_slab(big, inp, got, "panel sweep")
        return
    if model == "mix4":
        mix, st0 = P.mixture(lay.m, 4)
        got = _sweeps_on_plan(plan, "mixture", 4, dict(std_beta=std_beta, log_null_pi=mix["log_null_pi"], u_logs=mix["u_logs"],
                                                       sqrt_half_var_tau=mix["shvt"], mu_mult=mix["mu_mult"]), st0, big.dq)
    else:
        g, st0 = P.grid(lay.m, 5)
        active = np.array([4, 0, 2], dtype=np.int32)
        got = _grid_on_plan(plan, std_beta, g, st0, active, big.dq)
    LO.assert_all_finite(got, f"{model} {big.name}")
    for grp, blocks in lay.groups.items():
        s, e = lay.snps(blocks)
        sub = LO.sub_ld(big.name, grp)
        part = SimpleNamespace(std_beta=std_beta[s:e].copy())
        st0g = {k: _rows(v, s, e) for k, v in st0.items()}
        if model == "mix4":
            ref = _run_mix(O, sub, part, {k: _rows(v, s, e) for k, v in mix.items()}, st0g, SWEEPS)
        else:
            ref = _run_grid(O, sub, part, {k: _rows(v, s, e) for k, v in g.items()}, st0g, active, sweeps=SWEEPS)
        LO.assert_group_equal(got, ref, lay, grp, H.STATE, model)


def _grid_on_plan(plan, std_beta, g, st0, active, dq):
    return _sweeps_on_plan(plan, "grid", st0["eta"].shape[1], dict(std_beta=std_beta, u_logs=g["u_logs"], half_var_tau=g["hvt"],
                                                                   mu_mult=g["mu_mult"]), st0, dq, active)


# ---- the batched matrix-core grid kernel ------------------------------------------------------------------------------------------
def batched_grid_kernel(self, big):
    plan, lay = big.plan, big.lay
    std_beta = LO.sumstats(big.name).std_beta
    g, st0 = P.grid(lay.m, 32)
    active = np.array([31, 0, 7, 8, 21], dtype=np.int32)
    got = _grid_on_plan(plan, std_beta, g, st0, active, big.dq)
    LO.assert_all_finite(got, f"batched grid {big.name}")
    rest = [c for c in range(32) if c not in set(int(a) for a in active)]
    for k in H.STATE:
        assert np.array_equal(got[k][:, rest], st0[k][:, rest]), k
    for grp, blocks in lay.groups.items():
        s, e = lay.snps(blocks)
        ref = _run_grid(O, LO.sub_ld(big.name, grp), SimpleNamespace(std_beta=std_beta[s:e].copy()),
                        {k: _rows(v, s, e) for k, v in g.items()}, {k: _rows(v, s, e) for k, v in st0.items()}, active,
                        sweeps=SWEEPS)
        LO.assert_group_equal(got, ref, lay, grp, H.STATE, "batched grid")


# ---- float64 state: the tile kernel and the row-by-row route; then fp32 again on the upper form --------------------------------------
@pytest.mark.parametrize("route", ["tile", "row_by_row"])
def float64_state(self, big, route, monkeypatch):
    from viprs_amd import _lib as L
    if route == "tile":
        monkeypatch.delenv("VIPRS_F64_ROW_BY_ROW", raising=False)
    else:
        monkeypatch.setenv("VIPRS_F64_ROW_BY_ROW", "1")
    inp = P.spike_slab(LO.sumstats(big.name).std_beta.astype(np.float64), np.float64)
    got = _spike_slab_on_plan(big.plan, inp, big.dq)
    assert got["q"].dtype == np.float64
    _check_spike_slab(big, inp, got, f"float64 {route}")
    if big.lay.low_memory:
        # the tile kernel sweeps the packed form: the lower triangles of the dense squares are zero now (the row-by-row
        # kernels read a row's own window and take the squares as they find them) ...
        assert route != "tile" or big.plan.info(L.INFO_UPPER_MIRRORED) == 0
        # ... the product gathers what lies left of the diagonal from the column above it, without converting the storage ...
        _check_product_and_scores(big, "product over the zero lower triangle" if route == "tile" else "product after float64")
        assert route != "tile" or big.plan.info(L.INFO_UPPER_MIRRORED) == 0
        # ... and an fp32 sweep mirrors every square of the buffer again (mirror_lower_kernel both ways over all of it)
        inp32 = P.spike_slab(LO.sumstats(big.name).std_beta)
        got32 = _spike_slab_on_plan(big.plan, inp32, big.dq)
        assert big.plan.info(L.INFO_UPPER_MIRRORED) == 1
        _check_spike_slab(big, inp32, got32, f"fp32 after float64 {route}")


# ---- the elastic-net and the Gibbs sweeps: three columns, the middle one unswept ---------------------------------------------------
def _dense_blocks_only(big):
    """These two sweeps have no row-by-row kernel: the block above kMaxDenseBlock is left out of them."""
    active = np.ones(len(big.lay.sizes), dtype=bool)
    active[big.lay.oversize] = False
    big.plan.set_active_blocks(active)


def elastic_net_sweep(self, big):
    from tests import test_gpu_enet as E
    from viprs_amd.plan import DeviceState
    plan, lay = big.plan, big.lay
    std_beta = LO.sumstats(big.name).std_beta
    _, _, st0 = E._start(lay.m, E.GRID, junk_cols=(1,))
    mult, pen = P.enet(lay.m, E.GRID)
    active = np.array(E.ACTIVE, dtype=np.int32)
    _dense_blocks_only(big)
    try:
        st = DeviceState(plan, "float32", model="grid", width=3, placement="off")
        st.upload("std_beta", std_beta)
        st.upload("mu_mult", mult)
        st.upload("half_var_tau", pen)
        st.upload("u_logs", np.full_like(mult, np.nan))          # not read
        for k in E.FIELDS:
            st.upload(k, st0[k])
        for _ in range(SWEEPS):
            st.enet_sweep(big.dq, active_model_idx=active)
        got = {k: st.download(k) for k in E.FIELDS}
        st.close()
    finally:
        plan.set_active_blocks(None)
    LO.assert_all_finite(got, f"elastic net {big.name}")
    for k in E.FIELDS:
        assert np.array_equal(got[k][:, 1].view(np.uint32), st0[k][:, 1].view(np.uint32)), k
    for grp, blocks in lay.groups.items():
        s, e = lay.snps(blocks)
        want = E._replay(LO.sub_ld(big.name, grp), std_beta[s:e].copy(), _rows(mult, s, e), _rows(pen, s, e),
                         {k: _rows(v, s, e) for k, v in st0.items()}, SWEEPS, E.ACTIVE)
        for c in E.ACTIVE:
            assert 0 < np.count_nonzero(want["eta"][:, c]) < e - s, c
        LO.assert_group_equal(got, want, lay, grp, E.FIELDS, "elastic net")


def gibbs_sweep(self, big):
    from tests import test_gpu_gibbs as GT
    from viprs_amd.plan import DeviceState
    plan, lay = big.plan, big.lay
    ss = LO.sumstats(big.name)
    _, st0 = GT._start(ss.n_per_snp, GT.PAIRS, junk_cols=(1,))
    inputs = P.gibbs(lay.m, GT.PAIRS)
    active = np.array(GT.ACTIVE, dtype=np.int32)
    _dense_blocks_only(big)
    try:
        st = DeviceState(plan, "float32", model="grid", width=3, placement="off")
        st.upload("std_beta", ss.std_beta)
        for k, a in inputs.items():
            st.upload(k, a)
        for k in GT.FIELDS:
            st.upload(k, st0[k])
        draws = []
        for i in range(SWEEPS):
            st.gibbs_sweep(big.dq, active_model_idx=active, seed=GT.SEED, draw_index=i)
            draws.append((st.gibbs_download("unif"), st.gibbs_download("noise")))
        got = {k: st.download(k) for k in GT.FIELDS}
        st.close()
    finally:
        plan.set_active_blocks(None)
    LO.assert_all_finite(got, f"Gibbs {big.name}")
    for k in GT.FIELDS:
        assert np.array_equal(got[k][:, 1].view(np.uint32), st0[k][:, 1].view(np.uint32)), k
    for grp, blocks in lay.groups.items():
        s, e = lay.snps(blocks)
        want = GT._replay(LO.sub_ld(big.name, grp), ss.std_beta[s:e].copy(), {k: _rows(v, s, e) for k, v in inputs.items()},
                          {k: _rows(v, s, e) for k, v in st0.items()}, [(_rows(u, s, e), _rows(z, s, e)) for u, z in draws],
                          GT.ACTIVE)
        for c in GT.ACTIVE:
            assert 0 < np.count_nonzero(want["eta"][:, c]) < e - s, c
        LO.assert_group_equal(got, want, lay, grp, GT.FIELDS, "Gibbs")


# ---- MINRES, Lanczos, SuSiE: the solvers on ld_rows.h ---------------------------------------------------------------------------
def _group_blocks(big):
    for grp, blocks in big.lay.groups.items():
        s, e = big.lay.snps(blocks)
        sub = LO.sub_ld(big.name, grp)
        yield grp, blocks, s, e, (sub.ld_left_bound, sub.ld_indptr, sub.ld_data, sub.low_memory)


def _same_per_block(what, big, grp, blocks, got, want, fields):
    for f in fields:
        a, b = np.asarray(getattr(got, f))[blocks], np.asarray(getattr(want, f))
        assert np.array_equal(a, b), (f"{what} {big.name} group {grp}: {f} of the group's blocks "
                                      f"{np.nonzero(np.atleast_1d((a != b).reshape(len(blocks), -1).any(axis=1)))[0].tolist()}: "
                                      f"device {a.tolist()} replay {b.tolist()}")


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def ridge_solve(self, big, T):
    from tests.test_gpu_ridge import REPLAY_MAXITER, RTOL
    b = LO.sumstats(big.name).std_beta.astype(T)
    for k in (3, REPLAY_MAXITER):
        x, info = big.plan.solve_ridge(b, 0.5, dq_scale=big.dq, rtol=RTOL[T], maxiter=k, check_every=1 if k == 3 else 4)
        assert np.isfinite(x).all()
        for grp, blocks, s, e, arrays in _group_blocks(big):
            xr, ir = OR.replayed_solve(*arrays, b[s:e].copy(), 0.5, big.dq, RTOL[T], maxiter=k)
            if k == REPLAY_MAXITER:
                assert np.all(ir.status == 0) and 8 < ir.iterations.max() < REPLAY_MAXITER
            _same_per_block(f"ridge maxiter={k}", big, grp, blocks, info, ir, ("iterations", "status", "relres"))
            LO.assert_group_equal({"x": x}, {"x": xr}, big.lay, grp, ("x",), f"ridge maxiter={k}")


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def extremal_eigenvalues(self, big, T):
    from tests.test_gpu_spectrum import FIELDS, REPLAY_MAXITER, REPLAY_RTOL
    for k in (5, REPLAY_MAXITER):
        got = big.plan.extremal_eigenvalues(dq_scale=big.dq, rtol=REPLAY_RTOL, maxiter=k, float_precision=T)
        assert all(np.isfinite(getattr(got, f)).all() for f in FIELDS)
        for grp, blocks, s, e, arrays in _group_blocks(big):
            want = OR.replayed_spectrum(*arrays, big.dq, REPLAY_RTOL, k, T)
            if k == REPLAY_MAXITER:
                assert np.all(want.status == 0) and 16 < want.iterations.max() < REPLAY_MAXITER
            _same_per_block(f"Lanczos maxiter={k}", big, grp, blocks, got, want, FIELDS)


@pytest.mark.parametrize("T", ["float32", "float64"])
def susie(self, big, T):
    from tests import susie_replay as SU
    from tests.test_gpu_susie import _z_scores
    z = _z_scores(big.lay.m)
    got = big.plan.susie(z, 3, 50.0, True, dq_scale=big.dq, tol=1e-4, max_iter=6, check_every=2, float_precision=T)
    assert np.isfinite(got.alpha).all() and np.isfinite(got.mu).all()
    for grp, blocks, s, e, arrays in _group_blocks(big):
        want = SU.susie_replay(*arrays, z[s:e].copy(), 3, 50.0, True, None, big.dq, 1e-4, 6, T)
        _same_per_block("SuSiE", big, grp, blocks, got, want, ("prior_variance", "post_var", "iterations", "delta", "status"))
        LO.assert_group_equal({"alpha": got.alpha, "mu": got.mu}, {"alpha": want.alpha, "mu": want.mu}, big.lay, grp,
                              ("alpha", "mu"), "SuSiE")


# ---- the fillers: device against device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["far_filler", "oversize"])
def filler_equals_the_block_alone(self, big, which):
    """The dense-route filler behind 2^32 and the block above kMaxDenseBlock (read from the raw buffer by the row-by-row
    kernels): their sweep and their product `==` the same block in a device-generated plan of its own.  No oracle on 10^8
    entries; tests/test_synth_device.py links a generated plan to an uploaded one."""
    from viprs_amd.plan import LDPlan
    lay, full = big.lay, big.full
    b = int(getattr(lay, which))
    s, e = lay.snps([b])
    inp, got = _spike_slab_whole_plan(big)
    rng = np.random.default_rng(71)
    B = np.asfortranarray(rng.standard_normal((lay.m, 3)).astype(np.float32))
    y = big.plan.dot(B, dq_scale=big.dq)
    one = syn.make_ld([int(lay.sizes[b])], low_memory=lay.low_memory, ld_dtype=lay.ld_dtype, rho=full.rho[[b]],
                      params=[full.params[b]], kind="longrange", data=False)
    alone = LDPlan.synthetic(one)
    try:
        want = _spike_slab_on_plan(alone, _slice_inputs(inp, s, e), big.dq)
        y1 = alone.dot(_rows(B, s, e), dq_scale=big.dq)
    finally:
        alone.close()
    assert np.count_nonzero(want["eta_diff"]) > 0.3 * (e - s)
    sub = syn.SyntheticLD(None, None, None, np.array([0, e - s]), None, lay.low_memory)
    for name, g, w in (("sweep", {k: got[k][s:e] for k in H.STATE}, want), ("product", {"dot": y[s:e]}, {"dot": y1})):
        msg = P.first_difference(g, w, sub)
        assert msg is None, f"{name} {big.name} {which} (block {b}, SNPs from {s}): {msg}"


# ---- one uploaded plan: a windowed component behind 2^31 raw entries ----------------------------------------------------------------
@pytest.fixture(scope="class")
def windowed(gpu):
    """The uploaded plan of `large_offset_plans.windowed_plan` (2.15 GB of int8, uploaded once for the class)."""
    from viprs_amd.plan import LDPlan
    lb, ip, start, sub = LO.windowed_plan()
    data = LO.windowed_plan_data()
    plan = LDPlan(lb, ip, data, True)
    del data
    yield SimpleNamespace(plan=plan, start=start, sub=sub, m=int(lb.shape[0]), dq=sub.dq_scale)
    plan.close()


def _assert_windowed_equal(got, ref, w, fields, what):
    msg = P.first_difference({k: got[k][w.start:] for k in fields}, ref, w.sub, fields)
    assert msg is None, f"{what}, the part behind the filler (SNPs from {w.start}): {msg}"


class TestUploadedWindowedPlan:
    """The band kernel, the ragged side of estep_tile.h, ld_rows.h and ld_clump.h on raw offsets beyond 2^31."""

    def test_plan(self, windowed):
        from viprs_amd import _lib as L
        plan = windowed.plan
        assert plan.info(L.INFO_NNZ) > 2 ** 31 and plan.n_blocks == 3
        assert plan.info(L.INFO_N_RAGGED) == 2 and plan.info(L.INFO_N_DENSE) == 1
        print(f"uploaded plan: {plan.info(L.INFO_LD_BYTES_DEVICE) / 1e9:.2f} GB of LD on the device")

    @pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
    def test_sweep_with_and_without_the_band_kernel(self, windowed, T, monkeypatch):
        """float32: the band kernel, then (VIPRS_BAND=0) its generic twin; float64: the tile kernel's windowed rows.  The
        sweeps visit the two blocks behind the filler (`set_active_blocks`): a chain over 143 000 rows of zeros would only
        cost time."""
        w = windowed
        rng = np.random.default_rng(LO.SEED + 3)
        beta = rng.standard_normal(w.m) * 0.004
        beta[rng.integers(0, w.m, w.m // 50)] += 0.05
        beta[w.start + rng.integers(0, w.sub.m, w.sub.m // 50)] += 0.05
        inp = P.spike_slab(beta.astype(T), T)
        part = _slice_inputs(inp, w.start, w.m)
        ref = H.run_oracle(w.sub, part, part.state_copy(), sweeps=SWEEPS)
        assert 0 < int((ref["eta_diff"] == 0).sum()) < w.sub.m
        w.plan.set_active_blocks([False, True, True])
        try:
            for band in ("1", "0"):
                monkeypatch.setenv("VIPRS_BAND", band)
                got = _spike_slab_on_plan(w.plan, inp, w.dq)
                LO.assert_all_finite(got, f"uploaded plan VIPRS_BAND={band}")
                _assert_windowed_equal(got, ref, w, H.STATE, f"sweep {np.dtype(T).name} VIPRS_BAND={band}")
                for k in H.STATE:                             # the filler's SNPs are not visited
                    assert np.array_equal(got[k][:w.start], inp.state_copy()[k][:w.start]), k
        finally:
            w.plan.set_active_blocks(None)

    def test_ld_product_and_ld_scores(self, windowed):
        w = windowed
        B = np.asfortranarray(np.random.default_rng(71).standard_normal((w.m, 3)).astype(np.float32))
        y = w.plan.dot(B, dq_scale=w.dq)
        scores = w.plan.ld_scores(B, None, dq_scale=w.dq)
        LO.assert_all_finite({"dot": y, "ld_scores": scores}, "uploaded plan")
        assert np.array_equal(y[:w.start], B[:w.start])                       # R = I on the filler
        Bg = _rows(B, w.start, w.m)
        arrays = (w.sub.ld_left_bound, w.sub.ld_indptr, w.sub.ld_data, True)
        S2, S0 = OR.replay_scores(*arrays, Bg, np.float32)
        want = {"dot": DR.finish(OR.replay_dot(*arrays, Bg), Bg, w.dq, True, np.float32),
                "ld_scores": SR.finish(S2, S0, Bg, None, w.dq, np.float32)}
        _assert_windowed_equal({"dot": y, "ld_scores": scores}, want, w, ("dot", "ld_scores"), "product")

    def test_clump(self, windowed):
        from tests.test_clump_reference import chisq_draw
        from tests.test_gpu_clump import R2_5
        from viprs_amd.stats.clump import clump_host, clump_order
        w = windowed
        chisq = chisq_draw(w.sub.m, 7)
        order, member = clump_order(chisq, 1.0), chisq >= 0.3
        r = clump_host(w.sub.ld_left_bound, w.sub.ld_indptr, w.sub.ld_data, True, order, R2_5, member, w.dq)
        assert ((r >= 0) & (r != np.arange(w.sub.m)[:, None])).sum(axis=0)[0] > 0.05 * w.sub.m
        whole = np.concatenate([np.zeros(w.start, dtype=bool), member])
        got = w.plan.clump(order + w.start, R2_5, member=whole, dq_scale=w.dq)
        assert np.all(got[:w.start] == -1)
        want = np.where(r >= 0, r + w.start, -1).astype(np.int32)
        _assert_windowed_equal({"index_of": got}, {"index_of": want}, w, ("index_of",), "clump")


# ---- one class per plan -----------------------------------------------------------------------------------------------------------
class _Int8SweepPlan:
    test_plan_is_what_the_block_list_implies = plan_is_what_the_block_list_implies
    test_ld_product_and_ld_scores = ld_product_and_ld_scores
    test_clump = clump
    test_panel_sweep = panel_sweep_three_models
    test_float64_state = float64_state
    test_elastic_net_sweep = elastic_net_sweep
    test_gibbs_sweep = gibbs_sweep
    test_filler_equals_the_block_alone = filler_equals_the_block_alone


class TestInt8Symmetric(_Int8SweepPlan):
    KEY = ("i8-sym", "0")


class TestInt8SymmetricBatchedGrid:
    KEY = ("i8-sym", "1")
    test_batched_grid_kernel = batched_grid_kernel


class TestInt8Upper(_Int8SweepPlan):
    KEY = ("i8-upper", "0")


class TestInt8UpperBatchedGrid:
    KEY = ("i8-upper", "1")
    test_batched_grid_kernel = batched_grid_kernel


class TestInt8UpperSolvers:
    KEY = ("i8-upper-solvers", "0")
    test_plan_is_what_the_block_list_implies = plan_is_what_the_block_list_implies
    test_ridge_solve = ridge_solve
    test_extremal_eigenvalues = extremal_eigenvalues
    test_susie = susie


class _ByteOffsetPlan:
    test_plan_is_what_the_block_list_implies = plan_is_what_the_block_list_implies
    test_ld_product_and_ld_scores = ld_product_and_ld_scores
    test_panel_sweep = panel_sweep_spike_slab


class TestFloat32Upper(_ByteOffsetPlan):
    KEY = ("f32-upper", "0")


class TestInt16Symmetric(_ByteOffsetPlan):
    KEY = ("i16-sym", "0")
