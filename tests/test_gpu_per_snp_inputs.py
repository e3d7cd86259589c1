"""GPU: every kernel family of the E-step sweep (panel, batched matrix-core grid, band, generic, float64 tile) and the
elastic-net and Gibbs policies, fed per-SNP inputs that DIFFER from SNP to SNP (tests/per_snp_inputs.py), bit for bit against
the oracle or the committed replays, two sweeps each (the second reads a state that varies along the SNPs too).

Every other sweep test builds u_logs, sqrt_half_var_tau / half_var_tau, mu_mult, log_null_pi, the starting var_gamma, the
elastic net's mult / pen and the Gibbs chains' inputs from one sample size and one prior for all SNPs: a kernel that fetched
one of them at the wrong SNP (the panel-local row, a neighbouring lane's row, the previous panel's row after a hand-off,
j * K + k with the wrong j) stays `==` the oracle there.  tests/test_per_snp_inputs.py shows on the CPU that with these inputs
an exchange of two neighbouring SNPs' values changes the result in every block.  A failure names the first SNP that differs
(`per_snp_inputs.first_difference`): its block, 64-row panel and row say which role of the kernel read it."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import per_snp_inputs as P
from tests.test_band import _inputs as band_inputs, banded_ld, dense_beside_banded
from tests.test_gpu_models import _run_grid, _run_mix
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
PLAN = [2370, 1601, 130, 64, 1]            # tests/test_gpu_panel_roles.py: every role of the panel kernel
SWEEPS = 2
MODELS = ["spike_slab", "grid", "mix3", "mix4", "mix6", "mix12", "mix20"]
LD_FORMS = [(False, np.float32), (True, np.float32), (True, np.int8), (False, np.int16)]
LD_IDS = ["sym-f32", "upper-f32", "upper-i8", "sym-i16"]


@pytest.fixture
def S():
    """`e_step_hip` with an empty plan cache before and after: the cases set switches a plan reads when it is made."""
    from viprs_amd.vi import e_step_hip
    e_step_hip.clear_plan_cache()
    yield e_step_hip
    e_step_hip.clear_plan_cache()


@functools.lru_cache(maxsize=None)
def _problem(sizes, low_memory, ld_dtype, seed, T=np.float32):
    return syn.make_problem(sizes=list(sizes), low_memory=low_memory, ld_dtype=ld_dtype, seed=seed, kind="longrange",
                            float_precision=T)


def _untouched(got, st0, G, active):
    """The columns nobody lists keep their bits, in all five arrays."""
    rest = [c for c in range(G) if c not in set(int(a) for a in active)]
    assert rest
    for k in H.STATE:
        assert np.array_equal(got[k][:, rest], st0[k][:, rest]), k


# ---- the panel kernel, every role -----------------------------------------------------------------------------------------------
def _spike_slab_through_a_plan(ld, inp):
    """Through a plan of its own: the skip count of the last sweep is read from it."""
    from viprs_amd.plan import LDPlan
    st0 = inp.state_copy()
    ref = H.run_oracle(ld, inp, st0, sweeps=SWEEPS)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)
    try:
        got = {k: v.copy() for k, v in st0.items()}
        for _ in range(SWEEPS):
            plan.e_step(inp.std_beta, got["var_gamma"], got["var_mu"], got["eta"], got["q"], got["eta_diff"], inp.u_logs,
                        inp.sqrt_half_var_tau, inp.mu_mult, ld.dq_scale)
        skipped = plan.last_skipped()
    finally:
        plan.close()
    P.assert_equal(got, ref, ld, H.STATE)
    want = int((ref["eta_diff"] == 0).sum())
    assert 0 < want < ld.m and skipped == want


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("low_memory, ld_dtype", LD_FORMS, ids=LD_IDS)
def test_panel_kernel_every_role(gpu, S, low_memory, ld_dtype, model, monkeypatch):
    ld, ss, inp = _problem(tuple(PLAN), low_memory, ld_dtype, 53)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")      # teams of 8: the large class takes the narrow team strips
    monkeypatch.setenv("VIPRS_GRID_MFMA", "0")      # grid columns as panel items, not the batched matrix-core kernel
    S.clear_plan_cache()
    if model == "spike_slab":
        _spike_slab_through_a_plan(ld, P.spike_slab(inp.std_beta))
    elif model == "grid":
        g, st0 = P.grid(ld.m, 5)
        active = np.array([4, 0, 2], dtype=np.int32)
        got = _run_grid(S, ld, inp, g, st0, active, sweeps=SWEEPS)
        P.assert_equal(got, _run_grid(O, ld, inp, g, st0, active, sweeps=SWEEPS), ld, H.STATE)
        _untouched(got, st0, 5, active)
    else:
        mix, st0 = P.mixture(ld.m, int(model[3:]))
        P.assert_equal(_run_mix(S, ld, inp, mix, st0, SWEEPS), _run_mix(O, ld, inp, mix, st0, SWEEPS), ld, H.STATE)


# ---- the batched matrix-core grid kernel ----------------------------------------------------------------------------------------
# The blocks: 130 = two panels and two rows (one full 128-column tile and a partial one), 64 = exactly one panel, and a block
# of several tiles with a partial last panel.  With 40 models swept the oracle's time on a 1 300-SNP block (40 x 1300^2 x 2
# sweeps, 0.21 - 0.26 s) was 2.5 x the slowest case of tests/test_gpu_panel_roles.py: that case takes 780 = 6 tiles + 12 rows,
# the smallest kind of block that still has a tile in the second accumulator slot of an owner wave (tile 6: kGridResOwners = 6).
@pytest.mark.parametrize("G, active, sizes", [(32, [31, 0, 7, 8, 21], (130, 1300, 64)), (40, list(range(40)), (130, 780, 64))],
                         ids=["G32-5-active", "G40-two-chunks"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_batched_grid_kernel(gpu, S, low_memory, G, active, sizes, monkeypatch):
    monkeypatch.setenv("VIPRS_GRID_MFMA", "1")
    S.clear_plan_cache()
    ld, ss, inp = _problem(sizes, low_memory, np.float32, 33)
    g, st0 = P.grid(ld.m, G)
    active = np.array(active, dtype=np.int32)
    got = _run_grid(S, ld, inp, g, st0, active, sweeps=SWEEPS)
    P.assert_equal(got, _run_grid(O, ld, inp, g, st0, active, sweeps=SWEEPS), ld, H.STATE)
    if len(active) < G:
        _untouched(got, st0, G, active)


# ---- the band kernel and its generic twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["spike_slab", "grid", "mix4"])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("m, wl, wr, jitter", [(1500, 130, 70, 40), (64, 5, 9, 3)], ids=["ragged1500", "ragged64"])
def test_band_kernel_and_generic_kernel(gpu, S, m, wl, wr, jitter, low_memory, ld_dtype, model, monkeypatch):
    ld = banded_ld(m, wl, wr, low_memory, ld_dtype, seed=m, jitter=jitter)
    ss, inp0 = band_inputs(m)
    if model == "spike_slab":
        inp = P.spike_slab(ss.std_beta)
        st0 = inp.state_copy()
        ref = H.run_oracle(ld, inp, st0, sweeps=SWEEPS)
        run = lambda: H.run_hip(ld, inp, st0, sweeps=SWEEPS)
    elif model == "grid":
        g, st0 = P.grid(m, 5)
        active = np.array([4, 0, 2], dtype=np.int32)
        ref = _run_grid(O, ld, inp0, g, st0, active, sweeps=SWEEPS)
        run = lambda: _run_grid(S, ld, inp0, g, st0, active, sweeps=SWEEPS)
    else:
        mix, st0 = P.mixture(m, 4)
        ref = _run_mix(O, ld, inp0, mix, st0, SWEEPS)
        run = lambda: _run_mix(S, ld, inp0, mix, st0, SWEEPS)
    P.assert_equal(run(), ref, ld, H.STATE)                       # the band kernel
    monkeypatch.setenv("VIPRS_BAND", "0")
    S.clear_plan_cache()
    P.assert_equal(run(), ref, ld, H.STATE)                       # the row-by-row generic kernel


@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_wide_mixture_on_dense_and_windowed_blocks(gpu, S, low_memory):
    """K = 9: the wide panel chain on the dense block, the prologue launch in front of it and the generic kernel on the
    windowed component, in one sweep."""
    ld = dense_beside_banded([90], 300, 20, low_memory)
    ss, inp = band_inputs(ld.m, seed=16)
    mix, st0 = P.mixture(ld.m, 9)
    P.assert_equal(_run_mix(S, ld, inp, mix, st0, SWEEPS), _run_mix(O, ld, inp, mix, st0, SWEEPS), ld, H.STATE)


# ---- the generic kernel on dense blocks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_generic_kernel_on_dense_blocks(gpu, S, low_memory):
    """K = 33: more components than the panel kernels take."""
    ld, ss, inp = _problem((70, 333, 1), low_memory, np.float32, 31)
    mix, st0 = P.mixture(ld.m, 33)
    P.assert_equal(_run_mix(S, ld, inp, mix, st0, SWEEPS), _run_mix(O, ld, inp, mix, st0, SWEEPS), ld, H.STATE)


# ---- float64 state: the tile kernel and the row-by-row route --------------------------------------------------------------------
@pytest.mark.parametrize("model", ["spike_slab", "mix4", "grid8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_float64_tile_and_row_by_row(gpu, S, low_memory, model, monkeypatch):
    T = np.float64
    ld, ss, inp0 = _problem((1400, 333, 64, 1), low_memory, np.int8, 41, T)
    if model == "spike_slab":
        inp = P.spike_slab(inp0.std_beta, T)
        st0 = inp.state_copy()
        ref = H.run_oracle(ld, inp, st0, sweeps=SWEEPS)
        assert 0 < int((ref["eta_diff"] == 0).sum()) < ld.m        # both branches
        run = lambda: H.run_hip(ld, inp, st0, sweeps=SWEEPS)
    elif model == "mix4":
        mix, st0 = P.mixture(ld.m, 4, T)
        ref = _run_mix(O, ld, inp0, mix, st0, SWEEPS)
        run = lambda: _run_mix(S, ld, inp0, mix, st0, SWEEPS)
    else:
        g, st0 = P.grid(ld.m, 8, T)
        active = np.array([7, 0, 3, 4], dtype=np.int32)
        ref = _run_grid(O, ld, inp0, g, st0, active, sweeps=SWEEPS)
        run = lambda: _run_grid(S, ld, inp0, g, st0, active, sweeps=SWEEPS)
    monkeypatch.delenv("VIPRS_F64_ROW_BY_ROW", raising=False)
    S.clear_plan_cache()
    tile = run()
    assert tile["q"].dtype == T
    P.assert_equal(tile, ref, ld, H.STATE)
    monkeypatch.setenv("VIPRS_F64_ROW_BY_ROW", "1")
    S.clear_plan_cache()
    rows = run()
    P.assert_equal(rows, ref, ld, H.STATE)
    P.assert_equal(tile, rows, ld, H.STATE)
    if model == "grid8":
        _untouched(tile, st0, 8, active)
        _untouched(rows, st0, 8, active)


# ---- the elastic-net and the LDpred2 Gibbs policies -----------------------------------------------------------------------------
POLICY_LD = [(False, np.float32), (True, np.int8)]
POLICY_IDS = ["sym-f32", "upper-i8"]


def _column_1_keeps_its_bits(got, st0, fields):
    for k in fields:
        assert np.array_equal(got[k][:, 1].view(np.uint32), st0[k][:, 1].view(np.uint32)), k


@pytest.mark.parametrize("low_memory, ld_dtype", POLICY_LD, ids=POLICY_IDS)
def test_elastic_net_sweep(gpu, S, low_memory, ld_dtype, monkeypatch):
    from tests import test_gpu_enet as E
    ld, ss, inp = _problem(tuple(E.SIZES), low_memory, ld_dtype, 53)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")
    _, _, st0 = E._start(ld.m, E.GRID, junk_cols=(1,))
    mult, pen = P.enet(ld.m, E.GRID)
    want = E._replay(ld, inp.std_beta, mult, pen, st0, SWEEPS, E.ACTIVE)
    for g in E.ACTIVE:                                  # both sides of the threshold are taken
        assert 0 < np.count_nonzero(want["eta"][:, g]) < ld.m, g
    got = E._device(ld, inp.std_beta, mult, pen, st0, SWEEPS, np.array(E.ACTIVE, dtype=np.int32))
    P.assert_equal(got, want, ld, E.FIELDS)
    _column_1_keeps_its_bits(got, st0, E.FIELDS)


@pytest.mark.parametrize("low_memory, ld_dtype", POLICY_LD, ids=POLICY_IDS)
def test_gibbs_sweep(gpu, S, low_memory, ld_dtype, monkeypatch):
    from tests import test_gpu_gibbs as GT
    ld, ss, inp = _problem(tuple(GT.SIZES), low_memory, ld_dtype, 53)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")
    _, st0 = GT._start(ss.n_per_snp, GT.PAIRS, junk_cols=(1,))
    inputs = P.gibbs(ld.m, GT.PAIRS)
    got, draws = GT._device(ld, inp.std_beta, inputs, st0, SWEEPS, np.array(GT.ACTIVE, dtype=np.int32))
    GT._assert_draws_are_the_hosts(draws, inputs["half_var_tau"], GT.ACTIVE)      # (the noise is scaled by half_var_tau[j])
    want = GT._replay(ld, inp.std_beta, inputs, st0, draws, GT.ACTIVE)            # fed the device's own draws
    for g in GT.ACTIVE:
        assert 0 < np.count_nonzero(want["eta"][:, g]) < ld.m, g
    P.assert_equal(got, want, ld, GT.FIELDS)
    _column_1_keeps_its_bits(got, st0, GT.FIELDS)
    for unif, noise in draws:
        assert not unif[:, 1].any() and not noise[:, 1].any()
