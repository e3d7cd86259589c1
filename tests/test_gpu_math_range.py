"""GPU: the device's exp, sigmoid and softmax over the whole argument range, inside every kernel family that inlines them.

tests/math_range_inputs.py makes the argument an input (sqrt_half_var_tau = 0 / half_var_tau = 0: the sigmoid argument is
u_logs[j], the softmax arguments are u_logs[j, k] - max) and keeps small results visible (mu_mult = 2^e); the LD stays the
real LD, so the serial chain's own gamma -- the wave-uniform table lookup -- is seen through d and q, beside the per-lane
lookup whose gamma is stored.  Every case compares all five state arrays `==` with the oracle (the Gibbs and the SuSiE cases
with their replays, and say so) over two sweeps per pass, and the stored var_gamma with a long-double sigmoid / softmax inside
the bounds tests/test_math_range_inputs.py shows the reference to meet: 2 units of max(eps ref, smallest denormal) for the
sigmoid, K + 4 for a softmax component.  A failure names the first SNP that differs (block, panel, row); its argument
names the k, the table entry and the branch.  `math_mode="fast"` is compared with the exact mode inside the README's 1e-5."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import math_range_inputs as M
from tests.test_band import _inputs as band_inputs, banded_ld
from tests.test_gpu_models import _run_grid, _run_mix
from viprs_amd.utils import synthetic as syn

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not M.have_long_double(), reason="no extended-precision long double on this host")]
PLAN = [2370, 1601, 130, 64, 1]            # tests/test_gpu_panel_roles.py: every role of the panel kernel
SWEEPS = 2
F32, F64 = np.float32, np.float64
MODELS = ["spike_slab", "grid", "mix3", "mix4", "mix6", "mix12", "mix20"]
LD_FORMS = [(False, np.float32), (True, np.float32), (True, np.int8), (False, np.int16)]
LD_IDS = ["sym-f32", "upper-f32", "upper-i8", "sym-i16"]
GRID_ACTIVE = np.array([4, 0, 2], dtype=np.int32)          # 3 of 5 columns


@pytest.fixture
def S():
    """`e_step_hip` with an empty plan cache before and after: the cases set switches a plan reads when it is made."""
    from viprs_amd.vi import e_step_hip
    e_step_hip.clear_plan_cache()
    yield e_step_hip
    e_step_hip.set_default_math_mode("exact")
    e_step_hip.clear_plan_cache()


@functools.lru_cache(maxsize=None)
def _problem(sizes, low_memory, ld_dtype, seed, T=F32):
    return syn.make_problem(sizes=list(sizes), low_memory=low_memory, ld_dtype=ld_dtype, seed=seed, kind="longrange",
                            float_precision=T)


def _within(got, ref, bound, T, what):
    d = M.distance(got, ref, T)
    assert float(d.max()) <= bound, (what, float(d.max()), int(np.argmax(d)))


def _untouched(got, st0, G, active):
    rest = [c for c in range(G) if c not in set(int(a) for a in active)]
    for k in H.STATE:
        assert np.array_equal(got[k][:, rest], st0[k][:, rest]), k


# ---- the three models, one pass each --------------------------------------------------------------------------------------------
def _spike_slab_pass(ld, inp, sweep, ref_arg):
    """Two sweeps, compared after each; returns (device state, oracle state, SNPs applied in either sweep)."""
    got, ref = inp.state_copy(), inp.state_copy()
    seen = np.zeros(ld.m, dtype=bool)
    for _ in range(SWEEPS):
        ref = H.run_oracle(ld, inp, ref, sweeps=1)
        got = sweep(inp, got)
        M.assert_equal(got, ref, ld, H.STATE)
        seen |= ref["eta_diff"] != 0
    _within(got["var_gamma"][seen], ref_arg[seen], 2, inp.std_beta.dtype, "sigmoid")
    return got, ref, seen


def _spike_slab(ld, beta, A, passes, sweep=None, deal=None):
    sweep = sweep or (lambda inp, st: H.run_hip(ld, inp, st, sweeps=1))
    for p in range(passes):
        a = (deal or (lambda p: M.deal(A, ld.m, p)))(p)
        _spike_slab_pass(ld, M.spike_slab(beta, a), sweep, M.sigmoid_ref(a))


def _spike_slab_through_a_plan(ld, beta, A, passes):
    """Through a plan of its own: the skip count of the last sweep is read from it."""
    from viprs_amd.plan import LDPlan
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)

    def sweep(inp, st):
        plan.e_step(inp.std_beta, st["var_gamma"], st["var_mu"], st["eta"], st["q"], st["eta_diff"], inp.u_logs,
                    inp.sqrt_half_var_tau, inp.mu_mult, ld.dq_scale)
        return st
    try:
        for p in range(passes):
            a = M.deal(A, ld.m, p)
            got, ref, _ = _spike_slab_pass(ld, M.spike_slab(beta, a), sweep, M.sigmoid_ref(a))
            want = int((ref["eta_diff"] == 0).sum())
            assert 0 < want < ld.m and plan.last_skipped() == want
    finally:
        plan.close()


def _grid(S, ld, inp0, A, G, active, passes, args=None):
    T = inp0.std_beta.dtype
    for p in range(passes):
        a = M.grid_args(A, ld.m, G, p) if args is None else args(p)
        g, st0 = M.grid(a)
        got = _run_grid(S, ld, inp0, g, st0, active, sweeps=SWEEPS)
        M.assert_equal(got, _run_grid(O, ld, inp0, g, st0, active, sweeps=SWEEPS), ld, H.STATE)
        _within(got["var_gamma"][:, active], M.sigmoid_ref(a[:, active]), 2, T, "sigmoid")
        if len(active) < G:
            _untouched(got, st0, G, active)


def _mix(S, ld, inp0, A, K, passes=None, bundle=None):
    T = inp0.std_beta.dtype
    passes = passes or M.n_passes(int((A <= 0).sum()), ld.m * (K + 1))
    for p in range(passes):
        mix, st0, ref, _ = M.mixture(A, ld.m, K, p) if bundle is None else bundle(p)
        got = _run_mix(S, ld, inp0, mix, st0, SWEEPS)
        M.assert_equal(got, _run_mix(O, ld, inp0, mix, st0, SWEEPS), ld, H.STATE)
        _within(got["var_gamma"], ref[:, :K], K + 4, T, "softmax")


# ---- the panel kernel, every role, the whole list -------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("low_memory, ld_dtype", LD_FORMS, ids=LD_IDS)
def test_panel_kernel_whole_list(gpu, S, low_memory, ld_dtype, model, monkeypatch):
    ld, ss, inp = _problem(tuple(PLAN), low_memory, ld_dtype, 53)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")      # teams of 8: the large class takes the narrow team strips
    monkeypatch.setenv("VIPRS_GRID_MFMA", "0")      # grid columns as panel items, not the batched matrix-core kernel
    S.clear_plan_cache()
    A = M.arguments32()
    if model == "spike_slab":
        _spike_slab_through_a_plan(ld, inp.std_beta, A, M.n_passes(A.size, ld.m))
    elif model == "grid":
        deal = lambda p: _active_columns(A, ld.m, 5, GRID_ACTIVE, p)
        _grid(S, ld, inp, A, 5, GRID_ACTIVE, M.n_passes(A.size, ld.m * len(GRID_ACTIVE)), args=deal)
    else:
        _mix(S, ld, inp, A, int(model[3:]))


def _active_columns(A, m, G, active, p):
    """(m, G) arguments whose ACTIVE columns take consecutive deals of the list (the others repeat column 0's)."""
    a = np.empty((m, G), dtype=A.dtype, order="F")
    a[:] = M.deal(A, m, 0)[:, None]
    for i, g in enumerate(active):
        a[:, g] = M.deal(A, m, p * len(active) + i)
    return a


# ---- every lane against every table entry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["spike_slab", "grid", "mix4"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_every_lane_meets_every_table_entry(gpu, S, low_memory, model, monkeypatch):
    """[130, 64, 1], 32 passes of one sweep: row r of a panel takes table entry (r + p) mod 32 -- every (lane, entry) pair of
    both lookup flavours (the chain's v_readlane and finish()'s ds_bpermute)."""
    monkeypatch.setenv("VIPRS_GRID_MFMA", "0")
    S.clear_plan_cache()
    ld, ss, inp = _problem((130, 64, 1), low_memory, np.float32, 53)
    m = ld.m
    for p in range(32):
        a = M.deal_lane_table(m, p)
        if model == "spike_slab":
            sl = M.spike_slab(inp.std_beta, a)
            got = H.run_hip(ld, sl, sl.state_copy(), sweeps=1)
            ref = H.run_oracle(ld, sl, sl.state_copy(), sweeps=1)
            M.assert_equal(got, ref, ld, H.STATE)
            assert (ref["eta_diff"] != 0).all()
            _within(got["var_gamma"], M.sigmoid_ref(a), 2, F32, "sigmoid")
        elif model == "grid":
            a2 = np.asfortranarray(np.stack([a, M.deal_lane_table(m, p + 7)], axis=1))
            g, st0 = M.grid(a2)
            act = np.array([1, 0], dtype=np.int32)
            got = _run_grid(S, ld, inp, g, st0, act, sweeps=1)
            M.assert_equal(got, _run_grid(O, ld, inp, g, st0, act, sweeps=1), ld, H.STATE)
            _within(got["var_gamma"], M.sigmoid_ref(a2), 2, F32, "sigmoid")
        else:
            mix, st0, ref, _ = M.mixture_lane_table(m, 4, p)
            got = _run_mix(S, ld, inp, mix, st0, 1)
            M.assert_equal(got, _run_mix(O, ld, inp, mix, st0, 1), ld, H.STATE)
            _within(got["var_gamma"], ref[:, :4], 8, F32, "softmax")


# ---- the batched matrix-core grid kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_batched_grid_kernel(gpu, S, low_memory, monkeypatch):
    """G = 32: every column takes its own rotation of the list (32 x 974 arguments: the whole list in one pass)."""
    monkeypatch.setenv("VIPRS_GRID_MFMA", "1")
    S.clear_plan_cache()
    ld, ss, inp = _problem((130, 780, 64), low_memory, np.float32, 33)
    _grid(S, ld, inp, M.arguments32(), 32, np.arange(32, dtype=np.int32), 1)


# ---- the band kernel and its generic twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["spike_slab", "grid", "mix4"])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("m, wl, wr, jitter", [(1500, 130, 70, 40), (64, 5, 9, 3)], ids=["ragged1500", "ragged64"])
def test_band_kernel_and_generic_kernel(gpu, S, m, wl, wr, jitter, low_memory, ld_dtype, model, monkeypatch):
    """The whole list on 1 500 SNPs; on 64 SNPs eight passes of it (the 64-SNP band is the kernel's one-panel edge)."""
    ld = banded_ld(m, wl, wr, low_memory, ld_dtype, seed=m, jitter=jitter)
    ss, inp0 = band_inputs(m)
    A = M.arguments32()
    for band in ("1", "0"):                                     # the band kernel, then the row-by-row generic kernel
        monkeypatch.setenv("VIPRS_BAND", band) if band == "0" else monkeypatch.delenv("VIPRS_BAND", raising=False)
        monkeypatch.setenv("VIPRS_GRID_MFMA", "0")
        S.clear_plan_cache()
        if model == "spike_slab":
            _spike_slab(ld, inp0.std_beta, A, min(8, M.n_passes(A.size, m)) if m == 64 else M.n_passes(A.size, m))
        elif model == "grid":
            deal = lambda p: _active_columns(A, m, 5, GRID_ACTIVE, p)
            _grid(S, ld, inp0, A, 5, GRID_ACTIVE, min(8, M.n_passes(A.size, 3 * m)), args=deal)
        else:
            _mix(S, ld, inp0, A, 4, passes=min(8, M.n_passes(int((A <= 0).sum()), 5 * m)))


@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_generic_kernel_on_dense_blocks(gpu, S, low_memory):
    """K = 33: more components than the panel kernels take."""
    ld, ss, inp = _problem((70, 333, 1), low_memory, np.float32, 31)
    _mix(S, ld, inp, M.arguments32(), 33)


# ---- the Gibbs policy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_memory, ld_dtype", [(False, np.float32), (True, np.int8)], ids=["sym-f32", "upper-i8"])
def test_gibbs_sweep_against_the_replay(gpu, S, low_memory, ld_dtype, monkeypatch):
    """Against tests/gibbs_replay (not the oracle): three columns, column 1 swept by nobody, half_var_tau = 0 -- the argument
    is u_logs[j, g], var_gamma is stored.  The draws are uploaded (with half_var_tau = 0 the device's own noise would be
    infinite): the uniforms sit ON the strict comparison gamma > U for two SNPs in three (U = gamma: left out; U = the next
    float below: included), so one unit in the last place of the chain's gamma changes eta and, through q, its block."""
    from tests import test_gpu_gibbs as GT
    from viprs_amd.stats import gibbs as GB
    ld, ss, inp = _problem(tuple(PLAN), low_memory, ld_dtype, 53)
    if low_memory and ld_dtype != np.float32:
        monkeypatch.setenv("VIPRS_TEAM0", "8")
    m, A = ld.m, M.arguments32()
    rng = np.random.default_rng(M.SEED)
    args = M.grid_args(A, m, 3, 0)
    f = np.asfortranarray
    inputs = dict(mu_mult=f(rng.uniform(0.5, 1.0, (m, 3)).astype(F32)), half_var_tau=f(np.zeros((m, 3), F32)), u_logs=args)
    _, st0 = GT._start(ss.n_per_snp, GT.PAIRS, junk_cols=(1,))
    unif, noise = GB.gibbs_draws_host(GT.SEED, 0, f(np.full((m, 3), 5e4, F32)))
    unif, noise = f(unif.astype(F32)), f(noise.astype(F32))
    gamma = GT._replay(ld, inp.std_beta, inputs, st0, [(unif, noise)], GT.ACTIVE)["var_gamma"]     # (a function of u_logs alone)
    j = np.arange(m)[:, None]
    on = (gamma > 0) & (gamma < 1)
    unif = f(np.where(on & (j % 3 == 0), gamma, np.where(on & (j % 3 == 1), np.nextafter(gamma, F32(0)), unif)).astype(F32))
    unif[:, 1] = 0
    noise[:, 1] = 0
    draws = [(unif, noise)] * SWEEPS
    want = GT._replay(ld, inp.std_beta, inputs, st0, draws, GT.ACTIVE)
    plan, st = GT._open(ld, inp.std_beta, inputs, st0)
    try:
        for i in range(SWEEPS):
            st.gibbs_upload("unif", unif)
            st.gibbs_upload("noise", noise)
            st.gibbs_sweep(ld.dq_scale, active_model_idx=np.array(GT.ACTIVE, dtype=np.int32), seed=GT.SEED, draw_index=i,
                           keep_draws=True)
        got = {k: st.download(k) for k in GT.FIELDS}
        st.close()
    finally:
        plan.close()
    for g in GT.ACTIVE:
        assert 0 < np.count_nonzero(want["eta"][:, g]) < m and np.isfinite(want["q"][:, g]).all(), g
    M.assert_equal(got, want, ld, GT.FIELDS)
    _within(got["var_gamma"][:, GT.ACTIVE], M.sigmoid_ref(args[:, GT.ACTIVE]), 2, F32, "sigmoid")
    for k in GT.FIELDS:
        assert np.array_equal(got[k][:, 1].view(np.uint32), st0[k][:, 1].view(np.uint32)), k


# ---- float64 state --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _f64_problem(low_memory):
    """[130, 64, 1, 300] with real LD and one 1-SNP block for every other argument of the float64 list."""
    ld0, ss, inp0 = _problem((130, 64, 1, 300), low_memory, np.int8, 41, F64)
    n = M.arguments64().size - ld0.m
    return M.with_singletons(ld0, n), ld0.m, np.concatenate([inp0.std_beta, np.resize(inp0.std_beta, n)])


def _both_f64_routes(S, monkeypatch, run, ld):
    monkeypatch.delenv("VIPRS_F64_ROW_BY_ROW", raising=False)
    S.clear_plan_cache()
    run()                                                           # the tile route
    monkeypatch.setenv("VIPRS_F64_ROW_BY_ROW", "1")
    S.clear_plan_cache()
    run()                                                           # row by row: exp with ballot and select in special()


@pytest.mark.parametrize("model", ["spike_slab", "grid", "mix4", "mix6", "mix12"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_float64_every_route(gpu, S, low_memory, model, monkeypatch):
    """The whole float64 list in one pass; both routes `==` the oracle, so `==` each other (mix12 is row by row on either).
    Spike-and-slab: the 1-SNP blocks of the deepest arguments take a larger std_beta (tests/test_math_range_inputs.py), so
    gamma is applied down to the subnormals."""
    from tests.test_math_range_inputs import _f64_std_beta
    ld, n_coupled, beta = _f64_problem(low_memory)
    A = M.arguments64()
    inp0 = M.spike_slab(beta, np.zeros(ld.m, F64))
    if model == "spike_slab":
        a = M.deal(A, ld.m, 0)
        b = _f64_std_beta(beta, M.sigmoid_ref(a), n_coupled)
        run = lambda: _spike_slab(ld, b, A, 1)
    elif model == "grid":
        run = lambda: _grid(S, ld, inp0, A, 3, np.array([2, 0], dtype=np.int32), 1)
    else:
        run = lambda: _mix(S, ld, inp0, A, int(model[3:]), passes=1)
    _both_f64_routes(S, monkeypatch, run, ld)


# ---- SuSiE ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ["float32", "float64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_susie_weights_against_the_replay(gpu, low_memory, T):
    """Against tests/susie_replay (not the oracle): L = 1, one iteration, fixed prior variance, z = 0 -- w_j = log_prior[j];
    with one SNP of each block at 0, w_j - wmax is the argument itself and alpha_j = exp(w_j) / S.  Blocks of 300 and 64;
    the arguments are entries <= 0 of the float64 list, the special ranges of exp first (|x| < 2^-54, the subnormal results
    below -708.4, underflow, -inf) and eight deals of the rest."""
    from tests import susie_replay as SR
    from viprs_amd.plan import LDPlan
    ld, _, _ = _problem((300, 64), low_memory, np.float32, 29)
    A = M.arguments64()
    neg = A[A <= 0]
    deep = np.sort(neg[(neg < -700) & (neg >= -745.14)])
    first = np.concatenate([neg[neg > -1e-15], neg[neg < -745.14], deep[::deep.size // 280], M.deal(neg, 400, 0)])
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)
    try:
        for p in range(8):
            lp = (first[:ld.m] if p == 0 else M.deal(neg, ld.m, p)).copy()
            lp[[7, 300 + 63]] = 0.0                                 # the maximum of each block
            z = np.zeros(ld.m)
            want = SR.susie_replay(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, z, 1, 50.0, False, lp,
                                   ld.dq_scale, 1e-4, 1, T)
            got = plan.susie(z, 1, 50.0, False, log_prior=lp, dq_scale=ld.dq_scale, tol=1e-4, max_iter=1, float_precision=T)
            for f in ("alpha", "mu", "prior_variance", "post_var", "iterations", "delta", "status"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (p, f, M.first_difference(
                    dict(a=np.asarray(getattr(got, f))), dict(a=np.asarray(getattr(want, f))), ld) if f in ("alpha", "mu") else None)
            e = np.exp(lp.astype(np.longdouble))
            for s, t in ((0, 300), (300, 364)):
                ref = e[s:t] / e[s:t].sum()
                # float64: exp < 1 unit, n - 1 adds and a divide in double; float32 state: the same, rounded once
                _within(got.alpha[s:t, 0], ref, (t - s) + 3 if T == "float64" else 1, np.dtype(T), "alpha")
    finally:
        plan.close()


# ---- math_mode = "fast" ---------------------------------------------------------------------------------------------------------
def _fast_against_exact(fast, exact, what, both=None):
    """var_gamma of the fast kernels against the exact ones': 1e-5 relative where the exact result is a normal number, 2^-126
    absolute below (v_exp_f32 flushes denormals).  Returns the largest relative difference."""
    f, e = fast.astype(np.float64), exact.astype(np.float64)
    if both is not None:
        f, e = f[both], e[both]
    assert np.isfinite(f).all(), what
    normal = e >= np.finfo(F32).tiny
    rel = float((np.abs(f - e)[normal] / e[normal]).max())
    small = float(np.abs(f - e)[~normal].max()) if (~normal).any() else 0.0
    print(f"math_mode=fast, {what}: max relative difference {rel:.3e} over {int(normal.sum())} normal results, "
          f"max absolute difference below FLT_MIN {small:.3e}")
    assert rel <= 1e-5 and small <= 2.0 ** -126, (what, rel, small)
    return rel


@pytest.mark.parametrize("model", ["spike_slab", "grid", "mix4", "batched_grid"])
def test_fast_mode_over_the_whole_list(gpu, S, model, monkeypatch):
    monkeypatch.setenv("VIPRS_GRID_MFMA", "1" if model == "batched_grid" else "0")
    ld, ss, inp = _problem((130, 780, 64) if model == "batched_grid" else tuple(PLAN), False, np.float32, 53)
    A = M.arguments32()
    m = ld.m

    def in_both_modes(run):
        out = []
        for mode in ("exact", "fast"):
            S.clear_plan_cache()
            S.set_default_math_mode(mode)
            out.append(run())
            if mode == "fast":
                assert S.plan_for(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory).effective_math_mode() == "fast"
        return out
    if model == "spike_slab":
        for p in range(M.n_passes(A.size, m)):
            sl = M.spike_slab(inp.std_beta, M.deal(A, m, p))

            def run():
                st, seen = sl.state_copy(), np.zeros(m, dtype=bool)
                for _ in range(SWEEPS):
                    st = H.run_hip(ld, sl, st, sweeps=1)
                    seen |= st["eta_diff"] != 0
                return st["var_gamma"], seen
            (e, se), (f, sf) = in_both_modes(run)
            _fast_against_exact(f, e, f"panel spike-and-slab, pass {p}", both=se & sf)
    elif model == "mix4":
        for p in range(M.n_passes(int((A <= 0).sum()), m * 5)):
            mix, st0, _, _ = M.mixture(A, m, 4, p)
            e, f = in_both_modes(lambda: _run_mix(S, ld, inp, mix, st0, SWEEPS)["var_gamma"])
            _fast_against_exact(f, e, f"panel mix4, pass {p}")
    else:
        G, active = (32, np.arange(32, dtype=np.int32)) if model == "batched_grid" else (5, GRID_ACTIVE)
        for p in range(M.n_passes(A.size, m * len(active))):
            g, st0 = M.grid(_active_columns(A, m, G, active, p))
            e, f = in_both_modes(lambda: _run_grid(S, ld, inp, g, st0, active, sweeps=SWEEPS)["var_gamma"][:, active])
            _fast_against_exact(f, e, f"{model}, pass {p}")
