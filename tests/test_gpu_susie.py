"""SuSiE fine-mapping `viprs_plan_susie` (include/viprs_hip.h) on the device: every bit against the replay of the header's
step (tests/susie_replay.py), windowed LD, per-block stopping, determinism / independence, a call between two sweeps, the
model layer (`SuSiE`) against the host fit, and the refusals that need a plan."""
import ctypes
import functools

import numpy as np
import pytest

from tests import ridge_reference as RR
from tests import susie_replay as SR
from tests.test_gpu_ridge import CASES, SIZES, _arrays, _ld, _sweep_state
from tests.test_susie_reference import MEASURED, ar1_blocks
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

FIELDS = ("alpha", "mu", "prior_variance", "post_var", "iterations", "delta", "status")
BIT_CASES = ("ar1-fp32-sym", "ar1-fp32-upper", "longrange-int8-sym", "longrange-int8-upper")


def _plan(lb, ip, data, low_memory):
    from viprs_amd.plan import LDPlan
    return LDPlan(lb, ip, data, low_memory)


def _z_scores(m, seed=41, sd=3.0):
    """z-scores with a few strong signals: N(0, sd^2) -- a handful of |z| > 8 among thousands."""
    return sd * np.random.default_rng(seed).standard_normal(m)


def _same(name, got, want):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, f, a.dtype, b.dtype, a.shape, b.shape)
        bad = a != b
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            block = int(np.searchsorted(want.block_start, at[0], side="right") - 1) if a.shape[0] == want.alpha.shape[0] else at[0]
            raise AssertionError(f"{name}: {f} differs in {int(bad.sum())} entries, first at {at} (block {block}): device "
                                 f"{a[at]!r} replay {b[at]!r}")


@functools.lru_cache(maxsize=None)
def _replayed(case, T, L, estimate):
    ld, _ = _ld(case)
    z = _z_scores(ld.ld_left_bound.shape[0])
    return z, SR.susie_replay(*_arrays(ld), z, L, 50.0, estimate, None, ld.dq_scale, 1e-4, 6, T)


@pytest.mark.parametrize("T", ["float32", "float64"])
@pytest.mark.parametrize("estimate", [True, False], ids=["em", "fixed"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("case", BIT_CASES)
def test_bits_are_the_replayed_step(gpu, case, L, estimate, T):
    """`alpha`, `mu`, `prior_variance`, `post_var`, `iterations`, `delta` and `status` `==` the replay, over block sizes of
    one chunk, one wavefront, one pass of the workgroup, several passes and partial last chunks (SIZES of the ridge tests);
    `max_iter = 6` keeps the replay within seconds (blocks that converge earlier freeze on the way)."""
    ld, _ = _ld(case)
    z, want = _replayed(case, T, L, estimate)
    plan = _plan(*_arrays(ld))
    try:
        got = plan.susie(z, L, 50.0, estimate, dq_scale=ld.dq_scale, tol=1e-4, max_iter=6, check_every=2, float_precision=T)
        ms, steps, step_ms = plan.last_susie_ms()
    finally:
        plan.close()
    print(case, T, "L", L, "iterations", want.iterations.tolist(), "status", want.status.tolist())
    assert np.array_equal(got.block_start, np.concatenate([[0], np.cumsum(SIZES)]))
    _same(f"{case} {T} L={L} estimate={estimate}", got, want)
    assert got.ms == ms > 0.0 and step_ms > 0.0 and steps == L * min(6, 2 * -(-int(got.iterations.max()) // 2))


@pytest.mark.parametrize("T", ["float32", "float64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_windowed_ld(gpu, low_memory, T):
    lb, ip, data = RR.banded_ar1(2500, 0.95, 40, low_memory)
    z = _z_scores(2500, seed=42)
    want = SR.susie_replay(lb, ip, data, low_memory, z, 2, 50.0, True, None, 1.0, 1e-4, 4, T)
    plan = _plan(lb, ip, data, low_memory)
    try:
        got = plan.susie(z, 2, 50.0, True, tol=1e-4, max_iter=4, float_precision=T)
    finally:
        plan.close()
    assert got.block_start.tolist() == [0, 2500]
    _same(f"banded low_memory={low_memory} {T}", got, want)


# ---- per-block stopping ---------------------------------------------------------------------------------------------------
STOP_SIZES, STOP_RHOS = (63, 65, 257, 130), (0.5, 0.9, 0.97, 0.9)


@functools.lru_cache(maxsize=None)
def _stopping_problem():
    """Four AR(1) blocks (upper form): one clean planted effect, z = 0, noisy z-scores under rho = 0.97 (the slow block), two
    planted effects in LD with each other; block 1 excludes a SNP."""
    from viprs_amd.stats import susie as S
    lb, ip, data = ar1_blocks(STOP_SIZES, STOP_RHOS, low_memory=True)
    starts = np.concatenate([[0], np.cumsum(STOP_SIZES)])
    z = np.zeros(int(starts[-1]))
    R = [S.block_matrix(lb, ip, data, True, int(s), int(e)) for s, e in zip(starts[:-1], starts[1:])]
    b0 = np.zeros(63)
    b0[30] = 9.0
    z[0:63] = R[0] @ b0
    z[128:385] = _z_scores(257, seed=43, sd=2.5)
    b3 = np.zeros(130)
    b3[[40, 43]] = 6.0, 5.0
    z[385:] = R[3] @ b3
    lp = np.concatenate([np.full(n, -np.log(float(n))) for n in STOP_SIZES])
    lp[63:128] = -np.log(64.0)
    lp[70] = -np.inf
    return lb, ip, data, z, lp, starts


def _block_alone(lb, ip, data, s, e):
    o0, o1 = int(ip[s]), int(ip[e])
    return (lb[s:e] - s).astype(np.int32), (ip[s:e + 1] - o0).astype(np.int64), np.ascontiguousarray(data[o0:o1])


@pytest.mark.parametrize("T", ["float32", "float64"])
def test_per_block_stopping_independence_and_determinism(gpu, T):
    """Blocks that converge at different iterations, and one that is cut at max_iter = 2: every block's outputs are those of
    the same block fitted alone in a one-block plan, whatever `check_every` is, and a second call repeats the bits."""
    lb, ip, data, z, lp, starts = _stopping_problem()
    kw = dict(L=3, prior_variance=50.0, estimate_prior_variance=True, log_prior=lp, tol=1e-4, float_precision=T)
    plan = _plan(lb, ip, data, True)
    try:
        full = plan.susie(z, max_iter=40, check_every=1, **kw)
        again = plan.susie(z, max_iter=40, check_every=1, **kw)
        every5 = plan.susie(z, max_iter=40, check_every=5, **kw)
        cut = plan.susie(z, max_iter=2, check_every=1, **kw)
        cut5 = plan.susie(z, max_iter=2, check_every=5, **kw)
        plan.set_active_blocks(np.arange(plan.n_blocks) % 2 == 0)
        filtered = plan.susie(z, max_iter=40, **kw)
        plan.set_active_blocks(None)
    finally:
        plan.close()
    print(T, "iterations", full.iterations.tolist(), "status", full.status.tolist(), "cut", cut.iterations.tolist(),
          cut.status.tolist())
    assert full.converged and len(set(full.iterations.tolist())) >= 3 and full.iterations[1] == 2
    assert np.all(full.alpha[63:128][np.arange(65) != 7] == full.alpha[63, 0]) and np.all(full.alpha[70] == 0.0)
    assert np.all(full.mu[63:128] == 0.0)
    _same("a repeated call", again, full)
    _same("check_every=5", every5, full)
    _same("the active-block filter of the sweeps", filtered, full)
    _same("max_iter=2, check_every=5", cut5, cut)
    assert cut.status.tolist() == [int(n > 2) for n in full.iterations] and not cut.converged
    assert np.all(cut.iterations == 2)
    for k in range(4):
        s, e = int(starts[k]), int(starts[k + 1])
        alone = _plan(*_block_alone(lb, ip, data, s, e), True)
        try:
            for name, whole, max_iter in (("full", full, 40), ("cut", cut, 2)):
                one = alone.susie(z[s:e], max_iter=max_iter, **dict(kw, log_prior=lp[s:e]))
                for f in FIELDS:
                    w = getattr(whole, f)
                    w = w[s:e] if f in ("alpha", "mu") else w[k:k + 1]
                    assert np.array_equal(getattr(one, f), w), (name, k, f)
        finally:
            alone.close()
    # the replay agrees on the run to convergence too (float64: the exp, the sums and the product over tens of iterations)
    want = SR.susie_replay(lb, ip, data, True, z, 3, 50.0, True, lp, 1.0, 1e-4, 40, T)
    _same(f"to convergence {T}", full, want)


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_call_between_sweeps_leaves_the_sweeps_alone(gpu, T):
    """Upper form: the fp32 and the float64 sweeps keep the dense blocks in different storages; a fit between two sweeps
    reads whichever is there, like the product, and must not disturb what the second sweep computes."""
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=[500, 130, 1700], low_memory=True, seed=3, kind="longrange", float_precision=T)
    z = _z_scores(2330, seed=44)
    want = SR.susie_replay(*_arrays(ld), z, 2, 50.0, True, None, ld.dq_scale, 1e-4, 3, "float32")
    out = []
    for with_fit in (False, True):
        plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
        try:
            st = _sweep_state(plan, inp, T)
            st.e_step(ld.dq_scale)
            if with_fit:
                _same("between sweeps", plan.susie(z, 2, 50.0, True, dq_scale=ld.dq_scale, max_iter=3), want)
            st.e_step(ld.dq_scale)
            out.append({k: st.download(k) for k in ("var_gamma", "var_mu", "eta", "q", "eta_diff")})
        finally:
            plan.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_model_layer(gpu):
    """`SuSiE(gdl).fit()` on the device against the `fit_fn = susie_host` backend: PIP and bbar within 10 x the measured
    distance of the replay from `susie_host` (tests/test_susie_reference.py), identical credible sets, the planted effects."""
    from tests.test_susie_model import PLANTED, loader
    from viprs_amd.model import SuSiE
    from viprs_amd.stats import susie as S
    gdl = loader()
    dev = SuSiE(gdl, L=4, dequantize_on_the_fly=True).fit()
    host = SuSiE(gdl, L=4, dequantize_on_the_fly=True, fit_fn=S.susie_host).fit()
    assert dev.info.converged and dev.info.ms > 0.0 and dev.info.alpha.dtype == np.float32
    bb = lambda mdl: np.sum(mdl.info.alpha.astype(np.float64) * mdl.info.mu.astype(np.float64), axis=1)
    d_pip = max(float(np.max(np.abs(dev.pip[c] - host.pip[c]))) for c in (1, 2))
    d_bbar = float(np.max(np.abs(bb(dev) - bb(host))))
    print("max |dPIP|", d_pip, "max |dbbar|", d_bbar, "iterations", dev.info.iterations.tolist(), host.info.iterations.tolist())
    assert d_pip <= 10 * MEASURED["float32"][0] and d_bbar <= 10 * MEASURED["float32"][1]
    assert np.array_equal(dev.info.iterations, host.info.iterations)
    sets_d, sets_h = dev.credible_sets(), host.credible_sets()
    assert [(cs["block"], cs["effect"], cs["snps"].tolist()) for cs in sets_d] == \
           [(cs["block"], cs["effect"], cs["snps"].tolist()) for cs in sets_h]
    assert [(cs["chromosome"], cs["index"].tolist()) for cs in sets_d] == [(1, [20]), (1, [150]), (2, [45])]
    for c, eff in PLANTED.items():
        assert all(dev.pip[c][j] > 0.99 for j in eff)
    assert dev.to_table()["CS"].to_numpy().nonzero()[0].tolist() == [20, 150, 230]


# ---- the refusals that read the plan, and the empty plan --------------------------------------------------------------------
def test_bad_values_are_refused_before_any_launch(gpu):
    from viprs_amd import _lib as L
    lb, ip, data = ar1_blocks((5, 3), (0.5, 0.5))
    plan = _plan(lb, ip, data, False)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    try:
        def call(z=None, lp=None, v=None):
            z = np.ones(8) if z is None else z
            alpha, mu = np.full((8, 2), 7.0, np.float32, order="F"), np.full((8, 2), 7.0, np.float32, order="F")
            out = (np.full(4, -5.0), np.full(4, -5.0), np.full(2, -5, np.int32), np.full(2, -5.0), np.full(2, -5, np.int32))
            rc = L.lib.viprs_plan_susie(plan.handle, L.F32, 2, p(z), p(lp), p(v), 50.0, 1, 1.0, 1e-4, 5, 1, p(alpha), p(mu),
                                        *(p(o) for o in out))
            untouched = np.all(alpha == 7.0) and np.all(mu == 7.0) and all(np.all(o == -5) for o in out)
            return rc, L.last_error(), untouched

        def with_value(n, at, value, fill=1.0):
            a = np.full(n, fill)
            a[at] = value
            return a

        uniform = np.concatenate([np.full(5, -np.log(5.0)), np.full(3, -np.log(3.0))])
        block = uniform.copy()
        block[5:] = -np.inf
        for kw, word in ((dict(z=with_value(8, 3, np.nan)), "z must"), (dict(z=with_value(8, 7, np.inf)), "z must"),
                         (dict(lp=with_value(8, 2, np.nan, -1.0)), "log_prior"), (dict(lp=with_value(8, 2, np.inf, -1.0)), "log_prior"),
                         (dict(lp=block), "every SNP"),
                         (dict(v=with_value(4, 3, -1.0)), "prior variance"), (dict(v=with_value(4, 0, np.nan)), "prior variance"),
                         (dict(v=with_value(4, 1, np.inf)), "prior variance")):
            rc, msg, untouched = call(**kw)
            assert rc == L.EINVAL and word in msg and untouched, (kw, rc, msg)
        one = uniform.copy()
        one[6] = -np.inf                                        # (one excluded SNP is legal)
        rc, _, untouched = call(lp=one, v=with_value(4, 1, 0.0))
        assert rc == L.OK and not untouched
    finally:
        plan.close()


def test_empty_plan(gpu):
    plan = _plan(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.float32), False)
    try:
        info = plan.susie(np.zeros(0), L=3)
    finally:
        plan.close()
    assert info.alpha.shape == (0, 3) and info.status.shape == (0,) and info.converged and info.ms == 0.0
