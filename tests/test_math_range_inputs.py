"""CPU: the argument lists of tests/math_range_inputs.py -- what they cover, that the recipe keeps small results visible, the
oracle's distance to a long-double sigmoid / softmax on them, and that the serial chain's own gamma is seen in the result.
Conditions on the recipe, met by the reference alone (the restated oracle, and the compiled reference where oracle/_ref
exists): the GPU cases of tests/test_gpu_math_range.py compare the kernels with that oracle `==` on the same bundles."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import math_range_inputs as M
from tests.test_gpu_models import _run_grid, _run_mix
from tests.test_per_snp_inputs import _Kind
from viprs_amd.utils import synthetic as syn

PLAN = [2370, 1601, 130, 64, 1]             # tests/test_gpu_panel_roles.py
B1601, B130, B64 = 1, 2, 3
SWEEPS = 2
KINDS = ["restated", pytest.param("reference", marks=pytest.mark.skipif(
    not O.have_reference(), reason="oracle/_ref not built (needs the reference's sources)"))]
needs_long_double = pytest.mark.skipif(not M.have_long_double(), reason="no extended-precision long double on this host")
F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _plan_problem():
    return syn.make_problem(sizes=PLAN, low_memory=False, seed=53, kind="longrange")


@functools.lru_cache(maxsize=None)
def _f64_problem():
    """[130, 64, 1, 300] with real LD and one 1-SNP block for every other argument of the float64 list."""
    ld0, ss, inp0 = syn.make_problem(sizes=[130, 64, 1, 300], low_memory=False, ld_dtype=np.int8, seed=41, kind="longrange",
                                     float_precision=F64)
    n = M.arguments64().size - ld0.m
    return M.with_singletons(ld0, n), ld0.m, np.concatenate([inp0.std_beta, np.resize(inp0.std_beta, n)])


def spike_slab_sweeps(run, ld, inp):
    """`SWEEPS` sweeps one at a time: (the final state, per sweep the SNPs that were applied -- eta_diff != 0)."""
    st, applied = inp.state_copy(), []
    for _ in range(SWEEPS):
        st = run(ld, inp, st)
        applied.append(st["eta_diff"] != 0)
    return st, applied


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_float32_list_covers_every_k_of_the_reduction():
    A = M.arguments32()
    assert A.dtype == F32 and 20000 <= A.size <= 25000 and not np.isnan(A).any()
    assert np.array_equal(A.view(np.uint32), M.arguments32().view(np.uint32))                  # deterministic
    assert np.unique(A.view(np.uint32)).size == A.size
    k = M.reduction_k32(A)
    assert np.array_equal(np.unique(k), np.arange(-4801, 1))       # so every table index and every exponent shift occurs
    assert np.array_equal(np.unique(k & 31), np.arange(32)) and (k >> 5).min() == -151 and (k >> 5).max() == 0
    # both sides of every boundary (k - 1/2) c: some argument of interval k lies within 2 float32 steps of its lower end
    neg = np.sort(A[(A <= 0) & (A >= -104)])
    kk = M.reduction_k32(neg)
    step = np.nonzero(np.diff(kk))[0]
    assert step.size == 4801 and np.all(np.nextafter(neg[step], F32(np.inf)) == neg[step + 1])
    for x in (0.0, M.TINY32, -M.TINY32, np.finfo(F32).tiny, -104.0, np.nextafter(F32(-104), F32(-200)), -np.inf, np.inf,
              float.fromhex("-0x1.9fe368p6"), -np.finfo(F32).max, 88.7, 104.0):
        assert (A == F32(x)).any(), x
    assert (A.view(np.uint32) == 0x80000000).any() and (A.view(np.uint32) == 0).any()          # -0 and +0


def test_float64_list_reaches_every_branch_of_special():
    A = M.arguments64()
    assert A.dtype == F64 and A.size <= 170000 and not np.isnan(A).any()
    x = -np.abs(A)                                                  # what the sigmoid hands to exp
    abstop = (x.view(np.uint64) & np.uint64(0x7fffffffffffffff)) >> np.uint64(52)
    tiny, sub, under = abstop < 0x3c9, (x > -1024) & (x <= -512), x <= -1024
    print(f"float64 list: {A.size} arguments; |x| < 2^-54: {tiny.sum()}, (-1024, -512]: {sub.sum()}, <= -1024: {under.sum()}")
    assert tiny.sum() >= 10 and sub.sum() >= 40000 and under.sum() >= 4
    e = np.array([O.exp_model(v) for v in x[sub][::7]])
    assert ((e > 0) & (e < np.finfo(F64).tiny)).sum() >= 500 and (e == 0).any() and (e >= np.finfo(F64).tiny).any()
    assert all(O.exp_model(v) == 0.0 for v in x[under]) and all(O.exp_model(v) == 1.0 + v for v in x[tiny])
    k = np.rint(x[(x >= -745.2)] / M.C64).astype(np.int64)          # one interior point per interval of ln2 / 128
    assert np.array_equal(np.unique(k), np.arange(k.min(), 1)) and k.min() <= -137612


@pytest.mark.parametrize("b", [130, 64])
def test_lane_table_arguments_meet_every_row_of_a_panel(b):
    x = M.lane_table_arguments()
    assert np.array_equal(np.sort(M.reduction_k32(x) & 31), np.arange(32))         # one argument per table entry
    assert np.array_equal(M.reduction_k32(x), -(np.arange(32) + 231))
    pairs = set()
    for p in range(32):
        a = M.deal_lane_table(sum([130, 64, 1]), p)
        s = 0 if b == 130 else 130
        pairs |= {(r % 64, int(t)) for r, t in zip(range(b), M.reduction_k32(a[s:s + b]) & 31)}
    assert len(pairs) == min(b, 64) * 32


# ---- visibility, result classes and the oracle's distance to the long-double reference ------------------------------------------
@needs_long_double
@pytest.mark.parametrize("kind", KINDS)
def test_float32_spike_slab_keeps_small_results_visible(kind):
    ld, ss, inp0 = _plan_problem()
    A = M.arguments32()
    run = lambda ld, inp, st: H.run_oracle(ld, inp, st, kind=kind, sweeps=1)
    visible = hidden = 0
    worst, max_q, results = 0.0, 0.0, []
    for p in range(M.n_passes(A.size, ld.m)):
        a = M.deal(A, ld.m, p)
        ref = M.sigmoid_ref(a)
        st, applied = spike_slab_sweeps(run, ld, M.spike_slab(inp0.std_beta, a))
        assert all(np.isfinite(v).all() for v in st.values())
        seen = applied[0] | applied[1]                              # per (pass, SNP): a wrapped-round argument counts twice
        vis = ref >= M.TINY32
        visible, hidden = visible + int(vis.sum()), hidden + int((vis & ~seen).sum())
        worst = max(worst, float(M.distance(st["var_gamma"][seen], ref[seen], F32).max()))
        max_q = max(max_q, float(np.abs(st["q"]).max()))
        results.append(st["var_gamma"][seen])
    g = np.unique(np.concatenate(results))
    fi = np.finfo(F32)
    classes = dict(denormal=int(((g > 0) & (g < fi.tiny)).sum()), below_eps=int(((g >= fi.tiny) & (g < fi.eps)).sum()),
                   upper_half=int(((g > 0.5) & (g < 1)).sum()), one=int((g == 1).sum()))
    print(f"{kind}: skipped in both sweeps {hidden} of {visible} = {hidden / visible:.4f}; max |q| {max_q:.3f}; applied results "
          f"within {worst:.3f} units of the long-double sigmoid; distinct applied results {classes}")
    assert hidden <= 0.10 * visible and max_q < 1
    assert worst <= 2
    assert classes["denormal"] >= 1000 and classes["below_eps"] >= 1000 and classes["upper_half"] >= 1000 and classes["one"]


@needs_long_double
@pytest.mark.parametrize("kind", KINDS)
def test_float32_grid_stores_every_result(kind):
    """No skip branch: all result classes, exact 0 included, are stored."""
    ld, ss, inp0 = _plan_problem()
    A = M.arguments32()
    G = 3
    active = np.arange(G, dtype=np.int32)
    worst, results = 0.0, []
    for p in range(M.n_passes(A.size, ld.m * G)):
        a = M.grid_args(A, ld.m, G, p)
        g, st0 = M.grid(a)
        st = _run_grid(_Kind(kind), ld, inp0, g, st0, active, sweeps=SWEEPS)
        assert all(np.isfinite(v).all() for v in st.values()) and float(np.abs(st["q"]).max()) < 1
        worst = max(worst, float(M.distance(st["var_gamma"], M.sigmoid_ref(a), F32).max()))
        results.append(st["var_gamma"].ravel())
    g = np.unique(np.concatenate(results))
    fi = np.finfo(F32)
    print(f"{kind}: grid results within {worst:.3f} units; {int(((g > 0) & (g < fi.tiny)).sum())} distinct denormals")
    assert worst <= 2
    assert (g == 0).any() and ((g > 0) & (g < fi.tiny)).sum() >= 1000 and ((g >= fi.tiny) & (g < fi.eps)).any()
    assert ((g > 0.5) & (g < 1)).any() and (g == 1).any()


@needs_long_double
@pytest.mark.parametrize("K", [3, 4, 6, 12, 20])
@pytest.mark.parametrize("kind", KINDS)
def test_float32_softmax_within_K_plus_4_units(kind, K):
    ld, ss, inp0 = _plan_problem()
    A = M.arguments32()
    neg = int((A <= 0).sum())
    worst, denormal, arg_lo = 0.0, 0, 0.0
    for p in range(min(2, M.n_passes(neg, ld.m * (K + 1)))):
        mix, st0, ref, arg = M.mixture(A, ld.m, K, p)
        u = np.concatenate([mix["u_logs"], mix["log_null_pi"][:, None]], axis=1)
        j = np.arange(ld.m)
        assert (u[j, j % (K + 1)] == u.max(axis=1)).all()                              # the maximum visits every slot
        assert (arg.max(axis=1) == 0).all() and (arg[1::2] != np.round(arg[1::2])).any()
        st = _run_mix(_Kind(kind), ld, inp0, mix, st0, SWEEPS)
        assert all(np.isfinite(v).all() for v in st.values()) and float(np.abs(st["q"]).max()) < 1
        worst = max(worst, float(M.distance(st["var_gamma"], ref[:, :K], F32).max()))
        denormal += int(((st["var_gamma"] > 0) & (st["var_gamma"] < np.finfo(F32).tiny)).sum())
        arg_lo = min(arg_lo, float(arg[np.isfinite(arg)].min()))
    print(f"{kind} K={K}: softmax within {worst:.3f} units of long double ({K + 4} allowed); {denormal} denormal results")
    assert worst <= K + 4 and denormal >= 100


def _f64_std_beta(beta, gamma_ref, n_coupled):
    """The 1-SNP blocks (q stays 0 there) whose gamma 2^1000 falls below 1 take a larger std_beta: gamma mu keeps the
    magnitude of the others' as far down as 2^22 reaches (gamma >= 2^-1022 2^-22; below that mu would overflow)."""
    with np.errstate(divide="ignore"):
        up = np.clip(np.floor(-np.log2(np.maximum(gamma_ref, M.TINY64)).astype(F64)) - 1000, 0, 22)
    up[:n_coupled] = 0
    return np.ldexp(beta, up.astype(np.int64))


@needs_long_double
@pytest.mark.parametrize("kind", KINDS)
def test_float64_spike_slab_keeps_small_results_visible(kind):
    ld, n_coupled, beta = _f64_problem()
    A = M.arguments64()
    a = M.deal(A, ld.m, 0)
    ref = M.sigmoid_ref(a)
    inp = M.spike_slab(_f64_std_beta(beta, ref, n_coupled), a)
    run = lambda ld, inp, st: H.run_oracle(ld, inp, st, kind=kind, sweeps=1)
    st, applied = spike_slab_sweeps(run, ld, inp)
    assert all(np.isfinite(v).all() for v in st.values()) and float(np.abs(st["q"]).max()) < 1
    seen = applied[0] | applied[1]
    vis = ref >= M.TINY64
    hidden = int((vis & ~seen).sum())
    worst = float(M.distance(st["var_gamma"][seen], ref[seen], F64).max())
    g = st["var_gamma"][seen]
    sub = int(((g > 0) & (g < np.finfo(F64).tiny)).sum())
    print(f"{kind}: float64 skipped in both sweeps {hidden} of {int(vis.sum())} = {hidden / vis.sum():.4f}; applied results within "
          f"{worst:.3f} units; {sub} applied subnormal results, smallest applied {g[g > 0].min():.3e}")
    assert hidden <= 0.10 * vis.sum() and worst <= 2 and sub >= 1000 and (g == 1).any() and (g < 1e-8).any()


# ---- the restatement against the reference on these bundles ---------------------------------------------------------------------
@pytest.mark.skipif(not O.have_reference(), reason="oracle/_ref not built (needs the reference's sources)")
@needs_long_double
@pytest.mark.parametrize("model", ["spike_slab", "grid", "mix4"])
@pytest.mark.parametrize("T", [F32, F64], ids=["f32", "f64"])
def test_restatement_equals_the_reference(T, model):
    if T == F32:
        ld, ss, inp0 = _plan_problem()
        beta = inp0.std_beta
    else:
        ld, _, beta = _f64_problem()
    inp0 = M.spike_slab(beta, np.zeros(ld.m, T))
    A = M.arguments(T)
    for p in range(2):
        if model == "spike_slab":
            inp = M.spike_slab(beta, M.deal(A, ld.m, p))
            got, ref = (H.run_oracle(ld, inp, inp.state_copy(), kind=k, sweeps=SWEEPS) for k in ("restated", "reference"))
        elif model == "grid":
            g, st0 = M.grid(M.grid_args(A, ld.m, 2, p))
            got, ref = (_run_grid(_Kind(k), ld, inp0, g, st0, np.arange(2, dtype=np.int32), sweeps=SWEEPS)
                        for k in ("restated", "reference"))
        else:
            mix, st0, _, _ = M.mixture(A, ld.m, 4, p)
            got, ref = (_run_mix(_Kind(k), ld, inp0, mix, st0, SWEEPS) for k in ("restated", "reference"))
        M.assert_equal(got, ref, ld, H.STATE)


# ---- the chain is seen ----------------------------------------------------------------------------------------------------------
def _others_change(sub, beta, a, row, T=F32):
    """Does moving row `row`'s argument by c (one table entry, 2.2 % in gamma) change q or eta_diff of another SNP of the block?
    mu_mult stays what the unmoved argument gave it: the function value alone moves."""
    inp = M.spike_slab(beta, a)
    base = H.run_oracle(sub, inp, inp.state_copy(), sweeps=SWEEPS)
    inp.u_logs = a.copy()
    inp.u_logs[row] -= T(M.C32)
    moved = H.run_oracle(sub, inp, inp.state_copy(), sweeps=SWEEPS)
    other = np.arange(a.size) != row
    return bool(((moved["q"] != base["q"]) | (moved["eta_diff"] != base["eta_diff"]))[other].any())


@needs_long_double
def test_one_argument_moved_by_c_changes_another_snp_of_its_block():
    """finish() of the panel kernel recomputes gamma per lane and stores it; the serial chain's own gamma (the other lookup
    flavour) reaches the output only through d and q.  With the real LD kept, every row position's argument is seen there."""
    ld, ss, inp0 = _plan_problem()
    for bi in (B64, B130, B1601):
        sub, s, e = M.block_problem(ld, bi)
        b = e - s
        a = M.deal_lane_table(b, 0)                                 # results near 0.005: every row is applied
        rows = range(b) if b <= 130 else sorted({r for p in range(0, b, 64) for r in (p, min(p + 63, b - 1))})
        for row in rows:
            assert _others_change(sub, inp0.std_beta[s:e], a, row), (bi, row)
