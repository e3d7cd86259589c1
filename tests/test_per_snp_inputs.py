"""CPU: the per-SNP inputs of tests/per_snp_inputs.py -- the restatement `==` the compiled reference on them, the proof that
they discriminate (exchanging neighbouring SNPs' inputs changes every block's result, which the constant inputs of every other
test cannot show), and the conditions the recipe has to keep for the GPU cases of tests/test_gpu_per_snp_inputs.py to mean
what they say."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import enet_replay as ER
from tests import gibbs_replay as GR
from tests import helpers as H
from tests import per_snp_inputs as P
from tests.test_gpu_models import _run_grid, _run_mix
from tests.test_oracle_vs_ref import _grid_inputs, _mixture_inputs
from viprs_amd.stats import gibbs as GB
from viprs_amd.utils import synthetic as syn

needs_ref = pytest.mark.skipif(not O.have_reference(), reason="oracle/_ref not built (needs the reference's sources)")
PLAN = [2370, 1601, 130, 64, 1]             # tests/test_gpu_panel_roles.py
B130, B64 = 2, 3                            # the blocks of PLAN the conditions name
SWEEPS = 2


class _Kind:
    """`oracle.oracle` with `kind` bound: what `_run_mix` / `_run_grid` take as their module."""

    def __init__(self, kind):
        self.kind = kind

    def cpp_e_step_mixture(self, *a):
        return O.cpp_e_step_mixture(*a, kind=self.kind)

    def cpp_e_step_grid(self, *a):
        return O.cpp_e_step_grid(*a, kind=self.kind)


# ---- the restatement against the reference --------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("model", ["spike_slab", "mix4", "grid8"])
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_restatement_equals_the_reference(low_memory, T, model):
    ld, ss, inp0 = syn.make_problem(sizes=[130, 64, 1, 257], low_memory=low_memory, seed=29, kind="longrange",
                                    float_precision=T)
    if model == "spike_slab":
        inp = P.spike_slab(ss.std_beta, T)
        st0 = inp.state_copy()
        got, ref = (H.run_oracle(ld, inp, st0, kind=k, sweeps=SWEEPS) for k in ("restated", "reference"))
        assert 0 < int((ref["eta_diff"] == 0).sum()) < ld.m              # both branches
    elif model == "mix4":
        mix, st0 = P.mixture(ld.m, 4, T)
        got, ref = (_run_mix(_Kind(k), ld, inp0, mix, st0, SWEEPS) for k in ("restated", "reference"))
    else:
        g, st0 = P.grid(ld.m, 8, T)
        active = np.array([5, 1, 6], dtype=np.int32)
        got, ref = (_run_grid(_Kind(k), ld, inp0, g, st0, active, sweeps=SWEEPS) for k in ("restated", "reference"))
        untouched = [c for c in range(8) if c not in active]
        assert np.all(ref["eta"][:, untouched] == 0) and np.array_equal(ref["var_gamma"][:, untouched], st0["var_gamma"][:, untouched])
    assert got["q"].dtype == T
    P.assert_equal(got, ref, ld, H.STATE)


# ---- the inputs discriminate ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan_problem(T=np.float32):
    return syn.make_problem(sizes=PLAN, low_memory=False, seed=53, kind="longrange", float_precision=T)


def _assert_every_block_changes(run, inputs, names, ld):
    """Exchanging j <-> j ^ 1 inside each block in ONE input array changes the result in every block of >= 2 SNPs."""
    base = run(inputs)
    big = np.diff(ld.block_start) >= 2
    for name in names:
        swapped = dict(inputs)
        swapped[name] = P.swap_neighbours(inputs[name], ld.block_start)
        out = run(swapped)
        changed = np.zeros(len(big), dtype=bool)
        for k in base:
            changed |= P.blocks_changed(out[k], base[k], ld.block_start)
        assert np.array_equal(changed, big), (name, changed)


def _assert_exchange_is_invisible(inputs, names, ld):
    """... and in the inputs every other test uses the exchange is no change at all."""
    for name in names:
        assert np.array_equal(P.swap_neighbours(inputs[name], ld.block_start), inputs[name]), name


def test_exchanging_neighbours_changes_every_block_spike_slab():
    ld, ss, old = _plan_problem()
    names = ("mu_mult", "u_logs", "sqrt_half_var_tau")
    new = P.spike_slab(ss.std_beta)

    def run(inp):
        def go(arrays):
            import copy
            x = copy.copy(inp)
            for k, v in arrays.items():
                setattr(x, k, v)
            return H.run_oracle(ld, x, inp.state_copy(), sweeps=SWEEPS)
        return go
    _assert_every_block_changes(run(new), {k: getattr(new, k) for k in names}, names, ld)
    # the old inputs: the exchange leaves the arrays, and so the result, as they were (run once to say so in results)
    olds = {k: getattr(old, k) for k in names}
    _assert_exchange_is_invisible(olds, names, ld)
    same = run(old)({k: P.swap_neighbours(v, ld.block_start) for k, v in olds.items()})
    H.assert_state_equal(same, run(old)(olds))


def test_exchanging_neighbours_changes_every_block_mixture():
    ld, ss, inp = _plan_problem()
    names = ("log_null_pi", "u_logs", "shvt", "mu_mult")
    mix, st0 = P.mixture(ld.m, 4)
    _assert_every_block_changes(lambda a: _run_mix(O, ld, inp, a, st0, SWEEPS), mix, names, ld)
    _assert_exchange_is_invisible(_mixture_inputs(ld, ss, 4)[0], names, ld)
    m = syn.make_mixture_inputs(ss, 4)
    _assert_exchange_is_invisible(m, ("log_null_pi", "u_logs", "sqrt_half_var_tau", "mu_mult"), ld)


def test_exchanging_neighbours_changes_every_block_grid():
    ld, ss, inp = _plan_problem()
    names = ("u_logs", "hvt", "mu_mult")
    g, st0 = P.grid(ld.m, 5)
    active = np.array([4, 0, 2], dtype=np.int32)
    _assert_every_block_changes(lambda a: _run_grid(O, ld, inp, a, st0, active, sweeps=SWEEPS), g, names, ld)
    _assert_exchange_is_invisible(_grid_inputs(ld, ss, 5)[0], names, ld)
    _assert_exchange_is_invisible(syn.make_grid_inputs(ss, 8), ("u_logs", "half_var_tau", "mu_mult"), ld)


def test_exchanging_neighbours_changes_every_block_enet():
    from tests.test_gpu_enet import FIELDS, GRID, _replay, _start
    ld, ss, inp = _plan_problem()
    old_mult, old_pen, st0 = _start(ld.m, GRID)
    mult, pen = P.enet(ld.m, GRID)
    run = lambda a: {k: v for k, v in _replay(ld, inp.std_beta, a["mult"], a["pen"], st0, SWEEPS).items() if k in FIELDS}
    _assert_every_block_changes(run, dict(mult=mult, pen=pen), ("mult", "pen"), ld)
    _assert_exchange_is_invisible(dict(mult=old_mult, pen=old_pen), ("mult", "pen"), ld)


def test_exchanging_neighbours_changes_every_block_gibbs():
    from tests.test_gpu_gibbs import FIELDS, PAIRS, SEED, _replay, _start
    ld, ss, inp = _plan_problem()
    old, st0 = _start(ss.n_per_snp, PAIRS)
    new = P.gibbs(ld.m, PAIRS)
    # the draws of the unexchanged inputs for every run (the noise is scaled by half_var_tau: held fixed, the exchange of
    # half_var_tau is seen through the sweep alone)
    draws = [GB.gibbs_draws_host(SEED, i, new["half_var_tau"]) for i in range(SWEEPS)]
    names = ("mu_mult", "half_var_tau", "u_logs")
    _assert_every_block_changes(lambda a: _replay(ld, inp.std_beta, a, st0, draws), new, names, ld)
    _assert_exchange_is_invisible(old, names, ld)


# ---- conditions on the inputs ---------------------------------------------------------------------------------------------------
def _skip_shares(T):
    """Per sweep: the boolean vector of the SNPs that took the skip branch (eta_diff == 0)."""
    ld, ss, _ = _plan_problem(T)
    inp = P.spike_slab(ss.std_beta, T)
    st = inp.state_copy()
    out = []
    for _ in range(SWEEPS):
        st = H.run_oracle(ld, inp, st, sweeps=1)
        out.append(st["eta_diff"] == 0)
    return ld, out


def test_conditions_on_the_inputs():
    """What the recipe (and the seed, per_snp_inputs.SEED) has to give on PLAN for the GPU cases to reach what they name."""
    ld, ss, _ = _plan_problem()
    m = ld.m
    inp = P.spike_slab(ss.std_beta)
    for name in ("mu_mult", "u_logs", "sqrt_half_var_tau"):
        a = getattr(inp, name)
        assert a.dtype == np.float32
        distinct = np.unique(a).size
        print(f"{name}: {distinct} distinct float32 values over {m} SNPs")
        assert distinct >= 0.9 * m, (name, distinct)
        # no value twice inside one 64-row panel: a lane that read its neighbour's row reads another value
        for s, e in zip(ld.block_start[:-1], ld.block_start[1:]):
            for p in range(int(s), int(e), 64):
                rows = a[p:min(p + 64, int(e))]
                assert np.unique(rows).size == rows.size, (name, "repeats inside the panel at SNP", p)
    assert np.unique(inp.var_gamma).size >= 0.9 * m                    # the starting state varies too
    # float32: the skip branch takes 1 % .. 50 % of the SNPs in each sweep, and the blocks of 64 and of 130 SNPs hold both kinds
    ld, skipped = _skip_shares(np.float32)
    for i, sk in enumerate(skipped):
        print(f"float32 sweep {i + 1}: {sk.mean():.4f} of the SNPs skipped")
        assert 0.01 <= sk.mean() <= 0.50, (i, sk.mean())
        for bi in (B130, B64):
            blk = sk[int(ld.block_start[bi]):int(ld.block_start[bi + 1])]
            assert blk.size in (130, 64) and blk.any() and not blk.all(), (i, bi, int(blk.sum()))
    # float64 (|eta_diff| < 1e-8 is rarer): at least one SNP and not all
    _, skipped = _skip_shares(np.float64)
    for i, sk in enumerate(skipped):
        print(f"float64 sweep {i + 1}: {sk.mean():.4f} of the SNPs skipped")
        assert 0 < sk.sum() < m, (i, int(sk.sum()))


@pytest.mark.parametrize("K", [3, 4, 33])
def test_mixture_and_grid_inputs_vary_along_the_snps(K):
    m = sum(PLAN)
    mix, st = P.mixture(m, K)
    assert mix["u_logs"].shape == (m, K) and mix["u_logs"].flags.c_contiguous and st["var_gamma"].flags.c_contiguous
    assert float(np.exp(mix["log_null_pi"].astype(np.float64)).min()) > 0.96           # sum_k pis_jk < 0.04
    for a in (mix["log_null_pi"], mix["u_logs"][:, 0], mix["u_logs"][:, K - 1], mix["shvt"][:, K - 1], st["var_gamma"][:, K - 1]):
        assert np.unique(a).size >= 0.9 * m
    # mu_mult of the last component (d = 1: the spike-and-slab tau).  The components with a smaller tau lie ever closer to 1,
    # where float32 has few values; that their neighbours differ often enough is what the exchange tests above show.
    assert np.unique(mix["mu_mult"][:, K - 1]).size >= 0.9 * m
    g, st = P.grid(m, K)
    assert g["hvt"].shape == (m, K) and g["hvt"].flags.f_contiguous and st["var_gamma"].flags.f_contiguous
    for a in (g["u_logs"][:, 0], g["hvt"][:, K - 1], g["mu_mult"][:, K - 1], st["var_gamma"][:, 0]):
        assert np.unique(a).size >= 0.9 * m


def test_enet_and_gibbs_inputs_vary_along_the_snps():
    m = sum(PLAN)
    pairs = ((0.2, 0.005), (0.5, 0.002), (0.9, 0.005))
    mult, pen = P.enet(m, pairs)
    assert mult.shape == pen.shape == (m, 3) and mult.flags.f_contiguous and mult.dtype == np.float32
    for g, (s, lam) in enumerate(pairs):
        assert np.all((mult[:, g] >= np.float32(0.5 * (1 - s))) & (mult[:, g] <= np.float32(1 - s)))
        assert np.all((pen[:, g] >= np.float32(lam * 10 ** -0.5)) & (pen[:, g] <= np.float32(lam * 10 ** 0.5)))
        assert np.unique(mult[:, g]).size >= 0.9 * m and np.unique(pen[:, g]).size >= 0.9 * m
    one = P.enet(m, pairs[:1])
    assert one[0].shape == one[1].shape == (m,)
    gb = P.gibbs(m, ((0.5, 0.2), (0.01, 0.2)))
    for k in ("mu_mult", "half_var_tau", "u_logs"):
        assert gb[k].shape == (m, 2) and gb[k].flags.f_contiguous
        assert np.unique(gb[k][:, 1]).size >= 0.9 * m, k


def test_draws_are_reproducible_and_shared_between_the_models():
    a, b = P.Draws(500), P.Draws(500)
    assert np.array_equal(a.n, b.n) and np.array_equal(a.pi, b.pi) and np.array_equal(a.w, b.w)
    assert 1e4 <= a.n.min() and a.n.max() <= 1e5 * 10 ** 0.3 and 1e-3 <= a.pi.min() and a.pi.max() <= 0.1
    assert not np.array_equal(a.n, P.Draws(500, seed=P.SEED + 1).n)
    # every model sees the same n_j: the spike-and-slab mu_mult is the mixture's for a component with the same tau
    inp = P.spike_slab(np.zeros(500, np.float32))
    vt = a.n / P.SIGMA_EPS + inp.tau_beta
    assert np.array_equal(inp.mu_mult, (a.n / (vt * P.SIGMA_EPS)).astype(np.float32))
    assert np.array_equal(inp.var_gamma, a.pi.astype(np.float32))


# ---- first_difference ------------------------------------------------------------------------------------------------------------
def test_first_difference_names_the_block_the_panel_and_the_row():
    ld = syn.make_ld(PLAN, data=False)
    rng = np.random.default_rng(3)
    ref = dict(eta=rng.standard_normal(ld.m).astype(np.float32), q=rng.standard_normal((ld.m, 3)).astype(np.float32))
    got = {k: v.copy() for k, v in ref.items()}
    assert P.first_difference(got, ref, ld) is None
    P.assert_equal(got, ref, ld, ("eta", "q"))
    j = 2370 + 1601 + 70                                      # row 70 of the 130-SNP block: panel 1, row 6
    got["q"][j, 2] += 1
    got["q"][j + 9, 0] += 1
    got["eta"][j + 1] += 1
    msg = P.first_difference(got, ref, ld)
    for part in (f"q[{j}, 2]", "row 70 of block 2 (130 SNPs, starts at 3971)", "panel 1 of 3", "row 6 of the panel", "'q': 2",
                 "'eta': 1"):
        assert part in msg, (part, msg)
    with pytest.raises(AssertionError, match="row 70 of block 2"):
        P.assert_equal(got, ref, ld, ("eta", "q"))
    got["eta"][4165] = np.nan                                  # the single-row block; the earlier difference still wins
    assert f"q[{j}, 2]" in P.first_difference(got, ref, ld)
    assert f"eta[{j + 1}]" in P.first_difference(got, ref, ld, fields=("eta",))
    got["eta"][j + 1] = ref["eta"][j + 1]
    assert "eta[4165]" in P.first_difference(got, ref, ld, fields=("eta",))
    assert "row 0 of block 4 (1 SNPs" in P.first_difference(got, ref, ld, fields=("eta",))
