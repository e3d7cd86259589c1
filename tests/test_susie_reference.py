"""SuSiE on the host (viprs_amd/stats/susie.py) and the replay of the device's step (tests/susie_replay.py): `susie_host`
against a dense textbook IBSS written here, the monotone ELBO, recovery of planted effects with their credible sets, the edge
cases of the definition, and how far the replay (the device's arithmetic) is from `susie_host`."""
import functools
import math

import numpy as np
import pytest

from tests import susie_replay as SR
from viprs_amd.plan import SusieInfo
from viprs_amd.stats import susie as S

SIZES, RHOS = (65, 200, 300), (0.5, 0.9, 0.97)
PLANTED = (8.0, -7.0, 6.0)


def ar1_blocks(sizes=SIZES, rhos=RHOS, low_memory=False, dtype=np.float32):
    """Dense AR(1) blocks rho^|i-j| as the arrays of an `LDPlan`: (left_bound, indptr, data)."""
    lb, length, rows = [], [], []
    start = 0
    for n, rho in zip(sizes, rhos):
        for j in range(n):
            lo, hi = (j + 1, n) if low_memory else (0, n)
            lb.append(start + min(lo, n - 1))
            length.append(max(hi - lo, 0))
            rows.append(np.power(rho, np.abs(np.arange(lo, hi) - j)))
        start += n
    ip = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    return np.array(lb, dtype=np.int32), ip, np.concatenate(rows).astype(dtype)


def planted_at(n):
    return (n // 6, n // 2, (5 * n) // 6)


@functools.lru_cache(maxsize=None)
def problem(low_memory=False):
    """The three AR(1) blocks and z = R b with three planted effects per block."""
    lb, ip, data = ar1_blocks(low_memory=low_memory)
    z, start = [], 0
    for n in SIZES:
        R = S.block_matrix(lb, ip, data, low_memory, start, start + n)
        b = np.zeros(n)
        b[list(planted_at(n))] = PLANTED
        z.append(R @ b)
        start += n
    return lb, ip, data, np.concatenate(z)


def textbook_ibss(R, z, L, V0, estimate, tol, max_iter, log_pi=None):
    """Dense IBSS with plain loops: the single-effect regression of SuSiE-RSS with residual variance 1, the full log Bayes
    factor log N(r; 0, 1 + V) - log N(r; 0, 1), the EM update of V."""
    n = len(z)
    log_pi = [-math.log(n)] * n if log_pi is None else list(log_pi)
    alpha = [[0.0] * n for _ in range(L)]
    mu = [[0.0] * n for _ in range(L)]
    V = [float(V0)] * L
    Rb = [[0.0] * n for _ in range(L)]
    for it in range(1, max_iter + 1):
        delta = 0.0
        for l in range(L):
            r = [z[j] - sum(Rb[k][j] for k in range(L) if k != l) for j in range(n)]
            lbf = [-0.5 * math.log(1.0 + V[l]) + 0.5 * r[j] ** 2 * V[l] / (1.0 + V[l]) + log_pi[j] for j in range(n)]
            top = max(lbf)
            wts = [math.exp(v - top) for v in lbf]
            tot = sum(wts)
            new = [v / tot for v in wts]
            delta = max(delta, max(abs(new[j] - alpha[l][j]) for j in range(n)))
            alpha[l] = new
            s = V[l] / (1.0 + V[l])
            mu[l] = [s * r[j] for j in range(n)]
            if estimate:
                V[l] = sum(new[j] * (s + mu[l][j] ** 2) for j in range(n))
            bbar = np.array([new[j] * mu[l][j] for j in range(n)])
            Rb[l] = list(R @ bbar)
        if delta < tol:
            return np.array(alpha).T, np.array(mu).T, np.array(V), it, True
    return np.array(alpha).T, np.array(mu).T, np.array(V), max_iter, False


@pytest.mark.parametrize("estimate", [True, False], ids=["em", "fixed"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_host_fit_is_the_textbook_ibss(low_memory, estimate):
    lb, ip, data, z = problem(low_memory)
    info = S.susie_host(lb, ip, data, low_memory, z, L=3, prior_variance=50.0, estimate_prior_variance=estimate,
                        tol=1e-4, max_iter=30)
    assert info.alpha.flags.f_contiguous and info.alpha.dtype == np.float64
    for k in range(3):
        s, e = int(info.block_start[k]), int(info.block_start[k + 1])
        R = S.block_matrix(lb, ip, data, low_memory, s, e)
        a, m, V, it, ok = textbook_ibss(R, z[s:e], 3, 50.0, estimate, 1e-4, 30)
        assert it == info.iterations[k] and ok == (info.status[k] == 0)
        assert np.max(np.abs(a - info.alpha[s:e])) < 1e-10 and np.max(np.abs(m - info.mu[s:e])) < 1e-9
        assert np.max(np.abs(V - info.prior_variance[k])) < 1e-9 * 50.0


@pytest.mark.parametrize("L", [1, 3, 10])
@pytest.mark.parametrize("estimate", [True, False], ids=["em", "fixed"])
def test_elbo_never_decreases(estimate, L):
    """From iteration to iteration, on every one of the three blocks, with a slack of 1e-9 |ELBO|."""
    lb, ip, data, z = problem()
    starts = np.concatenate([[0], np.cumsum(SIZES)])
    Rs = [S.block_matrix(lb, ip, data, False, int(s), int(e)) for s, e in zip(starts[:-1], starts[1:])]
    trace = {k: [] for k in range(3)}

    def record(k, it, st):
        s, e = int(starts[k]), int(starts[k + 1])
        lp = np.full(e - s, -np.log(float(e - s)))
        trace[k].append(S.elbo_block(Rs[k], z[s:e], lp, st["alpha"], st["mu"], st["prior_variance"], st["post_var"]))

    info = S.susie_host(lb, ip, data, False, z, L=L, estimate_prior_variance=estimate, tol=1e-4, max_iter=100,
                        callback=record)
    print("iterations", info.iterations.tolist())
    assert info.converged
    final = S.susie_elbo(lb, ip, data, False, z, info)
    for k in range(3):
        e = np.array(trace[k])
        assert len(e) == info.iterations[k] and e[-1] == final[k]
        assert np.all(np.diff(e) >= -1e-9 * np.abs(e[1:])), (k, np.diff(e).min())


def test_planted_effects_are_recovered_with_pure_credible_sets():
    lb, ip, data = ar1_blocks((65,), (0.5,))
    R = S.block_matrix(lb, ip, data, False, 0, 65)
    b = np.zeros(65)
    b[list(planted_at(65))] = PLANTED
    z = R @ b
    info = S.susie_host(lb, ip, data, False, z, L=5)
    pip = S.pips(info)
    assert np.all(pip[list(planted_at(65))] > 0.99)
    sets = S.credible_sets(info, lb, ip, data, False)
    assert sorted(int(cs["snps"][0]) for cs in sets) == sorted(planted_at(65))
    assert all(len(cs["snps"]) == 1 and cs["purity"] == 1.0 and cs["coverage"] >= 0.95 for cs in sets)
    # without the purity filter the two idle effects show: diffuse sets over most of the block
    loose = S.credible_sets(info, lb, ip, data, False, min_abs_corr=0.0)
    assert len(loose) > 3 and max(len(cs["snps"]) for cs in loose) > 30


def test_credible_sets_ties_subsampling_and_windows():
    lb, ip, data = ar1_blocks((8,), (0.9,), low_memory=True)
    alpha = np.zeros((8, 2), order="F")
    alpha[:, 0] = [0.0, 0.25, 0.25, 0.25, 0.125, 0.125, 0.0, 0.0]   # ties go to the lower index
    alpha[:, 1] = alpha[:, 0]                                   # a repeated set is dropped
    info = SusieInfo(alpha, np.zeros_like(alpha), [[1.0, 1.0]], [[0.5, 0.5]], [1], [0.0], [0], [0, 8])
    sets = S.credible_sets(info, lb, ip, data, True, coverage=0.75)
    assert len(sets) == 1 and sets[0]["snps"].tolist() == [1, 2, 3] and sets[0]["effect"] == 0
    assert sets[0]["purity"] == pytest.approx(0.81, rel=1e-6) and sets[0]["coverage"] == 0.75
    assert S.credible_sets(info, lb, ip, data, True, coverage=0.8)[0]["snps"].tolist() == [1, 2, 3, 4]
    assert S.credible_sets(info, lb, ip, data, True, coverage=0.8, min_abs_corr=0.75) == []
    # a set larger than n_purity is judged on a seeded subsample
    a, b = (S.credible_sets(info, lb, ip, data, True, coverage=0.8, min_abs_corr=0.0, n_purity=2, seed=sd)[0] for sd in (0, 0))
    assert a["purity"] == b["purity"] and a["purity"] >= 0.9 ** 3 - 1e-6
    # an entry outside a window counts as 0: the same block with a window of 1
    j = np.arange(8)
    length = np.minimum(1, 7 - j)
    ipw = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    lbw = np.minimum(j + 1, 7).astype(np.int32)
    dw = np.full(int(ipw[-1]), 0.9, dtype=np.float32)
    E = S.ld_entries(lbw, ipw, dw, True, [1, 2, 3])
    assert E[0, 2] == 0.0 and E[0, 1] == E[1, 0] == np.float32(0.9) and E[1, 1] == 1.0
    assert S.credible_sets(info, lbw, ipw, dw, True, coverage=0.75) == []
    off = SusieInfo(alpha, np.zeros_like(alpha), [[1e-10, 0.0]], [[0.5, 0.5]], [1], [0.0], [0], [0, 8])
    assert S.credible_sets(off, lb, ip, data, True) == [] and np.all(S.pips(off) == 0.0)


@pytest.mark.parametrize("fit", [S.susie_host, SR.susie_replay], ids=["host", "replay"])
def test_edge_cases_of_the_definition(fit):
    lb, ip, data = ar1_blocks((65, 1, 7), (0.5, 0.5, 0.9))
    z = np.zeros(73)
    z[65] = 5.0
    lp = np.concatenate([np.full(65, -np.log(65.0)), [0.0], np.full(7, -np.log(6.0))])
    lp[66 + 3] = -np.inf                                        # an excluded SNP
    z[66 + 3] = 9.0
    V0 = np.full((3, 2), 50.0)
    V0[2, 1] = 0.0                                              # an effect that is switched off
    info = fit(lb, ip, data, False, z, 2, V0, False, lp, 1.0, 1e-4, 50, "float64")
    # z = 0: alpha = pi, mu = 0, converged at the second iteration (the first moves alpha from 0 to pi)
    assert np.allclose(info.alpha[:65], 1.0 / 65, rtol=1e-14, atol=0) and np.all(info.mu[:65] == 0.0)
    assert info.status[0] == 0 and info.iterations[0] == 2
    # one SNP: alpha = 1 in every effect, the effects share z
    assert np.all(info.alpha[65] == 1.0) and info.status[1] == 0 and info.iterations[1] == 2
    s = 50.0 / 51.0
    m0 = s * 5.0
    m1 = s * (5.0 - m0)
    m0 = s * (5.0 - m1)
    assert info.mu[65].tolist() == pytest.approx([m0, s * (5.0 - m0)], rel=1e-14)
    # the excluded SNP and the V = 0 effect
    assert np.all(info.alpha[69] == 0.0)
    assert np.allclose(info.alpha[66:73, 1], np.exp(lp[66:73]), rtol=1e-14, atol=0) and np.all(info.mu[66:73, 1] == 0.0)
    assert info.post_var[2, 1] == 0.0 and info.prior_variance[2, 1] == 0.0
    assert np.isfinite(S.susie_elbo(lb, ip, data, False, z, info, lp)).all()
    assert S.pips(info)[69] == 0.0


def test_refusals_of_the_host_fit():
    lb, ip, data, z = problem()
    bad = z.copy()
    bad[3] = np.nan
    lp = np.zeros(565)
    lp[:65] = -np.inf
    for kw, word in ((dict(L=0), "L must"), (dict(L=33), "L must"), (dict(tol=0.0), "tol"), (dict(max_iter=0), "max_iter"),
                     (dict(dq_scale=np.inf), "dq_scale"), (dict(prior_variance=-1.0), "prior variance"),
                     (dict(prior_variance=np.full((3, 10), np.nan)), "prior variance"), (dict(z=bad), "z must"),
                     (dict(log_prior=lp), "every SNP"), (dict(log_prior=np.full(565, np.inf)), "log_prior"),
                     (dict(prior_variance=np.ones((2, 10))), "shape"), (dict(z=z[:-1]), "shape")):
        args = dict(z=z)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            S.susie_host(lb, ip, data, False, **args)


# max |PIP difference| and max |bbar difference| between the replay and `susie_host` over the six cases below, measured
# (the maxima over L in {1, 3, 10} and both prior-variance modes):
#   float64 state   PIP 1.0e-15   bbar 7.2e-15    (9.99e-16 and 7.11e-15 before rounding up)
#   float32 state   PIP 6.0e-8    bbar 8.0e-7     (5.96e-8 and 7.94e-7)
# The assertions are 10 x these: the margin covers other inputs of the same size class.
MEASURED = {"float64": (1.0e-15, 7.2e-15), "float32": (6.0e-8, 8.0e-7)}


@pytest.mark.parametrize("T", ["float64", "float32"])
def test_replay_against_the_host_fit(T):
    """The replay is the device's arithmetic (ordered sums, libm exp, the product in T); `susie_host` is NumPy float64.
    Measured maxima over the six cases: float64 state max |dPIP| 9.99e-16, max |dbbar| 7.11e-15; float32 state 5.96e-8 and
    7.94e-7 (`MEASURED` holds them rounded up).  The float64 figures are rounding noise, far below 1e-6."""
    lb, ip, data, z = problem()
    worst_pip = worst_bbar = 0.0
    for L in (1, 3, 10):
        for estimate in (True, False):
            host = S.susie_host(lb, ip, data, False, z, L, 50.0, estimate, None, 1.0, 1e-4, 100, T)
            rep = SR.susie_replay(lb, ip, data, False, z, L, 50.0, estimate, None, 1.0, 1e-4, 100, T)
            assert rep.alpha.dtype == np.dtype(T) and np.array_equal(rep.status, host.status)
            bb = lambda i: np.sum(i.alpha.astype(np.float64) * i.mu.astype(np.float64), axis=1)
            d_pip = float(np.max(np.abs(S.pips(rep) - S.pips(host))))
            d_bbar = float(np.max(np.abs(bb(rep) - bb(host))))
            print(T, "L", L, "em" if estimate else "fixed", "iterations", rep.iterations.tolist(), host.iterations.tolist(),
                  "max |dPIP|", d_pip, "max |dbbar|", d_bbar)
            worst_pip, worst_bbar = max(worst_pip, d_pip), max(worst_bbar, d_bbar)
    print(T, "worst", worst_pip, worst_bbar)
    assert worst_pip <= 10 * MEASURED[T][0] and worst_bbar <= 10 * MEASURED[T][1]
