"""CPU: the host definition of PRS-CSx (`viprs_amd.stats.csx`): the rejection sampler against the moments of the GIG density
(quadrature on a log grid, and the closed-form inverse Gaussian for p = -1/2), the coupled update with one population
against `cs_update_host`, two populations (closed-form rows, the floor, NaN, unlisted columns), and the sums."""
import numpy as np
import pytest

from viprs_amd.stats import cs as CS
from viprs_amd.stats import csx as CX
from viprs_amd.stats.gibbs import _open_unit

f32 = np.float32
N_DRAWS = 2 ** 18


def _rng_uniforms(seed):
    rng = np.random.default_rng(seed)
    return lambda attempt, idx: tuple(_open_unit(rng.integers(0, 2 ** 32, idx.shape[0], dtype=np.uint32)) for _ in range(3))


@pytest.mark.parametrize("p", [0.0, -0.5, -1.0, -1.5])
@pytest.mark.parametrize("omega", [0.01, 1.0, 100.0])
def test_gig_host_has_the_moments_of_the_density(p, omega):
    """2^18 draws: the sample means of X and of 1 / X lie within 5 standard errors of the moments of the density, integrated
    numerically on a log grid (the variance of each mean from the same quadrature)."""
    a, b = 2.0 * omega, 0.5 * omega                                  # sqrt(a b) = omega, scale sqrt(b / a) = 1 / 2
    x, attempts, capped = CX.gig_host(np.full(N_DRAWS, p), a, b, _rng_uniforms(int(1000 * omega) + int(-10 * p)))
    assert not capped.any() and attempts.min() >= 1 and attempts.max() < CX.MAX_ATTEMPTS and np.all(x > 0)
    m1, v1, i1, iv = CX.gig_moments(p, a, b)
    z_x, z_inv = (x.mean() - m1) / np.sqrt(v1 / N_DRAWS), ((1.0 / x).mean() - i1) / np.sqrt(iv / N_DRAWS)
    print(f"p = {p}, omega = {omega}: E X {x.mean():.6g} vs {m1:.6g} ({z_x:+.2f} se), E 1/X {(1 / x).mean():.6g} vs {i1:.6g} "
          f"({z_inv:+.2f} se), mean attempts {attempts.mean():.3f}, longest {attempts.max()}")
    assert abs(z_x) < 5 and abs(z_inv) < 5
    if p == -0.5:                                                    # inverse Gaussian(mu = sqrt(b / a), shape b)
        mu = np.sqrt(b / a)
        assert np.isclose(m1, mu, rtol=1e-9) and np.isclose(v1, mu ** 3 / b, rtol=1e-7)
        assert np.isclose(i1, 1.0 / mu + 1.0 / b, rtol=1e-9)
        assert abs(x.mean() - mu) < 5 * np.sqrt(mu ** 3 / b / N_DRAWS)
        assert abs((1.0 / x).mean() - (1.0 / mu + 1.0 / b)) < 5 * np.sqrt((1.0 / (mu * b) + 2.0 / b ** 2) / N_DRAWS)


def test_gig_host_takes_given_uniforms_and_stops_at_the_cap():
    rng = np.random.default_rng(5)
    un = rng.random((CX.MAX_ATTEMPTS, 3, 64))
    x, attempts, capped = CX.gig_host(np.zeros(64), np.full(64, 2.0), np.full(64, 0.5), un)
    again = CX.gig_host(0.0, 2.0, 0.5, un[:, :, 7])
    assert float(again[0]) == x[7] and int(again[1]) == attempts[7] and not capped.any()
    # W = 1 against a proposal in a tail of the envelope is never accepted: the last proposal stands, the cap is reported
    never = np.stack([np.full((CX.MAX_ATTEMPTS, 4), 0.999), np.full((CX.MAX_ATTEMPTS, 4), 0.5),
                      np.ones((CX.MAX_ATTEMPTS, 4))], axis=1)
    x, attempts, capped = CX.gig_host(np.zeros(4), 2.0, 0.5, never)
    assert capped.all() and np.all(attempts == CX.MAX_ATTEMPTS) and np.all(np.isfinite(x))
    x, attempts, capped = CX.gig_host(np.zeros(2), np.array([np.nan, 2.0]), 0.5, un[:, :, :2])
    assert np.isnan(x[0]) and capped[0] and attempts[0] == CX.MAX_ATTEMPTS and np.isfinite(x[1]) and not capped[1]


def _state(rng, m, G):
    eta = (0.02 * rng.standard_normal((m, G))).astype(f32, order="F")
    eta[rng.random((m, G)) < 0.1] = 0
    n = rng.uniform(2e4, 6e4, m)
    fields = [np.asfortranarray(rng.random((m, G)).astype(f32)) for _ in range(5)]
    return eta, n, fields


def test_one_population_is_cs_update_host():
    rng = np.random.default_rng(11)
    m, G = 700, 3
    eta, n, fields = _state(rng, m, G)
    psi0 = np.asfortranarray(rng.uniform(0.01, 1.0, (m, G)).astype(f32))
    delta0 = np.asfortranarray(rng.random((m, G)).astype(f32))
    variates = [np.asfortranarray(v) for v in CS.cs_variates_host(3, 9, m, np.arange(G))]
    params = np.array([[2, 0.7, 0.03], [0, 1.3, 2.0]])               # (column, sigma2, phi), column 1 not listed
    want = [psi0.copy(order="F"), delta0.copy(order="F")] + [f.copy(order="F") for f in fields[2:]]
    CS.cs_update_host(n, eta, want[0], want[1], want[2], want[3], want[4], params, 0.8, variates)
    psi, delta = psi0.copy(order="F"), delta0.copy(order="F")
    mine = [f.copy(order="F") for f in fields]
    attempts, capped = CX.csx_update_host(np.arange(m)[None, :], [n], [eta], psi, delta, [tuple(mine)], params[:, [0, 2, 1]],
                                          0.8, variates, seed=3, draw_index=9)
    assert capped == 0 and not attempts.any()
    for got, ref in zip((psi, delta, mine[2], mine[3], mine[4]), want):
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(mine[0][:, [0, 2]], psi[:, [0, 2]]) and np.array_equal(mine[1][:, [0, 2]], delta[:, [0, 2]])
    assert np.array_equal(mine[1][:, 1], fields[1][:, 1]) and np.array_equal(psi[:, 1], psi0[:, 1])   # not listed: untouched
    # drawn from (seed, draw_index) when no variates are given: the same bits
    psi2, delta2 = psi0.copy(order="F"), delta0.copy(order="F")
    CX.csx_update_host(np.arange(m)[None, :], [n], [eta], psi2, delta2, [tuple(f.copy(order="F") for f in fields)],
                       params[:, [0, 2, 1]], 0.8, None, seed=3, draw_index=9)
    assert np.array_equal(psi2[:, [0, 2]], psi[:, [0, 2]]) and np.array_equal(delta2[:, [0, 2]], delta[:, [0, 2]])
    # prepare only: the fields from the stored psi, nothing drawn
    prep = [f.copy(order="F") for f in fields]
    ref = [f.copy(order="F") for f in fields[2:]]
    CX.csx_update_host(np.arange(m)[None, :], [n], [eta], psi, delta, [tuple(prep)], params[:, [0, 2, 1]], 0.8,
                       prepare_only=True)
    CS.cs_update_host(n, eta, psi.copy(order="F"), delta, ref[0], ref[1], ref[2], params, 0.8, prepare_only=True)
    assert all(np.array_equal(a, b) for a, b in zip(prep[2:], ref))


def test_two_populations_rows_floor_nan_and_the_sums():
    rng = np.random.default_rng(12)
    m0, m1, G = 300, 260, 2
    # union: 200 shared, 100 only in population 0, 60 only in population 1 (population 1 in another order)
    perm = rng.permutation(m1)
    row_of = np.full((2, 360), -1, dtype=np.int64)
    row_of[0, :300] = np.arange(300)
    row_of[1, 100:300] = perm[:200]
    row_of[1, 300:] = perm[200:]
    (eta0, n0, f0), (eta1, n1, f1) = _state(rng, m0, G), _state(rng, m1, G)
    eta0[150, 0] = eta1[row_of[1, 150], 0] = 0.0                      # B == 0 with two carrying populations
    eta0[151, 0] = np.nan
    psi = np.asfortranarray(rng.uniform(0.01, 1.0, (360, G)).astype(f32))
    delta = np.zeros((360, G), dtype=f32, order="F")
    keep = [a.copy() for a in (psi, *f0, *f1)]
    params = np.array([[0, 0.5, 0.9, 1.1]])
    attempts, capped = CX.csx_update_host(row_of, [n0, n1], [eta0, eta1], psi, delta, [tuple(f0), tuple(f1)], params, 1.0,
                                          seed=4, draw_index=2)
    both = np.arange(100, 300)
    assert capped == 1 and attempts[151, 0] == CX.MAX_ATTEMPTS and np.isnan(psi[151, 0])   # a NaN ends at the cap, stays NaN
    assert psi[150, 0] == f32(2.0 ** -40) and attempts[150, 0] == 0
    ok = np.setdiff1d(both, [150, 151])
    assert np.all(attempts[ok, 0] >= 1) and attempts[ok, 0].max() < 12 and not attempts[:100].any() and not attempts[300:].any()
    assert np.all((psi[ok, 0] >= f32(2.0 ** -40)) & (psi[ok, 0] <= 1))
    # rows carried by one population: the closed form of that population alone
    variates = [np.asfortranarray(np.repeat(v, G, axis=1)) for v in CS.cs_variates_host(4, 2, 360, [0])]
    for k, (eta, n, rows) in enumerate(((eta0, n0, np.arange(100)), (eta1, n1, np.arange(300, 360)))):
        sub = [keep[0][rows].copy(order="F"), np.zeros((rows.shape[0], G), dtype=f32, order="F")] + \
              [np.zeros((rows.shape[0], G), dtype=f32, order="F") for _ in range(3)]
        r = row_of[k, rows]
        CS.cs_update_host(n[r], np.asfortranarray(eta[r]), *sub, np.array([[0, params[0, 2 + k], 0.5]]), 1.0,
                          [np.asfortranarray(v[rows]) for v in variates])
        assert np.array_equal(psi[rows, 0], sub[0][:, 0]) and np.array_equal(delta[rows, 0], sub[1][:, 0])
        assert np.array_equal((f0, f1)[k][3][r, 0], sub[3][:, 0])
    # the scatter: every population holds the shared psi and delta at its rows and the fields of the existing formulas
    for k, (f, n, s2) in enumerate(((f0, n0, 0.9), (f1, n1, 1.1))):
        u = np.flatnonzero(row_of[k] >= 0)
        u = u[u != 151]
        r = row_of[k, u]
        p = psi[u, 0].astype(np.float64)
        assert np.array_equal(f[0][r, 0], psi[u, 0]) and np.array_equal(f[1][r, 0], delta[u, 0])
        assert np.array_equal(f[2][r, 0], (p / (1.0 + p)).astype(f32))
        assert np.array_equal(f[3][r, 0], (n[r] * (1.0 + 1.0 / p) / (2.0 * s2)).astype(f32)) and np.all(f[4][r, 0] == 32)
    # the column that is not listed keeps its bits everywhere
    assert np.array_equal(psi[:, 1], keep[0][:, 1]) and not delta[:, 1].any()
    for now, then in zip((*f0, *f1), keep[1:]):
        assert np.array_equal(now[:, 1], then[:, 1])
    # the same call again: the same bits
    psi2 = keep[0].copy(order="F")
    d2 = np.zeros_like(delta)
    CX.csx_update_host(row_of, [n0, n1], [eta0, eta1], psi2, d2, [tuple(a.copy() for a in f0), tuple(a.copy() for a in f1)],
                       params, 1.0, seed=4, draw_index=2)
    assert np.array_equal(psi2.view(np.uint32), psi.view(np.uint32)) and np.array_equal(d2, delta)
    s = CX.csx_sums_host(np.nan_to_num(psi), delta)
    assert s.shape == (2, 2) and np.isclose(s[0, 0], delta[:, 0].astype(np.float64).sum(), rtol=1e-12)
    assert np.isclose(s[1, 1], psi[:, 1].astype(np.float64).sum(), rtol=1e-12)
    assert np.array_equal(CX.csx_sums_host(np.nan_to_num(psi), delta, cols=[1]), s[1:])


def test_attempt_uniforms_are_a_stream_of_their_own():
    """The counter of attempt a differs from the variates' (a + 1 = 0) and from every other attempt's in bits 16..21."""
    u = np.arange(50)
    first = CX.csx_attempt_uniforms(7, 3, u, 2, 0)
    assert all(v.dtype == f32 and np.all((v > 0) & (v < 1)) for v in first)
    ub = CS.cs_uniforms_host(7, 3, 50, [2])[0][:, 0]
    assert not np.array_equal(first[0], ub)
    assert not np.array_equal(first[0], CX.csx_attempt_uniforms(7, 3, u, 2, 1)[0])
    assert np.array_equal(first[1], CX.csx_attempt_uniforms(7, 3, u, 2, 0)[1])
    with pytest.raises(ValueError):
        CX.csx_update_host(np.zeros((9, 1), dtype=np.int64), [], [], None, None, [], np.zeros((1, 11)))
