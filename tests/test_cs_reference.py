"""CPU: the host definition of PRS-CS (`viprs_amd.stats.cs`) -- the closed-form GIG(1/2) draw against its moments (and SciPy's
`geninvgauss` where SciPy imports), the Gamma(3/2) construction, the variate stream beside the Gibbs stream, the update's
contract, ``u_logs = 32`` in the C replay of the Gibbs sweep, the sums against `math.fsum`."""
import math

import numpy as np
import pytest

from tests import gibbs_replay as GR
from viprs_amd.stats import cs as CS
from viprs_amd.stats import gibbs as GB
from viprs_amd.utils import synthetic as syn

f32, f64 = np.float32, np.float64
N = 2 ** 20
GIG_CASES = [(2.0, 3.0), (0.5, 1e-8), (10.0, 0.0), (1e-3, 5.0), (4.0, 1e3)]


def _z(x, mean):
    return (x.mean() - mean) / (x.std() / math.sqrt(x.shape[0]))


@pytest.mark.parametrize("a, b", GIG_CASES)
def test_gig_half_moments(a, b):
    rng = np.random.default_rng(int(1000 * a) + 7)
    x = CS.gig_half_from_variates(a, b, rng.standard_normal(N), rng.random(N))
    assert x.dtype == f64 and np.all(np.isfinite(x)) and np.all(x > 0)
    z = _z(x, math.sqrt(b / a) + 1.0 / a)
    print(f"GIG(1/2, {a}, {b}): z-score of the mean {z:.2f}")
    assert abs(z) < 5
    if b > 0 and (a, b) != (0.5, 1e-8):                  # (1 / x of that case has a huge variance)
        zi = _z(1.0 / x, math.sqrt(a / b))
        print(f"   z-score of the mean of 1 / x {zi:.2f}")
        assert abs(zi) < 5


@pytest.mark.parametrize("a, b", [(2.0, 3.0), (1e-3, 5.0), (4.0, 1e3)])
def test_gig_half_against_scipy(a, b):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(3)
    x = CS.gig_half_from_variates(a, b, rng.standard_normal(20000), rng.random(20000))
    # geninvgauss(p, c, scale): density ~ y^(p-1) exp(-c (y + 1/y) / 2) of y = x / scale
    p = stats.kstest(x, stats.geninvgauss(0.5, math.sqrt(a * b), scale=math.sqrt(b / a)).cdf).pvalue
    assert p > 1e-3, p


def test_gig_half_is_elementwise_and_handles_beta_zero():
    z, u = np.array([0.3, -1.2, 2.0]), np.array([0.1, 0.5, 0.99])
    both = CS.gig_half_from_variates(np.array([1.0, 2.0, 3.0]), np.array([0.0, 1.0, 0.0]), z, u)
    assert both[0] == z[0] ** 2 / 1.0 and both[2] == z[2] ** 2 / 3.0
    assert both[1] == CS.gig_half_from_variates(2.0, 1.0, z[1], u[1])


def test_gamma_three_halves():
    rng = np.random.default_rng(5)
    g = 0.5 * rng.standard_normal(N) ** 2 - np.log(rng.random(N))
    assert abs(g.mean() - 1.5) < 5 * math.sqrt(1.5 / N)
    assert abs(g.var() - 1.5) < 5 * math.sqrt(13.5 / N)           # (fourth central moment of Gamma(3/2): 15.75)


def test_variate_stream_is_not_the_gibbs_stream():
    seed, di = 0x0123456789ABCDEF, 2 ** 40 + 5
    w = CS.cs_words_host(seed, di, 4, [0, 2])
    assert w.shape == (4, 2, 4) and w.dtype == np.uint32
    assert w[3, 1].tolist() == [0x32640B4A, 0x72A0B088, 0xB5179BB5, 0xBBC314DC]
    assert w[0, 0].tolist() == [0x69AFD173, 0x785CAF58, 0x599D66BE, 0x599A2F6B]
    # the counter is (j, g + 2^31, lo, hi), the key the halves of the seed
    direct = GB.philox4x32_10(np.array([3, 2 + 2 ** 31, 5, 256], dtype=np.uint64), np.array([0x89ABCDEF, 0x01234567], dtype=np.uint64))
    assert direct.tolist() == w[3, 1].tolist()
    g = GB.gibbs_words_host(seed, di, 4, [0, 2])
    assert not (g == w).all(axis=-1).any()
    ub, z1, z2, e = CS.cs_variates_host(seed, di, 4, [0, 2])
    assert all(v.dtype == f32 and v.shape == (4, 2) for v in (ub, z1, z2, e))
    assert ub[3, 1] == f32((2 * (0x32640B4A >> 9) + 1) * 2.0 ** -24) and np.all(e > 0)
    u = CS.cs_uniforms_host(seed, di, 4, [0, 2])
    assert np.allclose(z1 ** 2 + z2 ** 2, -2 * np.log(u[1].astype(f64)), rtol=1e-6) and np.array_equal(u[0], ub)
    # a variate depends on (seed, draw_index, j, g) alone
    assert np.array_equal(CS.cs_variates_host(seed, di, 3, [2])[1][:, 0], z1[:3, 1])


def _state(m, G, seed):
    rng = np.random.default_rng(seed)
    F = lambda a: np.asfortranarray(a.astype(f32))
    eta = 0.02 * rng.standard_normal((m, G))
    eta[rng.random((m, G)) < 0.2] = 0.0
    return dict(n=rng.uniform(2e4, 9e4, m), eta=F(eta), psi=F(rng.uniform(1e-3, 1, (m, G))), delta=F(rng.uniform(0.1, 5, (m, G))),
                mu_mult=F(rng.random((m, G))), half_var_tau=F(rng.uniform(1, 9, (m, G))), u_logs=F(rng.normal(size=(m, G))))


def _update(s, params, psi_max=1.0, variates=None, prepare_only=False):
    CS.cs_update_host(s["n"], s["eta"], s["psi"], s["delta"], s["mu_mult"], s["half_var_tau"], s["u_logs"], params, psi_max,
                      variates, prepare_only)


FIELDS = ("psi", "delta", "mu_mult", "half_var_tau", "u_logs")


def test_update_contract():
    m, G = 500, 3
    s = _state(m, G, 1)
    before = {k: s[k].copy() for k in FIELDS + ("eta",)}
    v = tuple(np.asfortranarray(np.repeat(a, 2, axis=1)[:, :G]) for a in CS.cs_variates_host(9, 4, m, [0, 1]))
    params = np.array([[2, 0.8, 0.3], [0, 1.7, 1e-3]])
    _update(s, params, variates=v)
    for k in FIELDS + ("eta",):                                     # the unlisted column keeps its bits
        assert np.array_equal(s[k][:, 1].view(np.uint32), before[k][:, 1].view(np.uint32)), k
    for g, sigma2, phi in params:
        g = int(g)
        assert np.all(s["psi"][:, g] >= f32(2.0 ** -40)) and np.all(s["psi"][:, g] <= 1) and (s["psi"][:, g] < 1).any()
        p = s["psi"][:, g].astype(f64)
        assert np.array_equal(s["mu_mult"][:, g], (p / (1 + p)).astype(f32)) and np.all(s["u_logs"][:, g] == 32)
        assert np.array_equal(s["half_var_tau"][:, g], (s["n"] * (1 + 1 / p) / (2 * sigma2)).astype(f32))
        z1, z2, e = (a[:, g].astype(f64) for a in v[1:])
        delta = (0.5 * z2 * z2 + e) / (before["psi"][:, g].astype(f64) + phi)
        assert np.array_equal(s["delta"][:, g], delta.astype(f32))
        zero = before["eta"][:, g] == 0                               # at eta = 0: z1^2 / (2 delta), clamped
        assert zero.sum() > 50
        want = np.minimum(np.maximum(z1 * z1 / (2 * delta), 2.0 ** -40), 1.0)
        assert np.array_equal(s["psi"][zero, g], want[zero].astype(f32))
        # elsewhere: the GIG draw of its own function
        x = CS.gig_half_from_variates(2 * delta, s["n"] * before["eta"][:, g].astype(f64) ** 2 / sigma2, z1, v[0][:, g])
        assert np.allclose(s["psi"][:, g], np.minimum(np.maximum(x, 2.0 ** -40), 1.0), rtol=1e-6)
    # a smaller cap
    t = _state(m, G, 1)
    _update(t, params, psi_max=0.25, variates=v)
    assert t["psi"][:, [0, 2]].max() == f32(0.25) and np.array_equal(t["delta"], s["delta"])


def test_prepare_only_changes_nothing_but_the_three_fields():
    s = _state(300, 2, 2)
    before = {k: s[k].copy() for k in FIELDS}
    _update(s, np.array([[1, 2.0, 0.5]]), prepare_only=True)
    assert np.array_equal(s["psi"], before["psi"]) and np.array_equal(s["delta"], before["delta"])
    for k in ("mu_mult", "half_var_tau", "u_logs"):
        assert np.array_equal(s[k][:, 0], before[k][:, 0]) and not np.array_equal(s[k][:, 1], before[k][:, 1])
    p = s["psi"][:, 1].astype(f64)
    assert np.array_equal(s["half_var_tau"][:, 1], (s["n"] * (1 + 1 / p) / 4.0).astype(f32))


def test_update_refuses_bad_arguments():
    s = _state(10, 2, 3)
    for params, kw in (([[2, 1, 1]], {}), ([[0, 1, 1], [0, 1, 1]], {}), ([[0, 0.0, 1]], {}), ([[0, 1, -1.0]], {}),
                       ([[0, np.nan, 1]], {}), ([[0, 1, np.inf]], {}), ([[0, 1, 1]], dict(psi_max=2.0 ** -40)),
                       ([[0, 1, 1]], dict(psi_max=np.inf)), ([[0.5, 1, 1]], {})):
        with pytest.raises(ValueError):
            _update(s, np.array(params, dtype=f64), prepare_only=True, **kw)


def test_u_logs_32_includes_every_snp_in_the_c_replay():
    """The inputs `cs_update_host` writes, swept by tests/gibbs_replay.c: gamma is exactly 1 and every effect is drawn."""
    ld, ss, _ = syn.make_problem(sizes=[130, 64, 1], low_memory=False, seed=53, kind="longrange")
    m = ld.m
    s = _state(m, 1, 4)
    s["n"] = np.asarray(ss.n_per_snp, dtype=f64)
    _update(s, np.array([[0, 0.9, 0.01]]), variates=tuple(np.asfortranarray(a) for a in CS.cs_variates_host(1, 0, m, [0])))
    unif, noise = GB.gibbs_draws_host(1, 0, s["half_var_tau"])
    unif[::7, 0] = np.nextafter(f32(1), f32(0))                      # the largest uniform there is
    eta, q = np.zeros((m, 1), dtype=f32, order="F"), np.zeros((m, 1), dtype=f32, order="F")
    _, mu, gam = GR.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False, ss.std_beta, s["mu_mult"], s["half_var_tau"],
                                 s["u_logs"], unif, noise, eta, q, ld.dq_scale)
    assert np.all(gam == 1) and np.all(eta != 0) and np.array_equal(eta, mu + noise)
    assert GB.sigmoid32(f32(32.0)) == 1 and GB.sigmoid32(np.nextafter(f32(16.0), f32(0))) < 1


@pytest.mark.parametrize("m", [1, 700, 70001])
def test_sums_against_fsum(m):
    s = _state(m, 2, 6)
    got = CS.cs_sums_host(s["n"], s["eta"], s["psi"], s["delta"], [1, 0])
    assert got.shape == (2, 4)
    nb = min(-(-m // 256), 256)
    D = -(-m // (nb * 256)) + 8 + -(-nb // 64) + 6
    for i, g in enumerate((1, 0)):
        e, p, d = (s[k][:, g].astype(f64) for k in ("eta", "psi", "delta"))
        t = e * e / p
        for k, (terms, C) in enumerate(((t, 2), (s["n"] * t, 3), (d, 0), (p, 0))):
            exact = math.fsum(terms)
            assert abs(got[i, k] - exact) <= 2.0 ** -52 * (D + C) * math.fsum(np.abs(terms)), (g, k)
    assert np.array_equal(CS.cs_sums_host(s["n"], s["eta"], s["psi"], s["delta"])[::-1], got)


def test_scalar_draws():
    rng = np.random.default_rng(1)
    s2 = np.array([CS.cs_sigma2_draw(rng, 5e4, 1000, 0.1, 0.12, 30.0) for _ in range(4000)])
    err = 0.5 * 5e4 * (1 - 0.2 + 0.12)
    assert abs(s2.mean() - err / (0.5 * 51000 - 1)) < 5 * s2.std() / math.sqrt(4000)
    # the floor: err is at least half the weighted quadratic form
    s2 = np.array([CS.cs_sigma2_draw(rng, 5e4, 1000, 0.6, 0.1, 3e4) for _ in range(4000)])
    assert abs(s2.mean() - 1.5e4 / (0.5 * 51000 - 1)) < 5 * s2.std() / math.sqrt(4000)
    a, b = np.random.default_rng(2), np.random.default_rng(2)
    phi = CS.cs_phi_draw(a, 1000, 0.5, 0.3, 40.0)
    w = b.gamma(1.0, 1.0 / 1.3)
    assert phi == b.gamma(500.5, 1.0 / (40.0 + w))
