"""CPU: the host definition of the LDpred2 Gibbs draws and sweep (viprs_amd/stats/gibbs.py) -- Philox4x32-10 against the
published known answers, the uniforms and the moments of the draws, `gibbs_sweep_host` `==` the C replay
(tests/gibbs_replay.c), the inclusion frequencies of the sampler on an identity LD block."""
import numpy as np
import pytest

from tests import gibbs_replay as GR
from viprs_amd.stats import gibbs as GB
from viprs_amd.utils import synthetic as syn


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10.  The implementation here was written from the published round function
    (Salmon et al. 2011, section 3.3) and reproduces both quoted vectors; a second transcription of the rounds -- the scalar
    loop below, Python integers only -- agrees with it on random counters and keys."""
    z = GB.philox4x32_10(np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32))
    assert [int(x) for x in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    o = GB.philox4x32_10(np.full(4, 0xFFFFFFFF, dtype=np.uint32), np.full(2, 0xFFFFFFFF, dtype=np.uint32))
    assert [int(x) for x in o] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]

    def scalar(c, k):
        c, k = list(c), list(k)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        return c
    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 2 ** 32, size=(50, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(50, 2), dtype=np.uint64)
    got = GB.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (50, 4)
    for i in range(50):
        assert [int(x) for x in got[i]] == scalar([int(x) for x in ctr[i]], [int(x) for x in key[i]])


def test_counter_and_key_layout():
    """key = the halves of the seed, counter = (j, g, the halves of draw_index)."""
    seed, idx = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    w = GB.gibbs_words_host(seed, idx, 5, [0, 7])
    for j in (0, 4):
        for i, g in enumerate((0, 7)):
            want = GB.philox4x32_10(np.array([j, g, idx & 0xFFFFFFFF, idx >> 32], dtype=np.uint64),
                                    np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
            assert np.array_equal(w[j, i], want)


def test_uniforms_are_odd_multiples_of_2_to_minus_24_and_the_moments_fit():
    """2^20 draws of one column.  Five standard errors: U has variance 1/12 (|mean - 0.5| < 5 sqrt(1 / 12) / 1024 = 1.4e-3), z
    variance 1 (|mean| < 5 / 1024 = 4.9e-3) and z^2 variance 2 (|var - 1| < 5 sqrt(2) / 1024 = 6.9e-3).  The draws are fixed
    by the seed."""
    n = 2 ** 20
    u, z = GB.gibbs_normals_host(20260101, 0, n, [0])
    u, z = u[:, 0], z[:, 0].astype(np.float64)
    assert u.dtype == np.float32 and np.all(u > 0) and np.all(u < 1)
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.round(k)) and np.all(k.astype(np.int64) % 2 == 1)
    w = GB.gibbs_words_host(20260101, 0, n, [0])[:, 0, 0].astype(np.int64)
    assert np.array_equal(k.astype(np.int64), 2 * (w >> 9) + 1)
    assert abs(u.astype(np.float64).mean() - 0.5) < 1.4e-3
    assert abs(z.mean()) < 4.9e-3
    assert abs(z.var() - 1.0) < 6.9e-3
    assert np.abs(z).max() <= 5.9                                # sqrt(-2 log 2^-24) = 5.77


def test_draws_host_layout():
    hvt = np.asfortranarray(np.random.default_rng(1).uniform(1e4, 1e5, size=(300, 3)).astype(np.float32))
    unif, noise = GB.gibbs_draws_host(9, 4, hvt, [2, 0])
    assert unif.flags.f_contiguous and unif.shape == (300, 3) and np.all(unif[:, 1] == 0) and np.all(noise[:, 1] == 0)
    u, z = GB.gibbs_normals_host(9, 4, 300, [2, 0])
    assert np.array_equal(unif[:, [2, 0]], u)
    sd = np.float32(1.0) / np.sqrt(np.float32(2.0) * hvt[:, [2, 0]])
    assert np.array_equal(noise[:, [2, 0]], z * sd)
    # a column's draws do not depend on the other columns listed
    only, _ = GB.gibbs_draws_host(9, 4, hvt, [0])
    assert np.array_equal(only[:, 0], unif[:, 0])
    other, _ = GB.gibbs_draws_host(9, 5, hvt, [0])
    assert not np.array_equal(other[:, 0], unif[:, 0])


def test_prep_is_ldpred2s_c_terms():
    """mu_mult = C2, half_var_tau = 1 / (2 C4), u_logs = logit(p) - 0.5 log(1 + C1) with C1 = n h2 / (m p)."""
    n = np.array([5e4, 8e4, 1e5])
    m, p, h2 = 1000, 0.02, 0.3
    mm, hvt, ul = GB.gibbs_prep_host(n, m, p, h2)
    c1 = n * h2 / (m * p)
    c2 = c1 / (1 + c1)
    c4 = c2 / n
    assert np.allclose(mm, c2, rtol=1e-6) and np.allclose(hvt, 1 / (2 * c4), rtol=1e-6)
    assert np.allclose(ul, np.log(p / (1 - p)) - 0.5 * np.log1p(c1), rtol=1e-6)
    # postp of the paper == the sigmoid of the E-step's logit
    r = 0.01
    c3 = c2 * r
    postp = 1 / (1 + (1 - p) / p * np.sqrt(1 + c1) * np.exp(-c3 ** 2 / (2 * c4)))
    assert np.allclose(1 / (1 + np.exp(-(ul.astype(np.float64) + hvt.astype(np.float64) * c3 ** 2))), postp, rtol=1e-5)


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_sweep_host_equals_the_c_replay(low_memory, ld_dtype):
    ld, ss, inp = syn.make_problem(sizes=[130, 64, 1], low_memory=low_memory, ld_dtype=ld_dtype, seed=53, kind="longrange")
    m = ld.m
    pairs = ((0.5, 0.2), (0.9, 0.4))
    mm, hvt, ul = GR.chain_inputs(ss.n_per_snp, pairs)
    eta = {k: np.zeros((m, 2), dtype=np.float32, order="F") for k in ("host", "c")}
    q = {k: np.zeros((m, 2), dtype=np.float32, order="F") for k in ("host", "c")}
    for it in range(3):
        unif, noise = GB.gibbs_draws_host(5, it, hvt)
        a = GB.gibbs_sweep_host(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, inp.std_beta, mm, hvt, ul, unif, noise,
                                eta["host"], q["host"], ld.dq_scale)
        b = GR.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, inp.std_beta, mm, hvt, ul, unif, noise,
                            eta["c"], q["c"], ld.dq_scale)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert np.array_equal(eta["host"], eta["c"]) and np.array_equal(q["host"], q["c"])
    frac = np.count_nonzero(eta["c"], axis=0) / m
    assert np.all((frac > 0.05) & (frac < 0.95)), frac      # (both branches of the draw are taken)
    # one-dimensional arrays are one chain
    e1, q1 = np.zeros(m, dtype=np.float32), np.zeros(m, dtype=np.float32)
    unif, noise = GB.gibbs_draws_host(5, 0, hvt)
    GB.gibbs_sweep_host(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, inp.std_beta, mm[:, 0].copy(), hvt[:, 0].copy(),
                        ul[:, 0].copy(), unif[:, 0].copy(), noise[:, 0].copy(), e1, q1, ld.dq_scale)
    e2 = np.zeros((m, 2), dtype=np.float32, order="F")
    q2 = np.zeros((m, 2), dtype=np.float32, order="F")
    GR.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, inp.std_beta, mm, hvt, ul, unif, noise, e2, q2,
                    ld.dq_scale)
    assert np.array_equal(e1, e2[:, 0]) and np.array_equal(q1, q2[:, 0])


def test_strict_comparison_on_the_host():
    """gamma == U leaves the SNP out; the next float below includes it."""
    lb, ip, data = np.zeros(1, dtype=np.int32), np.array([0, 1], dtype=np.int64), np.ones(1, dtype=np.float32)
    beta = np.array([0.01], dtype=np.float32)
    mm, hvt, ul = (np.asarray(v) for v in GB.gibbs_prep_host(np.array([1e5]), 100, 0.3, 0.3))
    zero = lambda: np.zeros(1, dtype=np.float32)
    for sweep in (GB.gibbs_sweep_host, GR.replay_sweep):
        _, _, gam = sweep(lb, ip, data, False, beta, mm, hvt, ul, zero(), zero(), zero(), zero())
        g = gam[0]
        assert 0 < g < 1
        eta = zero()
        sweep(lb, ip, data, False, beta, mm, hvt, ul, np.array([g]), zero(), eta, zero())
        assert eta[0] == 0
        sweep(lb, ip, data, False, beta, mm, hvt, ul, np.array([np.nextafter(g, np.float32(0))]), zero(), eta, zero())
        assert eta[0] != 0


def test_inclusion_frequencies_on_an_identity_block():
    """One 64-SNP block whose LD is the identity: q stays 0, gamma_j is a constant of the SNP, and over 2 000 sweeps the SNP is
    included Binomial(2000, gamma_j) times: within 5 sqrt(gamma (1 - gamma) / 2000) of gamma for every SNP."""
    m, sweeps = 64, 2000
    lb, ip, data = np.arange(m, dtype=np.int32), np.arange(m + 1, dtype=np.int64), np.ones(m, dtype=np.float32)
    n = np.full(m, 1e5)
    beta = np.linspace(0.0, 0.0135, m).astype(np.float32)
    mm, hvt, ul = GR.chain_inputs(n, ((0.1, 0.1),), m_total=1000)
    eta, q = np.zeros((m, 1), dtype=np.float32, order="F"), np.zeros((m, 1), dtype=np.float32, order="F")
    count = np.zeros(m)
    gamma = None
    for it in range(sweeps):
        unif, noise = GB.gibbs_draws_host(77, it, hvt)
        _, _, gam = GR.replay_sweep(lb, ip, data, False, beta, mm, hvt, ul, unif, noise, eta, q)
        assert np.all(q == 0)
        gamma = gam[:, 0] if gamma is None else gamma
        assert np.array_equal(gam[:, 0], gamma)
        count += eta[:, 0] != 0
    g = gamma.astype(np.float64)
    assert g.min() <= 0.1 and g.max() >= 0.9, (g.min(), g.max())
    bound = 5.0 * np.sqrt(g * (1.0 - g) / sweeps)
    assert np.all(np.abs(count / sweeps - g) <= bound), np.max(np.abs(count / sweeps - g) / np.maximum(bound, 1e-300))
