"""CPU: the SBayesR definition of viprs_amd/stats/bayesr.py -- the algebra that makes its update the mixture E-step's, the
host sweep `==` the C replay (tests/bayesr_replay.c), the tagged Philox stream, the component frequencies of the draw, the
sums."""
import numpy as np
import pytest

from tests import bayesr_replay as R
from tests import per_snp_inputs as PS
from viprs_amd.stats import bayesr as B
from viprs_amd.stats import cs as CS
from viprs_amd.stats import gibbs as GB
from viprs_amd.utils import synthetic as syn

SEED = 0x5DEECE66D1234567


def test_the_update_is_the_mixture_e_steps():
    """Section by section against the textbook conditional in float64: mean n r / C, variance sigma2_e / C, log-weight
    log pi_k - 0.5 log(1 + n gamma_k sigma2_beta / sigma2_e) + n^2 r^2 / (2 C sigma2_e), with C = n + sigma2_e / (gamma_k
    sigma2_beta).  The inputs are float32 (relative rounding 2^-24 each, a handful of them per expression): 1e-6."""
    rng = np.random.default_rng(3)
    m = 200
    n = 1e5 * 10.0 ** rng.uniform(-1, 0.3, m)
    pi, gamma, s2b, s2e = np.array([0.9, 0.05, 0.03, 0.02]), np.array([0.01, 0.1, 1.0]), 2.3e-5, 0.7
    mm, sv, ul, lnp = B.bayesr_prep_host(n, pi, gamma, s2b, s2e)
    assert mm.dtype == sv.dtype == ul.dtype == lnp.dtype == np.float32 and mm.shape == (m, 3) and lnp.shape == (m,)
    C = n[:, None] + s2e / (gamma * s2b)[None, :]
    r = 0.01 * rng.standard_normal(m)
    mean = n[:, None] * r[:, None] / C
    var = s2e / C
    logw = np.log(pi[1:])[None, :] - 0.5 * np.log1p(n[:, None] * (gamma * s2b)[None, :] / s2e) + (n[:, None] * r[:, None]) ** 2 / (2 * C * s2e)
    mu = mm.astype(np.float64) * r[:, None]
    assert np.allclose(mu, mean, rtol=1e-6, atol=0)
    assert np.allclose(1.0 / (2.0 * sv.astype(np.float64) ** 2), var, rtol=1e-6, atol=0)
    u = ul.astype(np.float64) + (sv.astype(np.float64) * mu) ** 2
    assert np.allclose(u, logw, rtol=0, atol=1e-6 * np.abs(logw).max())
    assert np.allclose(lnp, np.log(pi[0]), rtol=1e-7)
    # sd of the draw: float32(1 / sqrt 2) / sqrt_half_var_tau
    assert B.INV_SQRT2_F32 == np.float32(np.sqrt(0.5))
    assert np.allclose((B.INV_SQRT2_F32 / sv).astype(np.float64) ** 2, var, rtol=1e-6)
    # and what prep_mixture is handed says the same
    lp, lt, tau, lnp0, se, lam1 = B.bayesr_prep_args(pi, gamma, s2b, s2e)
    assert np.allclose(lp, np.log(pi[1:])) and np.allclose(tau, 1 / (gamma * s2b)) and np.allclose(lt, np.log(tau))
    assert lnp0 == np.log(pi[0]) and se == s2e and lam1 == 1.0
    vt = n[:, None] * lam1 / se + tau[None, :]                       # prep_mixture_body, csrc/abi_state.hip
    assert np.array_equal((n[:, None] / (vt * se)).astype(np.float32), mm) and np.array_equal(np.sqrt(0.5 * vt).astype(np.float32), sv)
    assert np.array_equal((lp[None, :] + 0.5 * (lt[None, :] - np.log(vt))).astype(np.float32), ul)


def _case(low_memory, ld_dtype, K, sizes=(130, 64, 1)):
    ld, ss, inp = syn.make_problem(sizes=list(sizes), low_memory=low_memory, ld_dtype=ld_dtype, seed=53, kind="longrange")
    return ld, inp.std_beta, R.spread_inputs(ld.m, K)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_sweep_host_equals_the_c_replay(low_memory, ld_dtype, K):
    ld, beta, (mm, sv, ul, lnp) = _case(low_memory, ld_dtype, K)
    m = ld.m
    state = [(np.zeros(m, np.float32), np.zeros(m, np.float32)) for _ in range(2)]
    for it in range(2):
        unif, z = B.bayesr_draws_host(SEED, it, m)
        outs = []
        for fn, (eta, q) in zip((B.bayesr_sweep_host, R.replay_sweep), state):
            outs.append(fn(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, beta, mm, sv, ul, lnp, unif, z, eta, q,
                           ld.dq_scale))
        for a, b, name in zip(outs[0], outs[1], ("eta_diff", "var_mu", "var_gamma", "kstar")):
            assert a.dtype == b.dtype and np.array_equal(a, b), (it, name)
        assert np.array_equal(state[0][0], state[1][0]) and np.array_equal(state[0][1], state[1][1]), it
        ks = outs[1][3]
        assert set(np.unique(ks)) == set(range(K + 1))
        assert np.array_equal(state[1][0] != 0, ks != 0)


def test_spread_parameters_give_every_outcome_in_every_block():
    """What tests/test_gpu_bayesr.py relies on, established here by the C replay alone: on the plan of the panel roles with
    per-SNP inputs every k* = 0 .. K occurs in every block of 64 or more SNPs, in both of two sweeps."""
    for K in (1, 3):
        ld, beta, (mm, sv, ul, lnp) = _case(False, np.int8, K, sizes=(2370, 1601, 130, 64, 1))
        eta, q = np.zeros(ld.m, np.float32), np.zeros(ld.m, np.float32)
        bs = np.asarray(ld.block_start)
        for it in range(2):
            unif, z = B.bayesr_draws_host(SEED, it, ld.m)
            ks = R.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False, beta, mm, sv, ul, lnp, unif, z, eta, q,
                                ld.dq_scale)[3]
            assert R.every_outcome_in_every_block(ks, bs, K), (K, it)
        for a in (mm, sv, ul):                       # the inputs differ from SNP to SNP
            assert np.all(np.abs(np.diff(a.astype(np.float64), axis=0)).max(axis=0) > 0)
        assert np.unique(lnp).shape[0] > ld.m // 2


def _philox_ints(c, k):
    """Philox4x32-10 on Python integers (Salmon et al. 2011)."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_philox_known_answers_of_the_tagged_counter():
    # the published vectors of Random123 first: the integer routine is Philox
    assert _philox_ints([0] * 4, [0] * 2) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox_ints([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    idx = 2 ** 40 + 5
    w = B.bayesr_words_host(SEED, idx, 12346)
    assert w.dtype == np.uint32 and w.shape == (12346, 4)
    # recorded words of counter (j, 2^30, 5, 256) under key (0xD1234567, 0x5DEECE66)
    assert [int(x) for x in w[0]] == [0xec72edb5, 0x5fb23007, 0xc1e20f45, 0x2ae323e0]
    assert [int(x) for x in w[12345]] == [0xfeba31f8, 0x0a44b72c, 0xf97858b1, 0x8a369b6b]
    for j in (0, 1, 777, 12345):
        assert [int(x) for x in w[j]] == _philox_ints([j, 1 << 30, idx & 0xFFFFFFFF, idx >> 32], [SEED & 0xFFFFFFFF, SEED >> 32])
    unif, z = B.bayesr_draws_host(SEED, idx, 12346)
    k = unif.astype(np.float64) * 2.0 ** 24
    assert unif.dtype == z.dtype == np.float32 and np.all((unif > 0) & (unif < 1))
    assert np.array_equal(k, 2 * (w[:, 0].astype(np.int64) >> 9) + 1)
    assert abs(float(z.mean())) < 5 / np.sqrt(12346) and abs(float(z.var()) - 1) < 5 * np.sqrt(2 / 12346)


def test_the_stream_shares_no_block_with_the_gibbs_and_cs_streams():
    """Equal (seed, draw_index): the second counter word is a column < 2^30 (Gibbs), a column + 2^31 (PRS-CS) or 2^30."""
    assert B.STREAM_TAG == 2 ** 30 and CS.CS_TAG == 2 ** 31
    m, cols = 512, np.arange(8)
    mine = {tuple(r) for r in B.bayesr_words_host(SEED, 9, m).tolist()}
    assert len(mine) == m
    for other in (GB.gibbs_words_host(SEED, 9, m, cols), CS.cs_words_host(SEED, 9, m, cols)):
        assert mine.isdisjoint({tuple(r) for r in other.reshape(-1, 4).tolist()})
    # ... and its counter is the one the docstring states: moving the tag onto a Gibbs column reproduces that stream
    assert np.array_equal(GB.gibbs_words_host(SEED, 9, m, [B.STREAM_TAG])[:, 0], B.bayesr_words_host(SEED, 9, m))


def test_component_frequencies_follow_the_softmax_weights():
    """One SNP, fixed q, 2^16 draws: the frequency of every outcome within 5 binomial standard errors of its weight."""
    N, K = 2 ** 16, 3
    mm, sv, ul, lnp = B.bayesr_prep_host(np.array([8e4]), (0.4, 0.2, 0.2, 0.2), (0.25, 1.0, 4.0), 1e-5, 1.0)
    beta, q = np.float32(0.004), np.float32(-0.001)
    unif, z = B.bayesr_draws_host(SEED, 3, N)
    mu, gam, _, _, _ = B.bayesr_snp_host(beta, q, mm[0], sv[0], ul[0], lnp[0], unif[0], z[0], np.float32(0))
    w = np.concatenate([[1.0 - gam.astype(np.float64).sum()], gam.astype(np.float64)])
    assert np.all(w > 0.05)
    ks = np.array([B.bayesr_snp_host(beta, q, mm[0], sv[0], ul[0], lnp[0], unif[i], z[i], np.float32(0))[2] for i in range(0, N)])
    freq = np.bincount(ks, minlength=K + 1) / N
    se = np.sqrt(w * (1 - w) / N)
    print("weights", w, "frequencies", freq, "standard errors", se)
    assert np.all(np.abs(freq - w) <= 5 * se)
    # the draw itself: mean mu_k and standard deviation sd_k within 5 standard errors on the SNPs that chose k
    b = np.array([B.bayesr_snp_host(beta, q, mm[0], sv[0], ul[0], lnp[0], unif[i], z[i], np.float32(0))[3] for i in range(0, N, 16)])
    kk = ks[::16]
    for k in range(1, K + 1):
        x = b[kk == k].astype(np.float64)
        sd = float(B.INV_SQRT2_F32 / sv[0, k - 1])
        assert abs(x.mean() - float(mu[k - 1])) < 5 * sd / np.sqrt(x.shape[0]) and abs(x.std() / sd - 1) < 5 / np.sqrt(2 * x.shape[0])
    assert np.all(b[kk == 0] == 0)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 2370])
def test_sums_against_a_direct_count(m):
    rng = np.random.default_rng(m)
    K = 3
    ks = rng.integers(0, K + 1, m).astype(np.int32)
    eta = np.where(ks > 0, 0.01 * rng.standard_normal(m), 0).astype(np.float32)
    q, beta = (0.01 * rng.standard_normal(m)).astype(np.float32), (0.01 * rng.standard_normal(m)).astype(np.float32)
    s = B.bayesr_sums_host(ks, eta, q, beta, K)
    assert s.shape == (2 * K + 4,) and s.dtype == np.float64
    assert np.array_equal(s[:K + 1], np.bincount(ks, minlength=K + 1).astype(np.float64))
    e = eta.astype(np.float64)
    want = [e[ks == k] @ e[ks == k] for k in range(1, K + 1)] + [q.astype(np.float64) @ e, e @ e, beta.astype(np.float64) @ e]
    assert np.allclose(s[K + 1:], want, rtol=1e-12, atol=1e-18)
    assert np.isclose(s[K + 1:2 * K + 1].sum(), s[2 * K + 2], rtol=1e-12)


def test_accumulate_host_and_hyper_parameter_draws():
    rng = np.random.default_rng(5)
    gam, mu = rng.random((50, 3)).astype(np.float32) / 3, rng.standard_normal((50, 3)).astype(np.float32)
    mean, pip = np.zeros(50), np.zeros(50)
    B.bayesr_accumulate_host(gam, mu, mean, pip)
    g, mm = gam.astype(np.float64), mu.astype(np.float64)
    assert np.array_equal(mean, (g[:, 0] * mm[:, 0] + g[:, 1] * mm[:, 1]) + g[:, 2] * mm[:, 2])
    assert np.array_equal(pip, (g[:, 0] + g[:, 1]) + g[:, 2])
    pi = B.draw_pi(np.random.default_rng(1), [900, 50, 30, 0])
    assert pi.shape == (4,) and np.all(pi > 0) and abs(pi.sum() - 1) < 1e-12
    a, b = np.random.default_rng(2), np.random.default_rng(2)
    assert B.draw_sigma2_beta(a, [1e-4, 2e-4, 3e-4], [0.01, 0.1, 1.0], 80, 1e-5) == \
        (1e-4 / 0.01 + 2e-4 / 0.1 + 3e-4 + 4 * 1e-5) / b.chisquare(84)
    a, b = np.random.default_rng(3), np.random.default_rng(3)
    assert B.draw_sigma2_e(a, 5e4, 0.3, 0.25, 0.05, 0.4) == (5e4 * (1 - 0.6 + 0.25 + 0.05) + 4 * 0.4) / b.chisquare(5e4 + 4)
    assert B.draw_sigma2_e(np.random.default_rng(3), 5e4, 2.0, 0.25, 0.05, 0.4) == B.SIGMA2_E_MIN          # the floor
    assert np.isclose(B.initial_sigma2_beta(0.5, 1000, B.DEFAULT_PI, B.DEFAULT_GAMMA), 0.5 / (1000 * 0.0122))
