"""CPU: the host reference of the LD scores (tests/ld_score_reference.py) against a dense float64 evaluation, the package's
host implementation (`viprs_amd.stats.ldsc.ld_scores_host`) against the reference, `simple_ldsc` against the formula, and
the model layer (`LDPredInf(h2=None)`, `h2_init=`) on the host path."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ld_score_reference as SR
from tests import ridge_reference as RR
from tests.test_gpu_ld_dot import _banded_windows
from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
from viprs_amd.stats import ldsc
from viprs_amd.utils import synthetic as syn

SIZES = (1, 2, 63, 64, 65, 130)
CHROM_SIZES = {1: [40, 25], 2: [33]}


def _dense_scores(ld, A, c, dq):
    """sum_k a_k (r^2 - (1 - r^2) c) off the diagonal, a_j on it, block by block from the dense float64 matrix."""
    out = np.zeros(A.shape)
    for bi, (s, e) in enumerate(zip(ld.block_start[:-1], ld.block_start[1:])):
        Rd = np.asarray(syn.dense_block(ld, bi), dtype=np.float64)
        r2 = Rd * Rd
        np.fill_diagonal(r2, 0.0)
        off = 1.0 - np.eye(e - s)
        out[s:e] = r2 @ A[s:e] + c * ((r2 - off) @ A[s:e]) + A[s:e]
    return out


@pytest.mark.parametrize("low_memory", [False, True])
@pytest.mark.parametrize("kind, ld_dtype", [("ar1", np.float32), ("longrange", np.int8), ("sample", np.int16)])
def test_reference_against_the_dense_matrix(kind, ld_dtype, low_memory):
    ld = syn.make_ld(SIZES, low_memory=low_memory, ld_dtype=ld_dtype, kind=kind)
    m = ld.m
    rng = np.random.default_rng(3)
    A = rng.standard_normal((m, 3))
    ref = SR.sums(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, A, mode="fsum")
    assert np.array_equal(ref["L"], np.concatenate([np.full(b, b - 1) for b in SIZES]))
    for c in (0.0, 1.0 / 98.0):
        corr = None if c == 0.0 else np.full(m, c)
        got = SR.exact_score(ref, corr, ld.dq_scale, np.float64)
        want = _dense_scores(ld, A, c, ld.dq_scale)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * (1.0 + np.abs(want).max()))
        # the epilogue in float64 NumPy scalars is the same number up to its own roundings
        fin = SR.finish(ref["S2"], ref["S0"], A, corr, ld.dq_scale, np.float64)
        assert np.all(np.abs(fin - got) <= SR.bound(ref, corr, ld.dq_scale, np.float64, ld.ld_data.dtype.itemsize))
    # unit weights: one column of ones
    unit = SR.sums(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, None, mode="fsum")
    ones = SR.sums(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, np.ones(m), mode="fsum")
    assert np.array_equal(unit["S2"], ones["S2"]) and np.array_equal(unit["S0"], ref["L"].astype(np.float64))


def _cases():
    for low_memory in (False, True):
        ld = syn.make_ld(SIZES, low_memory=low_memory, ld_dtype=np.int8, kind="longrange")
        yield ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, ld.dq_scale
        lb, ip = _banded_windows(400, 30, 45, low_memory, seed=14, jitter=20)
        data = np.random.default_rng(15).uniform(-1, 1, int(ip[-1])).astype(np.float32)
        yield lb, ip, data, low_memory, 1.0


def test_host_implementation_against_the_reference():
    for lb, ip, data, low_memory, dq in _cases():
        m = lb.shape[0]
        rng = np.random.default_rng(4)
        corr = rng.uniform(0.0, 0.02, m)
        for A in (None, rng.standard_normal(m), rng.standard_normal((m, 4))):
            ref = SR.sums(lb, ip, data, low_memory, A, mode="fsum")
            for c in (None, corr):
                got = ldsc.ld_scores_host(lb, ip, data, low_memory, A, c, dq)
                want = SR.exact_score(ref, c, dq, np.float64)
                assert got.shape == ((m,) if A is None else A.shape) and got.dtype == np.float64
                scale = dq * dq * ref["P"] + ref["Q"] + np.abs(ref["A"])
                assert np.all(np.abs(got - want) <= 1e-13 * scale)
        # a stored zero is an entry, a gap of the window is not: S0 counts the former only
        unit = SR.sums(lb, ip, data, low_memory, None, mode="fsum")
        big = ldsc.ld_scores_host(lb, ip, np.zeros_like(data), low_memory, None, np.ones(m), dq)
        assert np.array_equal(big, 1.0 - unit["L"])


def _gdl(**kw):
    return ArrayDataLoader.synthetic(CHROM_SIZES, ld_dtype=np.int8, n=5e4, kind="longrange", ld_sample_size=5e4, **kw)


def _formula(gdl, scores):
    chi2 = np.concatenate([gdl.sumstats_table[c].n_per_snp * gdl.sumstats_table[c].get_snp_pseudo_corr().astype(np.float64) ** 2
                           for c in sorted(scores)])
    n = np.concatenate([gdl.sumstats_table[c].n_per_snp for c in sorted(scores)])
    ell = np.concatenate([scores[c] for c in sorted(scores)])
    return (chi2.mean() - 1.0) * chi2.shape[0] / (ell.mean() * n.mean())


def test_simple_ldsc_against_the_formula():
    gdl = _gdl()
    assert all(ld.sample_size == 5e4 for ld in gdl.ld.values())
    for corrected in (True, False):
        scores = ldsc.ld_scores(gdl, corrected=corrected, score_fn=ldsc.ld_scores_host)
        for c, ld in gdl.ld.items():
            lop = ld.load(return_symmetric=False, dtype=np.float32)
            want = ldsc.ld_scores_host(lop.leftmost_idx, lop.ld_indptr, lop.ld_data, True, None,
                                       np.full(gdl.shapes[c], 1.0 / (5e4 - 2.0)) if corrected else None, 1.0)
            assert np.array_equal(scores[c], want)
            # both LD forms stand for the same matrix
            sym = ldsc.ld_scores(ld, corrected=corrected, low_memory=False, score_fn=ldsc.ld_scores_host)[None]
            np.testing.assert_allclose(sym, want, rtol=1e-12)
        h2 = ldsc.simple_ldsc(gdl, corrected=corrected, score_fn=ldsc.ld_scores_host)
        assert h2 == pytest.approx(_formula(gdl, scores), rel=1e-14)
        assert h2 == ldsc.simple_ldsc(gdl, ld_scores=scores)
    # attached scores are used where present; the real statistic where the caller has it
    with pytest.raises(ValueError, match="annotate_ld_scores"):
        gdl.ld[1].ld_score
    att = ldsc.annotate_ld_scores(gdl, score_fn=ldsc.ld_scores_host)
    assert all(np.array_equal(gdl.ld[c].ld_score, att[c]) for c in att)
    assert ldsc.simple_ldsc(gdl) == ldsc.simple_ldsc(gdl, ld_scores=att)
    ss = gdl.sumstats_table[1]
    assert np.array_equal(ss.get_chisq_statistic(), ss.n_per_snp * ss.get_snp_pseudo_corr().astype(np.float64) ** 2)
    chisq = np.full(gdl.shapes[1], 3.0)
    assert np.array_equal(SumstatsArrays(ss.get_snp_pseudo_corr(), ss.n_per_snp, chisq=chisq).get_chisq_statistic(), chisq)
    # no sample size, no corrected scores: the error names the remedy
    bare = LDArrays(upper=gdl.ld[2]._forms[False], stored_dtype=np.int8, dq_scale=gdl.ld[2].dq_scale)
    with pytest.raises(ValueError, match="sample_size"):
        ldsc.ld_scores(bare, score_fn=ldsc.ld_scores_host)
    assert ldsc.ld_scores(bare, corrected=False, score_fn=ldsc.ld_scores_host)[None].shape == (33,)


def test_ldsc_estimate_over_is_the_estimate_of_the_concatenations():
    gdl = _gdl()
    ss = gdl.sumstats_table
    scores = ldsc.ld_scores(gdl, score_fn=ldsc.ld_scores_host)
    for chroms in (sorted(ss), sorted(ss)[::-1], sorted(ss)[:1]):
        want = ldsc.ldsc_estimate(np.concatenate([ldsc.chisq_statistic(ss[c]) for c in chroms]),
                                  np.concatenate([scores[c] for c in chroms]),
                                  np.concatenate([ss[c].n_per_snp for c in chroms]))
        assert ldsc.ldsc_estimate_over(ss, scores, chroms) == want
    assert ldsc.ldsc_estimate_over(ss, scores, sorted(ss)) == ldsc.simple_ldsc(gdl, ld_scores=scores)


def test_zarr_store_answers_ld_scores(tmp_path):
    from viprs_amd.io.zarr_ld import ZarrLDMatrix, write_ld_store
    up = syn.make_ld([20, 13], low_memory=True, ld_dtype=np.int8, kind="longrange")
    stored = np.arange(33, dtype=np.float64) + 1.0
    write_ld_store(str(tmp_path / "with"), up.ld_indptr, up.ld_data, attrs={"Sample size": 400},
                   metadata={"ldscore": stored})
    write_ld_store(str(tmp_path / "without"), up.ld_indptr, up.ld_data, attrs={"Sample size": 400})
    assert np.array_equal(ZarrLDMatrix(str(tmp_path / "with")).ld_score, stored)
    mat = ZarrLDMatrix(str(tmp_path / "without"))
    with pytest.raises(ValueError, match="annotate_ld_scores"):
        mat.ld_score
    got = ldsc.annotate_ld_scores({7: mat}, dequantize_on_the_fly=True, score_fn=ldsc.ld_scores_host)[7]
    want = ldsc.ld_scores_host(up.ld_left_bound, up.ld_indptr, up.ld_data, True, None, np.full(33, 1.0 / 398.0), up.dq_scale)
    assert np.array_equal(got, want) and np.array_equal(mat.ld_score, want)


def test_ldpredinf_estimates_h2_on_the_host_path():
    from viprs_amd.model import LDPredInf
    gdl = _gdl()
    calls = []

    def score_fn(*a):
        calls.append(a)
        return ldsc.ld_scores_host(*a)

    model = LDPredInf(gdl, dequantize_on_the_fly=True, solve_fn=RR.solve, score_fn=score_fn)
    (lb, ip, data, low_memory, weights, corr, dq), = calls
    assert data.dtype == np.int8 and low_memory and weights is None and dq == 1.0 / 127.0
    assert np.array_equal(corr, np.full(gdl.m, 1.0 / (5e4 - 2.0)))
    want = ldsc.simple_ldsc(gdl, dequantize_on_the_fly=True, score_fn=ldsc.ld_scores_host)
    assert model.h2 == pytest.approx(want, rel=1e-14) and 0.0 < model.h2 <= 1.0 and model.get_heritability() == model.h2
    # LD of unknown sample size: no corrected scores, the error names the remedies
    with pytest.raises(ValueError, match="sample_size.*pass h2"):
        LDPredInf(ArrayDataLoader.synthetic(CHROM_SIZES, ld_dtype=np.int8, n=5e4, kind="longrange"), solve_fn=RR.solve)
    # (the default of the host path is the host implementation itself)
    assert LDPredInf(gdl, dequantize_on_the_fly=True, solve_fn=RR.solve).h2 == model.h2
    model.fit()
    assert model.lam == gdl.m / (model.n * model.h2) and model.solve_info.converged
    # an estimate outside (0, 1] is refused with its value
    null = ArrayDataLoader(gdl.ld, {c: SumstatsArrays(np.zeros(m), np.full(m, 5e4)) for c, m in gdl.shapes.items()})
    with pytest.raises(ValueError, match=r"h2 = -"):
        LDPredInf(null, solve_fn=RR.solve)


def test_h2_init_ldsc_against_the_formula():
    from viprs_amd.model import VIPRS, VIPRSMix, VIPRSMixPerChromosome, VIPRSPerChromosome
    gdl = _gdl()
    calls = []

    def score_fn(*a):
        calls.append(a)
        return ldsc.ld_scores_host(*a)

    scores = ldsc.ld_scores(gdl, score_fn=ldsc.ld_scores_host)
    pooled = _formula(gdl, scores)
    own = {c: _formula(gdl, {c: scores[c]}) for c in scores}
    assert len({round(v, 6) for v in own.values()}) == 2 and 0.01 < pooled < 0.99
    m = gdl.m
    model = VIPRS(gdl, e_step_fn=O.cpp_e_step, h2_init="ldsc", score_fn=score_fn)
    assert not calls                                   # computed where the hyper-parameters need it, once
    model.initialize_theta({"pi": 0.02})
    model.initialize_theta({"pi": 0.02})
    assert len(calls) == 2 and model.h2_ldsc["*"] == pytest.approx(pooled, rel=1e-14)
    assert float(model.sigma_epsilon) == np.float32(1.0 - pooled)
    assert float(model.tau_beta) == pytest.approx(0.02 * m / pooled, rel=1e-6)
    # given sigma_epsilon or tau_beta, nothing is computed
    calls.clear()
    fixed = VIPRS(gdl, e_step_fn=O.cpp_e_step, h2_init="ldsc", score_fn=score_fn)
    fixed.initialize_theta({"pi": 0.02, "sigma_epsilon": 0.9})
    fixed.initialize_theta({"pi": 0.02, "tau_beta": 50.0})
    assert not calls and float(fixed.sigma_epsilon) == np.float32(np.clip(1.0 - 0.02 * m / 50.0, 1e-4, 1.0 - 1e-4))
    # a number: clipped as the reference clips its estimate
    num = VIPRS(gdl, e_step_fn=O.cpp_e_step, h2_init=0.999)
    num.initialize_theta({"pi": 0.02})
    assert float(num.sigma_epsilon) == np.float32(1.0 - 0.99)
    mix = VIPRSMix(gdl, K=3, e_step_fn=O.cpp_e_step_mixture, h2_init=1e-6)
    mix.initialize_theta({"pis": np.array([0.01, 0.01, 0.01])})
    assert float(mix.sigma_epsilon) == np.float32(1.0 - 1e-3)
    mix = VIPRSMix(gdl, K=3, e_step_fn=O.cpp_e_step_mixture, h2_init="ldsc")
    mix.initialize_theta({"pis": np.array([0.01, 0.01, 0.01])})
    assert float(mix.sigma_epsilon) == np.float32(1.0 - pooled)
    np.testing.assert_allclose(mix.tau_beta, mix.d * (m * np.dot(1.0 / mix.d, mix.pi) / pooled), rtol=1e-6)
    # one model per chromosome: every chromosome starts from its own estimate
    per = VIPRSPerChromosome(gdl, e_step_fn=O.cpp_e_step, h2_init="ldsc")
    per.fit(max_iter=1, theta_0={"pi": 0.02})
    for c in per.groups:
        assert per.h2_ldsc[c] == pytest.approx(own[c], rel=1e-14)
        h2 = float(np.clip(own[c], 0.01, 0.99))
        assert per.history[c]["ELBO"] and per._em is not None
        pi, sig, tau = per._theta_for(c, {"pi": 0.02})
        assert sig == 1.0 - h2 and tau == 0.02 * gdl.shapes[c] / h2
    perm = VIPRSMixPerChromosome(gdl, K=2, e_step_fn=O.cpp_e_step_mixture, h2_init="ldsc")
    seen = []
    start = VIPRSMix.initialize_theta

    def spy(self, theta_0=None):
        start(self, theta_0)
        seen.append(float(self.sigma_epsilon))
    try:
        VIPRSMix.initialize_theta = spy
        perm.fit(max_iter=1, theta_0={"pis": np.array([0.01, 0.01])})
    finally:
        VIPRSMix.initialize_theta = start
    assert seen == [float(np.float32(1.0 - np.clip(own[c], 1e-3, 1.0 - 1e-3))) for c in perm.groups]

    class TwoRanks:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="world_size"):
        VIPRS(gdl, e_step_fn=O.cpp_e_step, h2_init="ldsc", comm=TwoRanks())
    with pytest.raises(ValueError, match="h2_init"):
        VIPRS(gdl, e_step_fn=O.cpp_e_step, h2_init="ldscore")


@pytest.mark.parametrize("cls_name", ["VIPRS", "VIPRSMix"])
def test_h2_init_none_changes_nothing(cls_name):
    import viprs_amd.model as M
    gdl = _gdl()
    kw = dict(e_step_fn=O.cpp_e_step) if cls_name == "VIPRS" else dict(K=3, e_step_fn=O.cpp_e_step_mixture)
    runs = []
    for extra in ({}, {"h2_init": None}):
        np.random.seed(1234)
        model = getattr(M, cls_name)(gdl, **kw, **extra).fit(max_iter=15)
        runs.append((model, np.random.get_state()))
    (a, sa), (b, sb) = runs
    assert a.history["ELBO"] == b.history["ELBO"] and len(a.history["ELBO"]) > 1
    assert float(a.sigma_epsilon) == float(b.sigma_epsilon) and np.array_equal(a.tau_beta, b.tau_beta)
    for c in a.post_mean_beta:
        assert np.array_equal(a.post_mean_beta[c], b.post_mean_beta[c])
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
