"""The order of `viprs_genotypes_class_sums` (tests/genotype_gwas_reference.py, a replay of include/viprs_hip.h) and what is
built on the class sums on the host: `class_sums_host`, `association`, `ArrayDataLoader.perform_gwas` and the loader form of
the pseudo_validation criterion.  No device."""
import os

import numpy as np
import pytest

from tests import genotype_gwas_reference as R
from viprs_amd import genotypes as G
from viprs_amd.io.plink_bed import pack_codes

HERE = os.path.dirname(os.path.abspath(__file__))
N_SIZES = [17, 33, 65, 257, 1025, 4097]


def test_replay_equals_int64_for_integer_values():
    rng = np.random.default_rng(11)
    for n in [1, 3, 16, 17, 65, 1025, 2049]:
        rows, codes = R.random_case(rng, 5, n)
        Y = rng.integers(-1000, 1000, size=(n, 3))
        want = np.stack([(codes == code).astype(np.int64) @ Y for code in R.CODES], axis=1)
        got = R.replay(rows, n, Y.astype(np.float64))
        assert got.shape == (5, 3, 3) and np.array_equal(got, want.astype(np.float64)), n


def test_replay_is_within_the_headers_bound_of_fsum_and_all_slots_agree():
    rng = np.random.default_rng(12)
    for n in [1, 15, 17, 65, 1023, 1025, 2049]:
        rows, _ = R.random_case(rng, 4, n)
        Y = rng.standard_normal((n, 2)) * np.exp(rng.uniform(-3, 3, size=(n, 1)))
        all64 = R.butterfly(R.slot_chains(R.terms(rows, n, Y)))
        assert np.all(all64 == all64[:, :, :1, :]), n
        err = np.abs(all64[:, :, 0, :] - R.exact(rows, n, Y))
        assert np.all(err <= R.bound(rows, n, Y)), (n, float((err / np.maximum(R.bound(rows, n, Y), 1e-300)).max()))


def test_replay_differs_from_the_plain_ascending_sum():
    """`==` on the device tells this order from another: for every n >= 33 some entry of the replay differs from the sum
    in ascending sample order (n = 17: one word, one slot, the same order, no difference)."""
    rng = np.random.default_rng(13)
    for n in N_SIZES:
        rows, _ = R.random_case(rng, 16, n, missing=0.05)
        Y = rng.standard_normal((n, 4))
        share = float(np.mean(R.replay(rows, n, Y) != R.ascending(rows, n, Y)))
        print(f"n = {n}: {share:.2f} of the entries differ from the ascending sum")
        assert (share > 0) == (n >= 33), (n, share)


def test_class_sums_host_is_within_the_bound_of_the_replay():
    rng = np.random.default_rng(14)
    for n in [1, 17, 65, 1025, 2049]:
        rows, _ = R.random_case(rng, 6, n)
        Y = rng.standard_normal((n, 3))
        got = G.class_sums_host(rows, n, Y)
        assert got.shape == (6, 3, 3) and got.dtype == np.float64
        # (each side within the header's bound of the exact sum)
        assert np.all(np.abs(got - R.replay(rows, n, Y)) <= 2.0 * R.bound(rows, n, Y)), n
        flat = G.class_sums_host(rows, n, Y[:, 1])
        assert flat.shape == (6, 3) and np.array_equal(flat, G.class_sums_host(rows, n, Y[:, 1:2])[:, :, 0])
        assert np.array_equal(G.HostGenotypes(rows, n).class_sums(Y), got)
    with pytest.raises(ValueError, match="NaN or inf"):
        G.class_sums_host(rows, n, np.full(n, np.nan))
    with pytest.raises(ValueError):
        G.class_sums_host(rows, n, np.zeros(n + 1))


def _cohort(rng, m, n, missing=0.1):
    """Codes with MAF >= 0.1 and the degenerate SNPs in front: 0 monomorphic, 1 all missing, 2 with two known genotypes."""
    codes = R.random_codes(rng, m, n, missing)
    codes[0] = 3
    codes[1] = 1
    codes[2] = 1
    codes[2, [3, n - 2]] = [0, 2]
    return codes


def _per_snp(codes, y, u):
    """N, BETA, SE, R per SNP over the complete pairs of the samples `u` by np.corrcoef and np.linalg.lstsq."""
    dose = np.array([2.0, np.nan, 1.0, 0.0])[codes]
    out = np.zeros((4, codes.shape[0]))
    for j in range(codes.shape[0]):
        ok = u & np.isfinite(dose[j])
        x, yy = dose[j, ok], y[ok]
        out[0, j] = ok.sum()
        if ok.sum() < 3 or np.ptp(x) == 0:
            continue
        A = np.stack([np.ones_like(x), x], axis=1)
        coef, res = np.linalg.lstsq(A, yy, rcond=None)[:2]
        out[1, j] = coef[1]
        out[2, j] = np.sqrt(res[0] / (ok.sum() - 2) / np.sum((x - x.mean()) ** 2))
        out[3, j] = np.corrcoef(x, yy)[0, 1]
    return out


def test_association_against_corrcoef_and_lstsq():
    """Missing genotypes, NaN phenotypes and a `keep` mask; two traits of unit scale in one pass, the second with a mask of
    its own.  Tolerance: `association_rtol(n)` relative, and the same figure absolute in units of the statistic's scale
    (R: 1; BETA and SE: sd(y) / sd(x) <= 1 / sqrt(2 0.1 0.9) < 2.4 here), since an error of the centred cross moment is
    relative to sqrt(cxx cyy), not to a correlation that may be near 0."""
    rng = np.random.default_rng(15)
    m, n = 24, 500
    codes = _cohort(rng, m, n)
    rows = pack_codes(codes, trailing_bits=rng.integers(0, 256, m))
    dose = np.array([2.0, 0.0, 1.0, 0.0])[codes]
    Y = np.stack([0.4 * dose[5] - 0.3 * dose[9] + rng.standard_normal(n), 0.5 * dose[7] + rng.standard_normal(n) + 30.0], axis=1)
    Y /= Y.std(axis=0)
    Y[rng.random((n, 2)) < 0.05] = np.nan
    keep = np.stack([rng.random(n) < 0.8, rng.random(n) < 0.6], axis=1)
    tol = R.association_rtol(n)
    g = G.HostGenotypes(rows, n)
    for kp in (None, keep[:, 0], keep):
        got = g.association(Y, keep=kp)
        assert set(got) == set(G.ASSOCIATION_FIELDS) and all(v.shape == (m, 2) and v.dtype == np.float64 for v in got.values())
        for t in range(2):
            u = np.isfinite(Y[:, t]) & (True if kp is None else kp if kp.ndim == 1 else kp[:, t])
            want = _per_snp(codes, Y[:, t], u)
            assert np.array_equal(got["N"][:, t], want[0])
            np.testing.assert_allclose(got["BETA"][:, t], want[1], rtol=tol, atol=2.4 * tol)
            np.testing.assert_allclose(got["SE"][:, t], want[2], rtol=tol, atol=2.4 * tol)
            np.testing.assert_allclose(got["R"][:, t], want[3], rtol=tol, atol=tol)
            live = want[2] > 0
            np.testing.assert_allclose(got["Z"][live, t], want[1][live] / want[2][live], rtol=4 * tol, atol=4 * tol * np.sqrt(n))
            # the degenerate SNPs: zeros and the true N
            for f in ("BETA", "SE", "Z", "R"):
                assert np.all(got[f][:3, t] == 0.0), f
            assert got["N"][1, t] == 0 and got["N"][2, t] <= 2 and got["N"][0, t] > 100
            assert np.all(np.abs(got["R"][3:, t]) <= 1.0) and abs(got["R"][5 if t == 0 else 7, t]) > 0.2
    # one complete trait: the mask column is dropped, the class counts are the exact counts
    y = np.nan_to_num(Y[:, 0])
    one = g.association(y)
    assert one["N"].shape == (m,) and np.array_equal(one["N"], g.counts()[:, [0, 2, 3]].sum(axis=1).astype(np.float64))
    np.testing.assert_allclose(one["R"], _per_snp(codes, y, np.ones(n, dtype=bool))[3], rtol=tol, atol=tol)
    c = g.counts().astype(np.float64)
    nn = c[:, 0] + c[:, 2] + c[:, 3]
    np.testing.assert_allclose(one["A1_FREQ"][nn > 0], ((2 * c[:, 0] + c[:, 2]) / (2 * np.maximum(nn, 1)))[nn > 0], rtol=1e-15)
    with pytest.raises(ValueError, match="keep"):
        g.association(y, keep=np.ones(n))
    with pytest.raises(ValueError, match="phenotype"):
        g.association(y[:-1])


# ---- the loader and the pseudo_validation criterion ----------------------------------------------------------------------
def _validation_loader(rng, m, n=300):
    from viprs_amd.data import ArrayDataLoader
    codes = R.random_codes(rng, m, n, 0.05)
    dose = np.array([2.0, 0.0, 1.0, 0.0])[codes]
    y = dose.T @ (rng.standard_normal(m) * (rng.random(m) < 0.05)) + rng.standard_normal(n)
    y[::17] = np.nan
    rows = pack_codes(codes, trailing_bits=rng.integers(0, 256, m))
    return ArrayDataLoader({}, {}, genotype={22: G.HostGenotypes(rows, n)}, phenotype=y), rows, y


def test_perform_gwas_fills_the_loader():
    from viprs_amd.data import ArrayDataLoader, SumstatsArrays
    rng = np.random.default_rng(16)
    gdl, rows, y = _validation_loader(rng, 40)
    assert gdl.sumstats_table == {} and gdl.n is None and gdl.m == 0
    out = gdl.perform_gwas()
    table = G.HostGenotypes(rows, 300).association(y)
    assert out is gdl.sumstats_table and isinstance(out[22], SumstatsArrays)
    assert np.array_equal(out[22].get_snp_pseudo_corr(), table["R"]) and np.array_equal(out[22].n_per_snp, table["N"])
    assert np.array_equal(out[22].get_chisq_statistic(), table["Z"] ** 2)
    assert set(gdl.gwas_table[22]) == set(G.ASSOCIATION_FIELDS)
    assert gdl.shapes == {22: 40} and gdl.m == 40 and gdl.n == float(table["N"].max())
    # a phenotype and a subset given to the call
    keep = np.arange(300) % 2 == 0
    gdl.perform_gwas(phenotype=2.0 * np.nan_to_num(y), keep=keep)
    assert np.array_equal(gdl.sumstats_table[22].n_per_snp, G.HostGenotypes(rows, 300).association(np.nan_to_num(y), keep)["N"])
    with pytest.raises(ValueError, match="no genotypes.*Remedy"):
        ArrayDataLoader({}, {}).perform_gwas()
    with pytest.raises(ValueError, match="no phenotype.*Remedy"):
        ArrayDataLoader({}, {}, genotype={22: G.HostGenotypes(rows, 300)}).perform_gwas()


def _fitted_grid():
    from oracle import oracle as O
    from tests.test_fit import loader_from_fixture
    from viprs_amd.model import HyperparameterGrid, VIPRSGrid
    fx = np.load(os.path.join(HERE, "golden", "fitgrid_independent.npz"))
    gdl = loader_from_fixture(fx)
    grid = HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=3, n_snps=gdl.m, h2_est=0.2, h2_se=0.1)
    return VIPRSGrid(gdl, grid, low_memory=True, e_step_fn=O.cpp_e_step).fit(pathwise=False, max_iter=20), gdl


def _copy_of(grid):
    import copy
    g2 = copy.copy(grid)
    for name in ("pip", "post_mean_beta", "post_var_beta", "var_gamma", "var_mu", "var_tau", "eta", "zeta", "q",
                 "_log_var_tau", "eta_diff"):
        setattr(g2, name, {c: v.copy() for c, v in getattr(grid, name).items()})
    g2.validation_result = grid.validation_result.copy()
    return g2


def test_pseudo_validation_takes_a_loader_after_perform_gwas():
    from viprs_amd.model.gridsearch import select_best_model
    from viprs_amd.model.gridsearch.grid_utils import pseudo_validation_std_beta
    grid, gdl = _fitted_grid()
    m = gdl.m
    rng = np.random.default_rng(17)
    val, rows, y = _validation_loader(rng, m)
    val.perform_gwas()
    by_hand = {22: val.sumstats_table[22].get_snp_pseudo_corr()}
    a = select_best_model(_copy_of(grid), validation_gdl=val, criterion="pseudo_validation")
    b = select_best_model(_copy_of(grid), validation_gdl=by_hand, criterion="pseudo_validation")
    assert a.best_model_idx == b.best_model_idx
    assert np.array_equal(a.validation_result["Pseudo_Validation_R2"], b.validation_result["Pseudo_Validation_R2"])
    assert len(set(np.asarray(a.validation_result["Pseudo_Validation_R2"]))) > 1
    # without SNP tables the SNP counts must agree
    short, _, _ = _validation_loader(rng, m - 1)
    short.perform_gwas()
    with pytest.raises(ValueError, match="SNP tables"):
        select_best_model(_copy_of(grid), validation_gdl=short, criterion="pseudo_validation")
    # aligned by SNP id: model SNP 5 is absent from the validation cohort, 7 has its alleles exchanged, 9 another pair
    ids = np.array([f"rs{j}" for j in range(m)])
    gdl.snp_table = {22: {"SNP": ids, "A1": np.full(m, "A"), "A2": np.full(m, "G")}}
    there = np.delete(np.arange(m), 5)
    a1, a2 = np.full(m, "A"), np.full(m, "G")
    a1[7], a2[7] = "G", "A"
    a2[9] = "T"
    order = rng.permutation(m - 1)                   # (the validation cohort lists its SNPs in another order)
    short.snp_table = {22: {"SNP": ids[there][order], "A1": a1[there][order], "A2": a2[there][order]}}
    r_short = short.sumstats_table[22].get_snp_pseudo_corr()
    want = np.zeros(m)
    want[there[order]] = r_short
    want[7] = -want[7]
    want[9] = 0.0
    assert want[5] == 0.0 and want[7] != 0.0
    got = pseudo_validation_std_beta(short, gdl)
    assert set(got) == {22} and np.array_equal(got[22], want)
    c = select_best_model(_copy_of(grid), validation_gdl=short, criterion="pseudo_validation")
    d = select_best_model(_copy_of(grid), validation_gdl={22: want}, criterion="pseudo_validation")
    assert c.best_model_idx == d.best_model_idx
    assert np.array_equal(c.validation_result["Pseudo_Validation_R2"], d.validation_result["Pseudo_Validation_R2"])
    gdl.snp_table = None


def test_pseudo_validation_per_chromosome_takes_a_loader():
    from oracle import oracle as O
    from tests import test_grid_per_chromosome as P
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import select_best_model_per_chromosome
    fx, gdl = P.load("fitchr_grid_3chr_upper")
    rng = np.random.default_rng(18)
    geno, n = {}, 250
    for c in gdl.chromosomes:
        codes = R.random_codes(rng, gdl.shapes[c], n, 0.05)
        geno[c] = G.HostGenotypes(pack_codes(codes, trailing_bits=rng.integers(0, 256, gdl.shapes[c])), n)
    val = ArrayDataLoader({}, {}, genotype=geno, phenotype=rng.standard_normal(n))
    val.perform_gwas()
    by_hand = {c: val.sumstats_table[c].get_snp_pseudo_corr() for c in gdl.chromosomes}
    a = select_best_model_per_chromosome(P.fit(fx, gdl, e_step_fn=O.cpp_e_step_grid), val, criterion="pseudo_validation")
    b = select_best_model_per_chromosome(P.fit(fx, gdl, e_step_fn=O.cpp_e_step_grid), by_hand, criterion="pseudo_validation")
    assert a.best_model_idx == b.best_model_idx and set(a.best_model_idx) == set(gdl.chromosomes)
    for c in gdl.chromosomes:
        assert np.array_equal(a.validation_result[c]["Pseudo_Validation_R2"], b.validation_result[c]["Pseudo_Validation_R2"])
        assert np.array_equal(a.post_mean_beta[c], b.post_mean_beta[c])
