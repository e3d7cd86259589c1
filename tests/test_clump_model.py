"""CPU: the model layer of clumping + thresholding through the `clump_fn` hook -- the effects of `ClumpThreshold` against
clumpings run at every p-value threshold on their own, `grid_table`, `select_best` for both criteria, `to_table`, and the
host path of `viprs_amd.stats.clump.clump`."""
import numpy as np
import pytest
from scipy.stats import chi2

from tests import genotype_score_reference as GR
from tests.test_clump_reference import dense_entries
from viprs_amd.data import ArrayDataLoader, SumstatsArrays
from viprs_amd.genotypes import counts_host, dose_table, score_host
from viprs_amd.io.plink_bed import pack_codes
from viprs_amd.model import ClumpThreshold
from viprs_amd.stats import clump as C
from viprs_amd.stats.ldsc import chisq_statistic

CHROM_SIZES = {1: [40, 25], 2: [33]}
R2 = (0.1, 0.3, 0.6)
P = (1e-4, 1e-2, 0.3, 1.0)


def _gdl(ld_dtype=np.int8):
    return ArrayDataLoader.synthetic(CHROM_SIZES, ld_dtype=ld_dtype, n=5e4, kind="longrange", h2=0.5)


def _merged(gdl, dtype):
    """The upper-form arrays of the loader's chromosomes, one after the other, as the model merges them."""
    from viprs_amd.data import merge_ld_arrays
    chroms = sorted(gdl.ld)
    lops = {c: gdl.ld[c].load(return_symmetric=False, dtype=dtype) for c in chroms}
    return merge_ld_arrays(chroms, gdl.shapes, {c: l.leftmost_idx for c, l in lops.items()},
                           {c: l.ld_indptr for c, l in lops.items()}, {c: l.ld_data for c, l in lops.items()})


def test_effects_and_grid_table():
    gdl = _gdl()
    calls = []

    def clump_fn(*a):
        calls.append(a)
        return C.clump_host(*a)

    model = ClumpThreshold(gdl, r2=R2, p_thresholds=P, dequantize_on_the_fly=True, clump_fn=clump_fn)
    assert model.post_mean_beta is None and model.n_models == 12
    with pytest.raises(ValueError, match="fit"):
        model.predict()
    assert model.fit() is model
    # one clumping call for all thresholds: the order holds every SNP up to the largest p-value, every SNP is a member
    (lb, ip, data, low_memory, order, r2, member, dq), = calls
    chisq = np.concatenate([chisq_statistic(gdl.sumstats_table[c]) for c in (1, 2)])
    assert data.dtype == np.int8 and low_memory and member is None and dq == 1.0 / 127.0 and np.array_equal(r2, R2)
    assert np.array_equal(order, C.clump_order(chisq, 0.0)) and order.shape[0] == gdl.m
    lb2, ip2, data2, seg = _merged(gdl, np.int8)
    assert np.array_equal(lb, lb2) and np.array_equal(ip, ip2) and np.array_equal(data, data2)
    b = np.concatenate([np.asarray(gdl.sumstats_table[c].get_snp_pseudo_corr(), dtype=np.float32) for c in (1, 2)])
    n_snps = []
    for g, r2_g in enumerate(R2):
        for t, p_t in enumerate(P):
            # model (r2_g, p_t) is the clumping run at p_t on its own: greedy clumping is prefix-consistent in the order
            cut = 0.0 if p_t >= 1.0 else chi2.isf(p_t, 1)
            alone = C.clump_host(lb, ip, data, True, C.clump_order(chisq, cut), r2_g, None, dq)
            keep = alone == np.arange(gdl.m)
            want = np.where(keep, b, np.float32(0.0))
            got = np.concatenate([model.post_mean_beta[c][:, g * len(P) + t] for c in (1, 2)])
            assert got.dtype == np.float32 and np.array_equal(got, want), (r2_g, p_t)
            n_snps.append(int(np.count_nonzero(want)))
    assert {c: v.shape for c, v in model.post_mean_beta.items()} == {1: (65, 12), 2: (33, 12)}
    assert list(model.grid_table.columns) == ["r2", "p_threshold", "n_snps"]
    assert model.grid_table["r2"].tolist() == [r for r in R2 for _ in P]
    assert model.grid_table["p_threshold"].tolist() == list(P) * len(R2)
    assert model.grid_table["n_snps"].tolist() == n_snps
    # the grid is not degenerate: more SNPs with a looser p-value and with a stricter LD threshold, and it thins out
    n = np.array(n_snps).reshape(len(R2), len(P))
    assert np.all(np.diff(n, axis=1) >= 0) and np.all(np.diff(n, axis=0) >= 0) and 0 < n.min() < n[0, -1] < n.max() <= gdl.m
    assert {c: v.shape for c, v in model.index_of.items()} == {1: (65, 3), 2: (33, 3)}
    assert model.index_of[2].min() >= 65 or model.index_of[2].min() == -1        # (indices of the merged plan)
    table = model.to_table()
    assert list(table.columns) == ["CHR", "IDX"] + [f"BETA_{i}" for i in range(12)] and len(table) == gdl.m
    assert np.array_equal(table["BETA_5"].to_numpy(), np.concatenate([model.post_mean_beta[c][:, 5] for c in (1, 2)]))


def test_defaults_and_refusals():
    gdl = _gdl(np.float32)
    model = ClumpThreshold(gdl, clump_fn=C.clump_host).fit()
    assert model.n_models == 36 and model.dequantize_scale == 1.0
    assert model.grid_table["r2"].tolist()[::9] == [0.1, 0.2, 0.5, 0.8]
    assert model.grid_table["p_threshold"].tolist()[:9] == [5e-8, 1e-6, 1e-4, 1e-3, 1e-2, 0.05, 0.1, 0.5, 1.0]

    class TwoRanks:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="world_size"):
        ClumpThreshold(gdl, clump_fn=C.clump_host, comm=TwoRanks())
    for kw in (dict(r2=[0.1] * 33), dict(r2=[-0.1]), dict(p_thresholds=[]), dict(p_thresholds=[0.0])):
        with pytest.raises(ValueError):
            ClumpThreshold(gdl, clump_fn=C.clump_host, **kw)


def _validation_loader(gdl, model, planted, seed=5, n=150):
    rng = np.random.default_rng(seed)
    geno, y = {}, np.zeros(n)
    for c in sorted(gdl.shapes):
        packed = pack_codes(GR.random_codes(rng, n, gdl.shapes[c], missing=0.02))
        geno[c] = (packed, n)
        beta = model.post_mean_beta[c][:, planted].astype(np.float64)
        y += score_host(packed, n, beta, dose_table(counts_host(packed, n), "mean", dtype=np.float64))
    return ArrayDataLoader({}, {}, n=n, genotype=geno, phenotype=y + 1e-3 * y.std() * rng.normal(size=n))


def test_select_best_by_validation():
    gdl = _gdl()
    model = ClumpThreshold(gdl, r2=R2, p_thresholds=P, dequantize_on_the_fly=True, clump_fn=C.clump_host).fit()
    planted = 6                                            # (r2 = 0.3, p = 0.3)
    grid = {c: b.copy() for c, b in model.post_mean_beta.items()}
    val = _validation_loader(gdl, model, planted)
    prs = model.predict(test_gdl=val)
    assert prs.shape == (150, 12) and np.all(np.isfinite(prs))
    with pytest.raises(ValueError, match="validation_gdl"):
        model.select_best()
    assert model.select_best(validation_gdl=val) is model
    r = np.asarray(model.validation_result["Validation_R2"])
    assert r.shape == (12,) and r[planted] == r.max() > 0.99 and r.min() < 0.99
    best = model.best_model_idx
    assert r[best] == r.max() and all(np.array_equal(grid[c][:, best], grid[c][:, planted]) for c in grid)
    assert all(np.array_equal(model.post_mean_beta[c], grid[c][:, best]) for c in grid) and model.n_models == 1
    assert model.predict(test_gdl=val).shape == (150,)
    assert list(model.to_table().columns) == ["CHR", "IDX", "BETA"]
    with pytest.raises(AssertionError):
        ClumpThreshold(gdl, clump_fn=C.clump_host).fit().select_best(criterion="ELBO")


def test_select_best_by_pseudo_validation():
    gdl = _gdl()
    model = ClumpThreshold(gdl, r2=R2, p_thresholds=P, dequantize_on_the_fly=True, clump_fn=C.clump_host).fit()
    rng = np.random.default_rng(11)
    vb = {c: np.asarray(gdl.sumstats_table[c].get_snp_pseudo_corr(), dtype=np.float64) + 0.002 * rng.normal(size=gdl.shapes[c])
          for c in gdl.shapes}
    got = model.pseudo_validate(vb)
    # (r'b)^2 / (b'Rb) from the dense matrix
    lb, ip, data, _ = _merged(gdl, np.int8)
    X, E = dense_entries(lb, ip, data, True)
    Rd = X / 127.0 + np.eye(gdl.m)
    B = np.concatenate([model.post_mean_beta[c] for c in (1, 2)]).astype(np.float64)
    r = np.concatenate([vb[c] for c in (1, 2)])
    want = (r @ B) ** 2 / np.einsum("ig,ig->g", B, Rd @ B)
    assert got.shape == (12,) and np.all(np.isfinite(want)) and np.allclose(got, want, rtol=1e-12, atol=0)
    grid = {c: b.copy() for c, b in model.post_mean_beta.items()}
    # as a loader with summary statistics, and as the dict itself
    val = ArrayDataLoader({}, {c: SumstatsArrays(vb[c], np.full(gdl.shapes[c], 5e4)) for c in vb})
    model.select_best(validation_gdl=val, criterion="pseudo_validation")
    assert np.allclose(model.validation_result["Pseudo_Validation_R2"], want, rtol=1e-12)
    assert model.best_model_idx == int(np.argmax(want)) and len(set(np.round(want, 12))) > 3
    assert all(np.array_equal(model.post_mean_beta[c], grid[c][:, model.best_model_idx]) for c in grid)
    again = ClumpThreshold(gdl, r2=R2, p_thresholds=P, dequantize_on_the_fly=True, clump_fn=C.clump_host).fit()
    assert again.select_best(validation_gdl=vb, criterion="pseudo_validation").best_model_idx == model.best_model_idx


def test_clump_on_the_host_path():
    gdl = _gdl()
    kw = dict(dequantize_on_the_fly=True, clump_fn=C.clump_host)
    got = C.clump(gdl, r2=0.05, p1=0.3, p2=0.8, **kw)
    assert sorted(got) == [1, 2]
    for c in (1, 2):
        lop = gdl.ld[c].load(return_symmetric=False, dtype=np.int8)
        chisq = chisq_statistic(gdl.sumstats_table[c])
        order = C.clump_order(chisq, chi2.isf(0.3, 1))
        member = chisq >= chi2.isf(0.8, 1)
        want = C.clump_host(lop.leftmost_idx, lop.ld_indptr, lop.ld_data, True, order, 0.05, member, 1.0 / 127.0)
        assert got[c].shape == (gdl.shapes[c],) and got[c].dtype == np.int32 and np.array_equal(got[c], want)
        assert 0 < order.shape[0] < gdl.shapes[c] and np.any(want == -1) and np.any((want >= 0) & (want != np.arange(gdl.shapes[c])))
        # both LD forms stand for the same matrix; several thresholds at once; chi^2 handed in
        sym = C.clump(gdl.ld[c], chisq=chisq, r2=(0.05, 0.3), p1=0.3, p2=0.8, low_memory=False, **kw)[None]
        assert sym.shape == (gdl.shapes[c], 2) and np.array_equal(sym[:, 0], want) and np.any(sym[:, 1] != sym[:, 0])
        # the natural order: LD pruning -- no kept pair reaches the threshold
        pruned = C.clump(gdl.ld[c], r2=0.05, order=np.arange(gdl.shapes[c]), **kw)[None]
        kept = np.flatnonzero(pruned == np.arange(gdl.shapes[c]))
        X, E = dense_entries(lop.leftmost_idx, lop.ld_indptr, lop.ld_data, True)
        Pm = E & (X * X >= 0.05 / ((1.0 / 127.0) * (1.0 / 127.0)))
        assert np.all(pruned >= 0) and 0 < kept.shape[0] < gdl.shapes[c] and not Pm[np.ix_(kept, kept)].any()
        assert np.all(Pm[pruned, np.arange(gdl.shapes[c])] | (pruned == np.arange(gdl.shapes[c])))
    with pytest.raises(ValueError, match="chisq"):
        C.clump(gdl.ld[1], r2=0.05, **kw)
