"""The `SuSiE` model class driven on the host (`fit_fn = susie_host`) over a two-chromosome synthetic loader: the merged plan,
the per-chromosome split, `to_table()`, the warning of a block that stops at `max_iter`, `prior_weights`."""
import warnings

import numpy as np
import pytest

from viprs_amd.data import ArrayDataLoader, SumstatsArrays
from viprs_amd.model import SuSiE
from viprs_amd.stats import susie as S

CHROM_SIZES = {1: [120, 65], 2: [90]}
N = 5e4
PLANTED = {1: {20: 8.0, 150: -7.0}, 2: {45: 6.0}}            # SNP index inside the chromosome -> z of the planted effect


def loader(ld_dtype=np.int8):
    """int8 AR(1) LD; z = R b with the planted effects, handed over as standardised effects z / sqrt(n)."""
    gdl = ArrayDataLoader.synthetic(CHROM_SIZES, ld_dtype=ld_dtype, n=N, kind="ar1")
    for c, sizes in CHROM_SIZES.items():
        sym = gdl.ld[c].load(return_symmetric=True)
        lb, ip, data = sym.leftmost_idx, sym.ld_indptr, sym.ld_data
        m = int(np.sum(sizes))
        z = np.zeros(m)
        for s, e in zip(np.cumsum([0] + sizes[:-1]), np.cumsum(sizes)):
            b = np.zeros(e - s)
            for j, v in PLANTED[c].items():
                if s <= j < e:
                    b[j - s] = v
            z[s:e] = S.block_matrix(lb, ip, data, False, int(s), int(e), gdl.ld[c].dq_scale) @ b
        n_per_snp = np.full(m, N) * (1.0 + 0.1 * (np.arange(m) % 3))        # (sample sizes that differ from SNP to SNP)
        gdl.sumstats_table[c] = SumstatsArrays(z / np.sqrt(n_per_snp), n_per_snp)
    return gdl


@pytest.mark.parametrize("low_memory", [True, False], ids=["upper", "sym"])
def test_fit_splits_per_chromosome_and_recovers_the_planted_effects(low_memory):
    gdl = loader()
    seen = {}

    def fit_fn(*args):
        seen["args"] = args
        return S.susie_host(*args)

    mdl = SuSiE(gdl, L=4, low_memory=low_memory, dequantize_on_the_fly=True, fit_fn=fit_fn).fit()
    lb, ip, data, lm, z, L, V, est, lp, dq, tol, max_iter, prec = seen["args"]
    assert data.dtype == np.int8 and lm == low_memory and dq == 1.0 / 127 and (L, V, est, lp) == (4, 50.0, True, None)
    assert (tol, max_iter, prec) == (1e-4, 100, "float32") and z.shape == (275,) and lb.shape == (275,)
    assert mdl.info.block_start.tolist() == [0, 120, 185, 275] and mdl.info.converged
    assert {c: v.shape for c, v in mdl.get_posterior_mean_beta().items()} == {1: (185,), 2: (90,)}
    assert {c: v.shape for c, v in mdl.get_pip().items()} == {1: (185,), 2: (90,)}
    assert mdl.post_mean_beta[1].dtype == np.float32 and mdl.pip[1].dtype == np.float64
    for c, eff in PLANTED.items():
        n_j = gdl.sumstats_table[c].n_per_snp
        for j, v in eff.items():
            assert mdl.pip[c][j] > 0.99
            assert mdl.post_mean_beta[c][j] * np.sqrt(n_j[j]) == pytest.approx(v, rel=0.05)
        idle = np.setdiff1d(np.arange(mdl.shapes[c]), list(eff))
        assert np.all(np.abs(mdl.post_mean_beta[c][idle] * np.sqrt(n_j[idle])) < 0.5)
    sets = mdl.credible_sets()
    assert [(cs["chromosome"], cs["index"].tolist()) for cs in sets] == [(1, [20]), (1, [150]), (2, [45])]
    assert [cs["snps"].tolist() for cs in sets] == [[20], [150], [230]]
    assert mdl.elbo().shape == (3,) and np.all(np.isfinite(mdl.elbo()))
    table = mdl.to_table()
    assert list(table.columns) == ["CHR", "IDX", "BETA", "PIP", "CS"] and len(table) == 275
    assert table["CS"].to_numpy().nonzero()[0].tolist() == [20, 150, 230]
    assert table["CS"].to_numpy()[[20, 150, 230]].tolist() == [1, 2, 3]
    per = mdl.to_table(per_chromosome=True)
    assert sorted(per) == [1, 2] and per[2]["CS"].to_numpy()[45] == 3 and np.array_equal(per[2]["PIP"], mdl.pip[2])


def test_a_block_that_stops_at_max_iter_warns():
    gdl = loader()
    mdl = SuSiE(gdl, L=4, dequantize_on_the_fly=True, fit_fn=S.susie_host)
    with pytest.warns(RuntimeWarning, match="Maximum iterations reached"):
        mdl.fit(max_iter=1)
    assert not mdl.info.converged and np.all(mdl.info.iterations == 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mdl.fit()
    assert mdl.info.converged


def test_prior_weights():
    gdl = loader()
    w = {1: np.ones(185), 2: np.ones(90)}
    w[1][20] = 0.0                                              # the planted SNP is excluded: its neighbours take the effect
    w[2][:45] = 3.0
    mdl = SuSiE(gdl, L=4, prior_weights=w, dequantize_on_the_fly=True, fit_fn=S.susie_host).fit()
    lp = mdl.log_prior
    assert lp[20] == -np.inf and lp[0] == pytest.approx(-np.log(119.0))
    assert lp[185] == pytest.approx(np.log(3.0 / (45 * 3 + 45))) and lp[185 + 45] == pytest.approx(np.log(1.0 / 180))
    for s, e in ((0, 120), (120, 185), (185, 275)):
        assert np.exp(lp[s:e]).sum() == pytest.approx(1.0)
    assert mdl.pip[1][20] == 0.0 and np.all(mdl.info.alpha[20] == 0.0)
    assert max(mdl.pip[1][19], mdl.pip[1][21]) > 0.3 and mdl.pip[1][150] > 0.99
    flat = SuSiE(gdl, L=4, prior_weights=np.concatenate([w[1], w[2]]), dequantize_on_the_fly=True, fit_fn=S.susie_host)
    assert np.array_equal(flat.log_prior, lp)
    for bad, word in ((np.ones(10), "expected 275"), (-np.ones(275), "finite and >= 0"),
                      (np.concatenate([np.zeros(120), np.ones(155)]), "zero for every SNP")):
        with pytest.raises(ValueError, match=word):
            SuSiE(gdl, prior_weights=bad, fit_fn=S.susie_host)


def test_an_unfitted_model_and_a_missing_device_raise():
    from viprs_amd import _lib
    mdl = SuSiE(loader(), fit_fn=S.susie_host)
    for call in (mdl.credible_sets, mdl.elbo, mdl.to_table):
        with pytest.raises(Exception, match="not fitted"):
            call()
    if _lib.device_count() < 1:                                 # (no quiet fall-back to the host fit)
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            SuSiE(loader())
