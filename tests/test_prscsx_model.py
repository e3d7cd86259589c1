"""CPU: the model layer of `PRSCSx` on its host backend (the C replay of the Gibbs sweep as `sweep_fn`, `viprs_amd.stats.csx`
for the coupled update): one population is `PRSCS` bit for bit, SNP matching with partial overlap, exchanged and mismatched
alleles, the divergence rule across populations, the results, the refusals, and a simulation in which the small population
gains from the large one."""
import functools

import numpy as np
import pytest

from tests import gibbs_replay as GR
from viprs_amd.model import PRSCS, PRSCSx
from viprs_amd.model.PRSCSx import match_snps

f32 = np.float32
KW = dict(n_iter=24, n_burnin=8, thin=2, dequantize_on_the_fly=True)


def _table(gdl, prefix="rs", a1="A", a2="G"):
    gdl.snp_table = {c: {"SNP": np.array([f"{prefix}{c}_{j}" for j in range(m)]), "A1": np.array([a1] * m),
                         "A2": np.array([a2] * m)} for c, m in gdl.shapes.items()}
    return gdl


def _B(beta_by_chrom):
    return np.concatenate([beta_by_chrom[c] for c in sorted(beta_by_chrom)])


def _second(n=2e4, chroms=None, noise=77):
    """A second population on the LD of the first: the same simulated effects, an independent noise draw, a smaller sample."""
    from viprs_amd.data import SumstatsArrays
    gdl = _table(GR.model_gdl(chroms=chroms, n=n))
    rng = np.random.default_rng(noise)
    for c, s in gdl.sumstats_table.items():
        b = np.asarray(s.get_snp_pseudo_corr(), dtype=np.float64)
        gdl.sumstats_table[c] = SumstatsArrays((b + rng.standard_normal(b.shape[0]) / np.sqrt(n)).astype(f32), s.n_per_snp)
    return gdl


@functools.lru_cache(maxsize=None)
def two(phi=(1e-2, None), seed=3):
    return PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": _second()}, phi=list(phi), seed=seed, sweep_fn=GR.replay_sweep,
                  **KW).fit()


def test_one_population_is_prscs_bit_for_bit():
    phi = [1e-2, None, 1.0]
    ref = PRSCS(GR.model_gdl(), phi=phi, seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    for gdl in (GR.model_gdl(), _table(GR.model_gdl())):              # without and with a SNP table
        x = PRSCSx({"EUR": gdl}, phi=phi, seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
        assert np.array_equal(_B(x.post_mean_beta["EUR"]).view(np.uint32), _B(ref.post_mean_beta).view(np.uint32))
        assert np.array_equal(x.phi_history, ref.phi_history) and np.array_equal(x.sigma2_history["EUR"], ref.sigma2_history)
        assert np.array_equal(x.phi_est, ref.phi_est) and np.array_equal(x.sigma2_est["EUR"], ref.sigma2_est)
        assert x.n_capped_total == 0 and x.m_union == 395 and np.array_equal(x.row_of, np.arange(395)[None, :])
    one = PRSCSx({"EUR": GR.model_gdl()}, phi=None, seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    assert {c: b.shape for c, b in one.post_mean_beta["EUR"].items()} == {1: (194,), 2: (201,)}
    assert list(one.to_table("EUR").columns) == ["CHR", "IDX", "BETA"] and one.meta_beta().shape == (395,)


def test_layout_results_and_coupling():
    x = two()
    assert x.populations == ["EUR", "EAS"] and x.m_union == 395 and x.n_models == 2 and x.n_capped_total == 0
    for name in x.populations:
        assert {c: b.shape for c, b in x.post_mean_beta[name].items()} == {1: (194, 2), 2: (201, 2)}
        assert all(b.dtype == f32 and np.all(np.isfinite(b)) for b in x.post_mean_beta[name].values())
        assert x.sigma2_history[name].shape == (24, 2) and np.all((x.sigma2_history[name] > 0.2) & (x.sigma2_history[name] < 5))
        assert np.array_equal(x.sigma2_est[name], x.sigma2_history[name][8:].mean(axis=0))
        assert list(x.to_table(name).columns) == ["CHR", "IDX", "BETA_0", "BETA_1"]
    assert list(x.grid_table.columns) == ["phi", "auto", "phi_est", "sigma2_est_EUR", "sigma2_est_EAS", "diverged"]
    assert np.all(x.phi_history[:, 0] == 1e-2) and len(np.unique(x.phi_history[:, 1])) == 24
    # the populations do not share their Gibbs draws, and the coupling changes the fit of each
    alone = PRSCS(GR.model_gdl(), phi=[1e-2, None], seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    assert not np.array_equal(_B(x.post_mean_beta["EUR"]), _B(alone.post_mean_beta))
    assert not np.array_equal(_B(x.post_mean_beta["EUR"]), _B(x.post_mean_beta["EAS"]))
    # same seed, same bits; another seed, another result
    y = PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": _second()}, phi=[1e-2, None], seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    assert all(np.array_equal(_B(x.post_mean_beta[k]).view(np.uint32), _B(y.post_mean_beta[k]).view(np.uint32)) for k in x.populations)
    assert not np.array_equal(_B(two(seed=4).post_mean_beta["EAS"]), _B(x.post_mean_beta["EAS"]))
    # meta_beta: between the two posterior means where both carry the SNP (one allele coding here)
    meta, a, b = x.meta_beta(), _B(x.post_mean_beta["EUR"]).astype(np.float64), _B(x.post_mean_beta["EAS"]).astype(np.float64)
    assert meta.shape == (395, 2) and np.all(meta >= np.minimum(a, b) - 1e-12) and np.all(meta <= np.maximum(a, b) + 1e-12)
    with pytest.raises(KeyError):
        x.to_table("AFR")


def test_partial_overlap_and_the_union_order():
    """The second population carries chromosome 1 only, and one SNP of its own in place of a shared one."""
    small = _second(chroms={1: GR.MODEL_CHROMS[1]})
    t = small.snp_table[1]
    t["SNP"] = t["SNP"].copy()
    t["SNP"][5] = "rs1_zz"
    row_of, flip, union = match_snps([_table(GR.model_gdl()).snp_table, small.snp_table], [{1: 194, 2: 201}, {1: 194}])
    assert row_of.shape == (2, 396) and not flip[0].any() and not flip[1].any()
    assert np.array_equal(row_of[0, :194], np.arange(194)) and row_of[0, 194] == -1 and np.array_equal(row_of[0, 195:], np.arange(194, 395))
    want = np.arange(194)
    want[5] = -1
    assert np.array_equal(row_of[1, :194], want) and row_of[1, 194] == 5 and np.all(row_of[1, 195:] == -1)
    assert union[194] == (1, "rs1_zz") and union[0] == (1, "rs1_0") and union[195] == (2, "rs2_0")
    x = PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": small}, phi=1e-2, seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    assert x.m_union == 396 and {c: b.shape for c, b in x.post_mean_beta["EAS"].items()} == {1: (194,)}
    assert x.meta_beta().shape == (396,) and x.n_capped_total == 0
    assert np.isclose(x.meta_beta()[194], x.post_mean_beta["EAS"][1][5], rtol=1e-12)   # carried by one population: its own mean


def test_exchanged_alleles_are_negated_for_the_fit_and_restored():
    flipped = _second()
    mask = {c: np.zeros(m, dtype=bool) for c, m in flipped.shapes.items()}
    mask[1][[0, 7, 100]] = mask[2][[3, 200]] = True
    from viprs_amd.data import SumstatsArrays
    for c, s in flipped.sumstats_table.items():
        b = np.asarray(s.get_snp_pseudo_corr())
        flipped.sumstats_table[c] = SumstatsArrays(np.where(mask[c], -b, b).astype(f32), s.n_per_snp)
        t = flipped.snp_table[c]
        t["A1"], t["A2"] = np.where(mask[c], "G", "A"), np.where(mask[c], "A", "G")
    x = PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": flipped}, phi=[1e-2, None], seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    ref = two()
    assert np.array_equal(_B(x.post_mean_beta["EUR"]), _B(ref.post_mean_beta["EUR"]))
    m = np.concatenate([mask[1], mask[2]])
    got, want = _B(x.post_mean_beta["EAS"]), _B(ref.post_mean_beta["EAS"])
    assert np.array_equal(got, np.where(m[:, None], -want, want)) and np.any(want[m] != 0)
    assert np.array_equal(x.meta_beta(), ref.meta_beta())            # in the coding of the first population


def test_an_allele_mismatch_raises_and_names_the_snp():
    bad = _second()
    bad.snp_table[2]["A2"] = bad.snp_table[2]["A2"].copy()
    bad.snp_table[2]["A2"][17] = "T"
    with pytest.raises(ValueError, match="rs2_17"):
        PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": bad}, sweep_fn=GR.replay_sweep, **KW)
    with pytest.raises(ValueError, match="snp_table"):
        PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": GR.model_gdl()}, sweep_fn=GR.replay_sweep, **KW)


def test_a_chain_that_diverges_in_one_population_is_dropped_in_all():
    calls, widths = [], []

    def sweep_fn(lb, ip, data, low_memory, std_beta, mu_mult, hvt, u_logs, unif, noise, eta, q, dq_scale):
        calls.append(eta.shape[1])
        out = GR.replay_sweep(lb, ip, data, low_memory, std_beta, mu_mult, hvt, u_logs, unif, noise, eta, q, dq_scale)
        if len(calls) == 14:                                         # the 7th sweep of the second population
            eta[3, 1] = 10.0
        return out

    x = PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": _second()}, phi=[1e-2, None, 1.0], seed=3, sweep_fn=sweep_fn, **KW).fit()
    assert x.grid_table["diverged"].tolist() == [False, True, False] and np.isnan(x.phi_est[1])
    assert calls == [3] * 14 + [2] * 34
    for name in x.populations:
        B = _B(x.post_mean_beta[name])
        assert not B[:, 1].any() and B[:, [0, 2]].any(axis=0).all() and np.all(np.isfinite(B))
        assert np.isnan(x.sigma2_history[name][6:, 1]).all() and np.isnan(x.sigma2_est[name][1])
    ref = PRSCSx({"EUR": _table(GR.model_gdl()), "EAS": _second()}, phi=[1e-2, None, 1.0], seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    assert np.array_equal(_B(x.post_mean_beta["EUR"])[:, [0, 2]], _B(ref.post_mean_beta["EUR"])[:, [0, 2]])


def test_coupled_fn_replays_a_logged_fit():
    """The logged (psi, delta) of every update, fed back through `coupled_fn`, reproduce the fit."""
    kw = dict(phi=[1e-2, None], seed=3, sweep_fn=GR.replay_sweep, **KW)
    gdls = lambda: {"EUR": _table(GR.model_gdl()), "EAS": _second()}
    a = PRSCSx(gdls(), keep_draws_log=True, **kw).fit()
    assert len(a.coupled_log) == 24 and a.coupled_log[0][0].shape == (395, 2)
    b = PRSCSx(gdls(), coupled_fn=lambda it, cols: a.coupled_log[it], **kw).fit()
    for name in a.populations:
        assert np.array_equal(_B(a.post_mean_beta[name]).view(np.uint32), _B(b.post_mean_beta[name]).view(np.uint32))


def test_refusals():
    gdl = _table(GR.model_gdl())

    class TwoRanks:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="world_size"):
        PRSCSx({"EUR": gdl}, sweep_fn=GR.replay_sweep, comm=TwoRanks())
    for kw in (dict(a=1.5), dict(b=1.0)):
        with pytest.raises(NotImplementedError, match="a = 1, b = 0.5"):
            PRSCSx({"EUR": gdl}, sweep_fn=GR.replay_sweep, **kw)
    for kw in (dict(phi=0.0), dict(phi=[]), dict(float_precision="float64"), dict(n_iter=10, n_burnin=10), dict(thin=0),
               dict(psi_max=0.0)):
        with pytest.raises(ValueError):
            PRSCSx({"EUR": gdl}, sweep_fn=GR.replay_sweep, **kw)
    for gdls in ({}, gdl, {k: gdl for k in range(9)}):
        with pytest.raises(ValueError, match="gdls"):
            PRSCSx(gdls, sweep_fn=GR.replay_sweep)
    from viprs_amd import _lib
    if _lib.device_count() < 1:
        with pytest.raises(RuntimeError, match="HIP device"):
            PRSCSx({"EUR": gdl})


def simulate(seed, n_large=5e4, n_small=5e3, h2=0.05, pi=0.02):
    """Two populations, 600 SNPs in three AR(1) blocks with population-specific correlations, the same causal effects, a
    large and a small GWAS; returns (correlation of the small population's PRS-CSx posterior mean with the simulated
    effects, the same for PRS-CS on the small population alone).  `h2`, `pi`: about 12 causal SNPs of h2 / 12 each, a
    z-score near sqrt(5 000 * 0.05 / 12) = 4.6 in the small GWAS and 14 in the large one -- the case the model is for:
    effects the large GWAS sees clearly and the small one does not.  (`make_sumstats`' defaults, h2 = 0.2 over 6 SNPs,
    put every causal SNP at z = 13 in the SMALL GWAS: nothing is left to borrow, and the coupled fit then loses about 0.05
    of correlation against the fit alone in each of five seeds -- EXPERIMENTS.md.)"""
    from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
    from viprs_amd.utils import synthetic as syn

    def loader(ld_seed, n, noise_seed):
        ld = syn.make_ld([250, 200, 150], low_memory=False, seed=ld_seed)
        ss = syn.make_sumstats(ld, n=n, seed=seed, noise_seed=noise_seed, h2=h2, pi=pi)
        gdl = ArrayDataLoader({1: LDArrays(symmetric=(ld.ld_left_bound, ld.ld_indptr, ld.ld_data), upper=None,
                                           stored_dtype=np.float32, dq_scale=ld.dq_scale, sample_size=None)},
                              {1: SumstatsArrays(ss.std_beta, ss.n_per_snp)}, n=ss.n)
        return _table(gdl), ss
    big, _ = loader(seed, n_large, None)
    small, ss = loader(seed + 100, n_small, seed + 1)
    kw = dict(phi=None, n_iter=150, n_burnin=50, thin=2, seed=1, low_memory=False, sweep_fn=GR.replay_sweep)
    joint = PRSCSx({"large": big, "small": small}, **kw).fit()
    alone = PRSCS(small, **kw).fit()
    r = lambda b: float(np.corrcoef(np.asarray(b, dtype=np.float64), ss.beta_true)[0, 1])
    return r(joint.post_mean_beta["small"][1]), r(alone.post_mean_beta[1])


def test_the_small_population_gains_from_the_large_one():
    """Seed 1 of five (1 .. 5, all of which agree; EXPERIMENTS.md lists the margins): the posterior mean of the small
    population (n = 5 000) correlates with the simulated effects more when it is fitted together with the large one
    (n = 50 000) than in a PRS-CS fit of its own."""
    joint, alone = simulate(1)
    print(f"correlation with the simulated effects, small population: PRS-CSx {joint:.3f}, PRS-CS alone {alone:.3f}")
    assert joint > alone
