"""CPU: the model layer of `SBayesR` on its host backend (`viprs_amd.stats.bayesr.bayesr_sweep_host`, or the C replay of the
same definition where many sweeps run) on three small chromosomes: determinism, chains that do not depend on their number,
a forced-divergent chain, pi on the simplex, layout, `to_table` and `predict()`, and the accuracy beside `LDpred2(mode="auto")`."""
import functools

import numpy as np

from tests import bayesr_replay as R
from tests import gibbs_replay as GR
from viprs_amd.model import LDpred2, SBayesR
from viprs_amd.stats import bayesr as B
from viprs_amd.utils import synthetic as syn

CHROMS = sorted(R.MODEL_CHROMS)
# The accuracy test.  Correlation of the posterior mean with the simulated effects, measured on this data (3 chromosomes,
# 491 SNPs, n = 5e4, h2 = 0.5, int8 longrange LD) for loader seeds 101 .. 105 -- SBayesR (400 sweeps, 100 of them burn-in, one
# chain) / LDpred2-auto (5 chains, 100 + 100 sweeps), both on the C replays:
#   0.9998 / 1.0000   0.9992 / 1.0000   0.9999 / 1.0000   0.9998 / 1.0000   0.9930 / 0.9999
# The differences are 0.0002, 0.0008, 0.0001, 0.0002 and 0.0069; the margin is three times the largest of them.
ACCURACY_SEEDS = (101, 102, 103, 104, 105)
ACCURACY_MARGIN = 0.02


def _B(model):
    return np.concatenate([model.post_mean_beta[c] for c in CHROMS])


def _fit(seed=3, sweep="c", **kw):
    args = dict(h2_init=0.3, n_iter=30, n_burnin=10, seed=seed, dequantize_on_the_fly=True)
    args.update(kw)
    if sweep == "c":
        args["sweep_fn"] = R.replay_sweep
    else:
        args["backend"] = "host"
    return SBayesR(R.model_gdl(), **args).fit()


@functools.lru_cache(maxsize=None)
def short_fit(seed=3, sweep="c", n_chains=1):
    return _fit(seed, sweep, n_chains=n_chains)


def test_defaults_and_layout():
    model = SBayesR(R.model_gdl(), h2_init=0.3, backend="host")
    assert model.K == 3 and model.gamma.tolist() == [0.01, 0.1, 1.0] and model.pi_init.tolist() == [0.95, 0.02, 0.02, 0.01]
    assert (model.n_iter, model.n_burnin, model.thin, model.n_chains) == (1000, 250, 1, 1) and model.n_models == 1
    assert SBayesR._ldsc_h2 is LDpred2._ldsc_h2                         # h2_init="ldsc": the LD-score estimate, as LDpred2's
    fit = short_fit()
    assert {c: b.shape for c, b in fit.post_mean_beta.items()} == {1: (194,), 2: (201,), 3: (96,)}
    assert all(b.dtype == np.float32 for b in fit.post_mean_beta.values()) and fit.best_model_idx == 0
    b = np.concatenate([fit.std_beta[c] for c in CHROMS]).astype(np.float64)
    x = _B(fit).astype(np.float64)
    assert np.all(np.isfinite(x)) and np.corrcoef(x, b)[0, 1] > 0.3 and x @ x < b @ b
    pip = np.concatenate([fit.pip[c] for c in CHROMS])
    assert np.all((pip > 0) & (pip <= 1.0 + 1e-6))
    t = fit.to_table()
    assert list(t.columns) == ["CHR", "IDX", "BETA", "PIP"] and len(t) == fit.m
    assert list(fit.grid_table.columns) == ["chain", "diverged", "n_sweeps", "h2", "sigma2_beta", "sigma2_e", "pi_0", "pi_1", "pi_2", "pi_3"]
    for bad in (dict(gamma=(1.0,) * 5, pi=(0.5,) + (0.1,) * 5), dict(pi=(0.9, 0.1)), dict(n_burnin=1000), dict(thin=0),
                dict(float_precision="float64"), dict(backend="cpu")):
        try:
            SBayesR(R.model_gdl(), h2_init=0.3, **dict(dict(backend="host"), **bad))
        except ValueError:
            continue
        raise AssertionError(bad)


def test_determinism_per_seed_and_the_two_host_sweeps_agree():
    a, b = short_fit(3, "host"), _fit(3, "host")
    assert np.array_equal(_B(a), _B(b)) and a.grid_table.equals(b.grid_table)
    assert np.array_equal(_B(a), _B(short_fit(3, "c")))                   # the NumPy definition and its C replay give one fit
    assert not np.array_equal(_B(a), _B(short_fit(4, "c")))


def test_a_chain_does_not_depend_on_the_number_of_chains():
    one, three = short_fit(3, "c", 1), short_fit(3, "c", 3)
    for c in CHROMS:
        assert np.array_equal(one.chain_beta[c][:, 0], three.chain_beta[c][:, 0])
        assert not np.array_equal(three.chain_beta[c][:, 0], three.chain_beta[c][:, 1])
    assert np.array_equal(one.pi_history[0], three.pi_history[0]) and np.array_equal(one.h2_history[0], three.h2_history[0])
    assert three.grid_table.shape[0] == 3 and not three.diverged.any()
    # the result is the mean over the chains
    full = np.concatenate([three.chain_beta[c] for c in CHROMS]).astype(np.float64)
    assert np.allclose(_B(three), full.mean(axis=1), rtol=1e-6, atol=1e-9)


def test_a_diverged_chain_is_reported_and_dropped():
    """Chain 1 gets normals of 1e18 from its third sweep on: sum eta^2 passes sum beta_hat^2, LDpred2's divergence rule."""
    def draws(seed, draw_index, m):
        unif, z = B.bayesr_draws_host(seed, draw_index, m)
        if draw_index >> 32 == 1 and (draw_index & 0xFFFFFFFF) >= 2:
            z = np.full(m, 1e18, dtype=np.float32)
        return unif, z
    bad = _fit(3, "c", n_chains=3, draws_fn=draws)
    assert bad.diverged.tolist() == [False, True, False] and bad.grid_table["diverged"].tolist() == [False, True, False]
    assert np.isnan(bad.h2_est[1]) and np.all(np.isnan(bad.pi_est[1])) and np.all(np.isfinite(bad.pi_est[[0, 2]]))
    good = short_fit(3, "c", 3)
    full = np.concatenate([good.chain_beta[c] for c in CHROMS]).astype(np.float64)
    assert np.all(np.isfinite(_B(bad))) and np.allclose(_B(bad), full[:, [0, 2]].mean(axis=1), rtol=1e-6, atol=1e-9)
    for c in CHROMS:
        assert not bad.chain_beta[c][:, 1].any()


def test_more_snps_than_samples_the_chains_diverge_and_say_so():
    """The limit the class docstring names, on data whose summary statistics are exactly consistent with the LD
    (`make_sumstats`: R beta + N(0, R / n)).  491 SNPs; n = 100 (m / n = 4.9): sigma2_e falls through its floor, pi_0 collapses,
    h2 passes 1 and the divergence rule stops both chains within 10 sweeps; the fit reports them and returns zeros.  n = 1000
    (m / n = 0.49): the same data recipe runs to the end."""
    kw = dict(h2_init=0.3, n_iter=60, n_burnin=20, seed=1, n_chains=2, dequantize_on_the_fly=True, sweep_fn=R.replay_sweep)
    bad = SBayesR(R.model_gdl(n=100, seed=101), **kw).fit()
    assert bad.diverged.all() and np.all(bad.n_sweeps < 10) and bad.grid_table["n_sweeps"].tolist() == bad.n_sweeps.tolist()
    assert not _B(bad).any() and all(not p.any() for p in bad.pip.values())
    for c in range(2):
        k = int(bad.n_sweeps[c]) - 1                         # the last sweep whose hyper-parameters were drawn: one before the stop
        assert bad.h2_history[c][k - 1] > 1.0 and bad.pi_history[c][k - 1][0] < 0.8
    fine = SBayesR(R.model_gdl(n=1000, seed=101), **kw).fit()
    assert not fine.diverged.any() and fine.n_sweeps.tolist() == [60, 60] and _B(fine).any()
    assert np.all(fine.h2_est > 0) and np.all(fine.h2_est < 1)


def test_pi_stays_on_the_simplex():
    fit = short_fit(3, "c", 3)
    for h in fit.pi_history:
        assert h.shape == (30, 4) and np.all(h > 0) and np.allclose(h.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.allclose(fit.pi_est.sum(axis=1), 1.0) and np.all(fit.sigma2_e_est >= B.SIGMA2_E_MIN) and np.all(fit.sigma2_beta_est > 0)


def test_thinning_and_predict():
    thin = _fit(3, "c", thin=5)
    assert not np.array_equal(_B(thin), _B(short_fit())) and np.corrcoef(_B(thin), _B(short_fit()))[0, 1] > 0.9
    # predict(): the scores of genotyped samples are X beta with the model's effects
    from tests import genotype_score_reference as GS
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.io.plink_bed import pack_codes
    model, rng, n = short_fit(), np.random.default_rng(5), 40
    geno = {c: (pack_codes(GS.random_codes(rng, n, model.shapes[c], missing=0.02)), n) for c in CHROMS}
    score = model.predict(test_gdl=ArrayDataLoader({}, {}, n=n, genotype=geno, phenotype=np.zeros(n)))
    assert score.shape == (n,) and np.all(np.isfinite(score)) and score.std() > 0


def _truth(seed, n=5e4):
    mt = float(sum(sum(s) for s in R.MODEL_CHROMS.values()))
    out = []
    for ci, (c, sizes) in enumerate(R.MODEL_CHROMS.items()):
        sym = syn.make_ld(sizes, low_memory=False, ld_dtype=np.int8, seed=seed + ci, kind="longrange")
        out.append(syn.make_sumstats(sym, n=n, seed=seed + ci, h2=R.MODEL_H2 * sum(sizes) / mt).beta_true)
    return np.concatenate(out)


def test_accuracy_beside_ldpred2_auto():
    rows = []
    for seed in ACCURACY_SEEDS:
        truth = _truth(seed)
        sb = SBayesR(R.model_gdl(seed=seed), h2_init=0.3, n_iter=400, n_burnin=100, seed=seed, dequantize_on_the_fly=True,
                     sweep_fn=R.replay_sweep).fit()
        lp = LDpred2(R.model_gdl(seed=seed), mode="auto", n_chains=5, h2_init=0.3, burn_in=100, num_iter=100, seed=seed,
                     dequantize_on_the_fly=True, sweep_fn=GR.replay_sweep).fit()
        assert np.array_equal(np.concatenate([sb.std_beta[c] for c in CHROMS]), np.concatenate([lp.std_beta[c] for c in CHROMS]))
        rows.append((float(np.corrcoef(_B(sb), truth)[0, 1]), float(np.corrcoef(_B(lp), truth)[0, 1])))
        assert not sb.diverged.any()
    print("corr(posterior mean, simulated effects), SBayesR / LDpred2-auto:", "  ".join(f"{a:.4f} / {b:.4f}" for a, b in rows))
    for a, b in rows:
        assert a >= b - ACCURACY_MARGIN, rows
