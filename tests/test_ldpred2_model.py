"""CPU: the model layer of `LDpred2` through the `sweep_fn` hook (`gibbs_sweep_host`, or the C replay of the same definition
where many sweeps run) on two chromosomes: grid and auto fits, layout and `grid_table`, a forced-divergent column, the seed,
`select_best` and `predict()`."""
import copy
import functools

import numpy as np
import pytest

from tests import gibbs_replay as GR
from tests.test_clump_model import _validation_loader
from viprs_amd.model import LDpred2
from viprs_amd.stats import gibbs as GB

f32 = np.float32
GRID_P, GRID_H2 = (0.05, 0.5, 1.0), (0.3,)


def _B(model):
    return np.concatenate([model.post_mean_beta[c] for c in (1, 2)])


@functools.lru_cache(maxsize=None)
def grid_fit(sweep="host", seed=3):
    return LDpred2(GR.model_gdl(), mode="grid", p=GRID_P, h2=GRID_H2, h2_init=0.3, burn_in=5, num_iter=10, seed=seed,
                   dequantize_on_the_fly=True, sweep_fn=GB.gibbs_sweep_host if sweep == "host" else GR.replay_sweep).fit()


@functools.lru_cache(maxsize=None)
def auto_fit(seed=3):
    return LDpred2(GR.model_gdl(), mode="auto", n_chains=4, h2_init=0.3, burn_in=20, num_iter=20, seed=seed,
                   dequantize_on_the_fly=True, sweep_fn=GR.replay_sweep).fit()


def test_grid_layout_and_table():
    model = grid_fit()
    assert model.n_models == 3 and {c: b.shape for c, b in model.post_mean_beta.items()} == {1: (194, 3), 2: (201, 3)}
    assert all(b.dtype == f32 for b in model.post_mean_beta.values())
    t = model.grid_table
    assert list(t.columns) == ["p", "h2", "diverged", "n_nonzero"]
    assert t["p"].tolist() == list(GRID_P) and t["h2"].tolist() == [0.3] * 3 and not t["diverged"].any()
    B = _B(model)
    assert np.all(np.isfinite(B)) and B.any(axis=0).all()
    # p = 1 includes every SNP in every sweep; a sparser prior includes fewer
    nz = t["n_nonzero"].tolist()
    assert nz[2] == model.m and 0 < nz[0] < nz[1] < nz[2]
    # the Rao-Blackwellised mean shrinks the marginal effects: correlated with them, smaller than them
    b = np.concatenate([model.std_beta[c] for c in (1, 2)]).astype(np.float64)
    for g in range(3):
        x = B[:, g].astype(np.float64)
        assert np.corrcoef(x, b)[0, 1] > 0.5 and x @ x < b @ b
    # the host definition and its C replay give one fit
    assert np.array_equal(_B(grid_fit("c")), B)


def test_default_grids():
    model = LDpred2(GR.model_gdl(), h2_init=0.4, dequantize_on_the_fly=True, sweep_fn=GR.replay_sweep)
    assert model.n_models == 68 and model.burn_in == 50 and model.num_iter == 100
    assert np.allclose(model.p, np.exp(np.linspace(np.log(1e-4), 0, 17))) and np.allclose(model.h2, [0.12, 0.28, 0.4, 0.56])
    assert model.chain_p[:17].tolist() == model.p.tolist() and np.all(model.chain_h2[:17] == model.h2[0])
    auto = LDpred2(GR.model_gdl(), mode="auto", h2_init=0.4, dequantize_on_the_fly=True, sweep_fn=GR.replay_sweep)
    assert auto.n_chains == 30 and auto.burn_in == 500 and auto.num_iter == 200 and auto.n_models == 1
    assert np.allclose(auto.chain_p, np.exp(np.linspace(np.log(1e-4), np.log(0.2), 30))) and np.all(auto.chain_h2 == 0.4)


def test_h2_from_ld_scores():
    from viprs_amd.stats.ldsc import simple_ldsc
    gdl = GR.model_gdl()
    for ld in gdl.get_ld_matrices().values():
        ld.sample_size = 5000
    model = LDpred2(gdl, dequantize_on_the_fly=True, sweep_fn=GR.replay_sweep)
    assert model.h2_init > 0 and np.isclose(model.h2_init, simple_ldsc(gdl, ld_scores=model.ld_score))
    assert np.allclose(model.h2, np.array([0.3, 0.7, 1.0, 1.4]) * model.h2_init)


def test_auto_runs_and_reports_its_chains():
    model = auto_fit()
    assert {c: b.shape for c, b in model.post_mean_beta.items()} == {1: (194,), 2: (201,)}
    assert model.p_est.shape == model.h2_est.shape == (4,) and model.p_history.shape == model.h2_history.shape == (40, 4)
    assert np.all(np.isfinite(model.p_history)) and np.all((model.p_est > 0) & (model.p_est <= 1))
    assert np.all(model.h2_est >= 1e-4) and np.all(model.h2_est < 2.0)
    assert np.array_equal(model.p_est, model.p_history[20:].mean(axis=0))
    t = model.grid_table
    assert list(t.columns) == ["p", "h2", "diverged", "n_nonzero", "kept"] and not t["diverged"].any() and t["kept"].any()
    # the MAD filter, from the reported estimates
    med = np.median(model.h2_est)
    mad = 1.4826 * np.median(np.abs(model.h2_est - med))
    assert t["kept"].tolist() == (np.abs(model.h2_est - med) <= 3 * mad).tolist()
    chains = np.concatenate([model.chain_beta[c] for c in (1, 2)]).astype(np.float64)
    # (the chains are stored in float32; the mean is formed from the float64 sums)
    assert np.allclose(_B(model), chains[:, model.chains_kept].mean(axis=1), rtol=1e-5, atol=1e-9)
    # p moved off its initial value: the chains sample it
    assert not np.allclose(model.p_history[-1], model.chain_p)
    prs = model.predict(test_gdl=_validation_loader(model.gdl, grid_fit("c"), planted=1))     # (genotypes of the same SNPs)
    assert prs.shape == (150,) and np.all(np.isfinite(prs)) and prs.std() > 0


def test_same_seed_same_result_other_seed_other_result():
    a, b = grid_fit("c", seed=3), LDpred2(GR.model_gdl(), mode="grid", p=GRID_P, h2=GRID_H2, h2_init=0.3, burn_in=5, num_iter=10,
                                          seed=3, dequantize_on_the_fly=True, sweep_fn=GR.replay_sweep).fit()
    assert np.array_equal(_B(a), _B(b)) and a.grid_table.equals(b.grid_table)
    assert not np.array_equal(_B(grid_fit("c", seed=4))[:, 0], _B(a)[:, 0])
    auto_again = LDpred2(GR.model_gdl(), mode="auto", n_chains=4, h2_init=0.3, burn_in=20, num_iter=20, seed=3,
                         dequantize_on_the_fly=True, sweep_fn=GR.replay_sweep).fit()
    assert np.array_equal(_B(auto_again), _B(auto_fit())) and np.array_equal(auto_again.p_history, auto_fit().p_history)
    assert not np.array_equal(auto_fit(seed=5).p_history, auto_fit().p_history)


def test_forced_divergent_column_is_dropped_and_reported_as_zero():
    """A column whose sum eta^2 exceeds sum beta_hat^2 in the 7th sweep: diverged, zero, out of the sweeps from there on; the
    others are what they are without it."""
    calls = []

    def sweep_fn(lb, ip, data, low_memory, std_beta, mu_mult, hvt, u_logs, unif, noise, eta, q, dq_scale):
        cols = [float(v) for v in u_logs[0]]                     # (the live columns, told apart by their logit)
        calls.extend(cols)
        out = GR.replay_sweep(lb, ip, data, low_memory, std_beta, mu_mult, hvt, u_logs, unif, noise, eta, q, dq_scale)
        if bad in cols and calls.count(bad) == 7:
            eta[3, cols.index(bad)] = 10.0
        return out

    ul = GB.gibbs_prep_host(GR.model_gdl().sumstats_table[1].n_per_snp, 395, GRID_P[1], 0.3)[2]
    bad = float(ul[0])
    model = LDpred2(GR.model_gdl(), mode="grid", p=GRID_P, h2=GRID_H2, h2_init=0.3, burn_in=5, num_iter=10, seed=3,
                    dequantize_on_the_fly=True, sweep_fn=sweep_fn).fit()
    t = model.grid_table
    assert t["diverged"].tolist() == [False, True, False] and t["n_nonzero"][1] == 0
    B = _B(model)
    assert not B[:, 1].any() and np.all(np.isfinite(B))
    assert calls.count(bad) == 7 and len(calls) == 7 + 2 * 15
    assert np.array_equal(B[:, [0, 2]], _B(grid_fit("c"))[:, [0, 2]])
    # not finite is diverged too
    def nan_fn(*a):
        out = GR.replay_sweep(*a)
        a[10][0, 0] = np.nan
        return out
    model = LDpred2(GR.model_gdl(), mode="grid", p=(0.5,), h2=(0.3,), h2_init=0.3, burn_in=1, num_iter=2,
                    dequantize_on_the_fly=True, sweep_fn=nan_fn).fit()
    assert model.grid_table["diverged"].tolist() == [True] and not _B(model).any()


def test_select_best_and_predict():
    model = copy.deepcopy(grid_fit("c"))
    grid = {c: b.copy() for c, b in model.post_mean_beta.items()}
    val = _validation_loader(model.gdl, model, planted=1)
    prs = model.predict(test_gdl=val)
    assert prs.shape == (150, 3) and np.all(np.isfinite(prs))
    assert model.select_best(validation_gdl=val) is model
    r = np.asarray(model.validation_result["Validation_R2"])
    assert r.shape == (3,) and model.best_model_idx == int(np.argmax(r)) == 1 and r[1] > 0.99
    assert all(np.array_equal(model.post_mean_beta[c], grid[c][:, 1]) for c in grid) and model.n_models == 1
    assert model.predict(test_gdl=val).shape == (150,)
    assert list(model.to_table().columns) == ["CHR", "IDX", "BETA"]
    # pseudo-validation against summary statistics of another cohort
    other = copy.deepcopy(grid_fit("c"))
    rng = np.random.default_rng(11)
    vb = {c: np.asarray(b, dtype=np.float64) + 0.002 * rng.normal(size=b.shape[0]) for c, b in other.std_beta.items()}
    other.select_best(validation_gdl=vb, criterion="pseudo_validation")
    r = np.asarray(other.validation_result["Pseudo_Validation_R2"])
    assert r.shape == (3,) and other.best_model_idx == int(np.argmax(r)) and r.max() > 0


def test_refusals():
    gdl = GR.model_gdl()

    class TwoRanks:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="world_size"):
        LDpred2(gdl, h2_init=0.3, sweep_fn=GR.replay_sweep, comm=TwoRanks())
    for kw in (dict(mode="inf"), dict(p=[0.0]), dict(p=[1.5]), dict(h2=[-1.0]), dict(float_precision="float64"),
               dict(num_iter=0), dict(h2_init="mle"), dict(h2_init=-0.1), dict(mode="auto", n_chains=0),
               dict(mode="auto", n_chains=3, p=[0.1, 0.2])):
        with pytest.raises(ValueError):
            LDpred2(gdl, **{"h2_init": 0.3, **kw}, sweep_fn=GR.replay_sweep)
    from viprs_amd import _lib
    if _lib.device_count() < 1:
        with pytest.raises(RuntimeError, match="HIP device"):
            LDpred2(gdl, h2_init=0.3)
