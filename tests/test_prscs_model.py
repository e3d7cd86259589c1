"""CPU: the model layer of `PRSCS` on its host backend (the C replay of the Gibbs sweep as `sweep_fn`, `viprs_amd.stats.cs` for
the rest): layout and table, the seed, chains that do not depend on the other entries of `phi`, a forced-divergent chain,
the refusals, and a sanity condition on accuracy."""
import functools

import numpy as np
import pytest

from tests import gibbs_replay as GR
from viprs_amd.model import PRSCS
from viprs_amd.stats import gibbs as GB

f32 = np.float32
KW = dict(n_iter=24, n_burnin=8, thin=2, dequantize_on_the_fly=True)


def _B(model):
    return np.concatenate([model.post_mean_beta[c] for c in (1, 2)])


@functools.lru_cache(maxsize=None)
def fit(phi=(1e-2, None, 1.0), seed=3, sweep="c"):
    return PRSCS(GR.model_gdl(), phi=list(phi), seed=seed, sweep_fn=GR.replay_sweep if sweep == "c" else GB.gibbs_sweep_host,
                 **KW).fit()


def test_layout_and_table():
    model = fit()
    assert model.n_models == 3 and {c: b.shape for c, b in model.post_mean_beta.items()} == {1: (194, 3), 2: (201, 3)}
    assert all(b.dtype == f32 for b in model.post_mean_beta.values()) and model.best_model_idx is None
    t = model.grid_table
    assert list(t.columns) == ["phi", "auto", "phi_est", "sigma2_est", "diverged"]
    assert t["auto"].tolist() == [False, True, False] and not t["diverged"].any()
    assert t["phi"][0] == 1e-2 and np.isnan(t["phi"][1]) and t["phi"][2] == 1.0
    assert model.phi_history.shape == model.sigma2_history.shape == (24, 3)
    assert np.all(model.phi_history[:, 0] == 1e-2) and np.all(model.phi_history[:, 2] == 1.0)
    assert len(np.unique(model.phi_history[:, 1])) == 24 and np.all(model.phi_history[:, 1] > 0)       # the auto chain samples it
    assert np.all((model.sigma2_history > 0.3) & (model.sigma2_history < 3))
    assert np.array_equal(model.phi_est, model.phi_history[8:].mean(axis=0))
    B = _B(model)
    assert np.all(np.isfinite(B)) and B.any(axis=0).all()
    # the Rao-Blackwellised mean shrinks the marginal effects: correlated with them, smaller than them
    b = np.concatenate([model.std_beta[c] for c in (1, 2)]).astype(np.float64)
    for g in range(3):
        x = B[:, g].astype(np.float64)
        assert np.corrcoef(x, b)[0, 1] > 0.5 and x @ x < b @ b
    # the host definition of the sweep and its C replay give one fit
    assert np.array_equal(_B(fit(sweep="host")), B)


def test_one_chain_is_a_vector():
    model = fit(phi=(None,))
    assert {c: b.shape for c, b in model.post_mean_beta.items()} == {1: (194,), 2: (201,)} and model.best_model_idx == 0
    assert list(model.to_table().columns) == ["CHR", "IDX", "BETA"]
    scalar = PRSCS(GR.model_gdl(), phi=None, seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    assert np.array_equal(_B(scalar), _B(model))


def test_same_seed_same_bits_other_seed_other_result():
    a = fit()
    b = PRSCS(GR.model_gdl(), phi=[1e-2, None, 1.0], seed=3, sweep_fn=GR.replay_sweep, **KW).fit()
    assert np.array_equal(_B(a).view(np.uint32), _B(b).view(np.uint32)) and a.grid_table.equals(b.grid_table)
    assert np.array_equal(a.phi_history, b.phi_history) and np.array_equal(a.sigma2_history, b.sigma2_history)
    c = fit(seed=4)
    assert not np.array_equal(_B(c)[:, 0], _B(a)[:, 0]) and not np.array_equal(c.sigma2_history, a.sigma2_history)


def test_a_chain_does_not_depend_on_the_other_entries():
    a, b = fit(), fit(phi=(1e-2, 0.5, None))
    assert np.array_equal(_B(a)[:, 0], _B(b)[:, 0]) and np.array_equal(a.sigma2_history[:, 0], b.sigma2_history[:, 0])
    assert not np.array_equal(_B(a)[:, 1], _B(b)[:, 1])
    alone = fit(phi=(1e-2,))
    assert np.array_equal(_B(alone), _B(a)[:, 0])


def test_forced_divergent_chain_is_dropped_and_reported_as_zero():
    """Chain 1's sum eta^2 exceeds sum beta_hat^2 in the 7th sweep: diverged, zero, out of the sweeps and of the updates
    from there on; the others are what they are without it."""
    widths = []

    def sweep_fn(lb, ip, data, low_memory, std_beta, mu_mult, hvt, u_logs, unif, noise, eta, q, dq_scale):
        widths.append(eta.shape[1])
        out = GR.replay_sweep(lb, ip, data, low_memory, std_beta, mu_mult, hvt, u_logs, unif, noise, eta, q, dq_scale)
        if len(widths) == 7:
            eta[3, 1] = 10.0
        return out

    model = PRSCS(GR.model_gdl(), phi=[1e-2, None, 1.0], seed=3, sweep_fn=sweep_fn, **KW).fit()
    t = model.grid_table
    assert t["diverged"].tolist() == [False, True, False] and np.isnan(t["phi_est"][1])
    B = _B(model)
    assert not B[:, 1].any() and np.all(np.isfinite(B))
    assert widths == [3] * 7 + [2] * 17
    assert np.isnan(model.phi_history[6:, 1]).all() and np.isfinite(model.phi_history[:6, 1]).all()
    assert np.array_equal(B[:, [0, 2]], _B(fit())[:, [0, 2]])

    def nan_fn(*a):
        out = GR.replay_sweep(*a)
        a[10][0, 0] = np.nan
        return out
    model = PRSCS(GR.model_gdl(), phi=0.1, n_iter=3, n_burnin=1, thin=1, dequantize_on_the_fly=True, sweep_fn=nan_fn).fit()
    assert model.grid_table["diverged"].tolist() == [True] and not _B(model).any()


def test_refusals():
    gdl = GR.model_gdl()

    class TwoRanks:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="world_size"):
        PRSCS(gdl, sweep_fn=GR.replay_sweep, comm=TwoRanks())
    for kw in (dict(a=1.5), dict(b=1.0), dict(a=0.5, b=0.5)):
        with pytest.raises(NotImplementedError, match="a = 1, b = 0.5"):
            PRSCS(gdl, sweep_fn=GR.replay_sweep, **kw)
    for kw in (dict(phi=0.0), dict(phi=[1e-2, -1.0]), dict(phi=[]), dict(phi=np.inf), dict(float_precision="float64"),
               dict(n_iter=10, n_burnin=10), dict(thin=0), dict(n_iter=12, n_burnin=10, thin=5), dict(psi_max=0.0),
               dict(psi_max=np.inf)):
        with pytest.raises(ValueError):
            PRSCS(gdl, sweep_fn=GR.replay_sweep, **kw)
    from viprs_amd import _lib
    if _lib.device_count() < 1:
        with pytest.raises(RuntimeError, match="HIP device"):
            PRSCS(gdl)


def test_the_auto_chain_beats_the_marginal_effects():
    """750 SNPs in three AR(1) blocks, 8 causal effects (synthetic.make_problem, seed 2): the posterior mean of the auto
    chain correlates with the simulated effects better than the marginal effects do -- 0.93 against 0.74 when this was
    written; seeds 1 to 6 all gave a margin of 0.19 or more."""
    from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
    from viprs_amd.utils import synthetic as syn
    ld, ss, _ = syn.make_problem(sizes=[300, 250, 200], low_memory=False, seed=2)
    gdl = ArrayDataLoader({1: LDArrays(symmetric=(ld.ld_left_bound, ld.ld_indptr, ld.ld_data), upper=None, stored_dtype=np.float32,
                                       dq_scale=ld.dq_scale, sample_size=None)}, {1: SumstatsArrays(ss.std_beta, ss.n_per_snp)},
                          n=ss.n)
    model = PRSCS(gdl, phi=None, n_iter=150, n_burnin=50, thin=2, seed=1, low_memory=False, sweep_fn=GR.replay_sweep).fit()
    b = model.post_mean_beta[1].astype(np.float64)
    r_fit, r_marginal = np.corrcoef(b, ss.beta_true)[0, 1], np.corrcoef(ss.std_beta.astype(np.float64), ss.beta_true)[0, 1]
    print(f"correlation with the simulated effects: PRS-CS-auto {r_fit:.3f}, marginal {r_marginal:.3f}")
    assert r_fit > r_marginal + 0.1 and 0 < model.phi_est[0] < 0.1 and 0.5 < model.sigma2_est[0] < 1.5
