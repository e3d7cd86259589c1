"""`VIPRSGridPathwisePerChromosome`: one PATHWISE grid search per chromosome (the reference CLI's default with --hyp-search GS /
BMA, bin/viprs_fit:238, :885, :501-504), every chromosome's current grid point in lock step on one spike-and-slab state.

Fixtures (tests/golden/make_fitchr_grid_pathwise_golden.py): each chromosome fitted ALONE by the reference,
``VIPRSGrid(sub_loader(c), grid_c).fit(pathwise=True)``.  The target of the lock-step fit is, bit for bit, the serial fit of
this package, ``VIPRSGrid(loader_of_c, grid_c).fit(pathwise=True)`` run once per chromosome; the reference's trajectories
agree at the tolerances of tests/test_per_chromosome.py::check_against_fixture.

CPU: the host logic with the oracle's spike-and-slab kernel through the ``e_step_fn`` hook (a commit is a NumPy column copy).
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_fit import loader_from_fixture
from tests.test_grid_per_chromosome import make_grid, one_chromosome_loader

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["fitchr_grid_pathwise_3chr_upper", "fitchr_grid_pathwise_2chr_sym_lambda", "fitchr_grid_pathwise_f64_lr_int8"]
MAX_ITER = 100


def load(name):
    fx = np.load(os.path.join(HERE, "golden", name + ".npz"))
    gdl = loader_from_fixture(fx)
    for c in gdl.chromosomes:
        if f"emp_lambda_min_{c}" in fx:                 # the LD's get_lambda_min of the fixture's chromosome
            gdl.ld[c]._lambda_min = float(fx[f"emp_lambda_min_{c}"])
    return fx, gdl


def model_kwargs(fx, e_step="oracle"):
    kw = dict(low_memory=bool(fx["low_memory"]), float_precision=str(fx["float_precision"]),
              dequantize_on_the_fly=bool(fx["dequantize_on_the_fly"]))
    if e_step == "oracle":
        kw["e_step_fn"] = O.cpp_e_step
    return kw


def fit(fx, gdl, e_step="oracle", grid=None, max_iter=MAX_ITER, **fit_kw):
    from viprs_amd.model import VIPRSGridPathwisePerChromosome
    model = VIPRSGridPathwisePerChromosome(gdl, grid if grid is not None else make_grid(fx, gdl.m), **model_kwargs(fx, e_step))
    return model.fit(max_iter=max_iter, **fit_kw)


def sequential(model, gdl, fx, e_step="oracle", max_iter=MAX_ITER, **fit_kw):
    """Every chromosome's own serial pathwise grid search, one after the other."""
    from viprs_amd.model import VIPRSGrid
    out = {}
    for c in model.groups:
        g = VIPRSGrid(one_chromosome_loader(gdl, c), model.grids[c], **model_kwargs(fx, e_step))
        kw = dict(fit_kw)
        if isinstance(kw.get("theta_0"), dict) and c in kw["theta_0"]:
            kw["theta_0"] = kw["theta_0"][c]
        if kw.get("theta_0") is not None:
            kw["theta_0"] = dict(kw["theta_0"])
        out[c] = g.fit(pathwise=True, max_iter=max_iter, **kw)
    return out


def check_against_fixture(model, fx):
    for c in (int(c) for c in fx["chroms"]):
        vr = model.validation_result[c]
        np.testing.assert_allclose(vr["sigma_epsilon"], fx[f"grid_sigma_epsilon_{c}"], rtol=1e-12)
        np.testing.assert_allclose(vr["pi"], fx[f"grid_pi_{c}"], rtol=1e-12)
        if f"grid_lambda_min_{c}" in fx:
            np.testing.assert_allclose(vr["lambda_min"], fx[f"grid_lambda_min_{c}"], rtol=1e-12)
        # the whole pathwise trajectory.  The reference forms the ELBO in float32 where this package sums in float64: on a
        # point whose ELBO changes by ~1e-6 the stopping rule may fire one iteration apart, and the points after it start
        # from states one iteration apart (their stopping iterations may then differ more).  The histories agree up to the
        # end of the first such point; after it the fitted points agree at the tolerances below
        nit, ref_nit = np.array([r.nit for r in model.optim_results[c]]), fx[f"nit_{c}"]
        h, ref = np.array(model.history[c]["ELBO"]), fx[f"elbo_history_{c}"]
        if np.array_equal(nit, ref_nit):
            assert len(h) == len(ref)
            k = len(nit) - 1
        else:
            k = int(np.argmax(nit != ref_nit))
            assert abs(int(nit[k]) - int(ref_nit[k])) == 1, (c, nit, ref_nit)
        n = 1 + int(np.sum(ref_nit[:k])) + int(min(nit[k], ref_nit[k]))
        np.testing.assert_allclose(h[:n], ref[:n], rtol=2e-7, atol=0.05)
        np.testing.assert_allclose(model.model_elbos[c], fx[f"elbo_{c}"], rtol=2e-7, atol=0.05)
        assert model.pip[c].shape == fx[f"pip_{c}"].shape == (model.shapes[c], model.n_models)
        # the tolerances of tests/test_grid_per_chromosome.py up to the first moved stop; behind it (a point there ran 14
        # iterations longer than the reference's) single entries sit up to 9e-5 / 2.5 % away
        for cols, atol, rtol in ((slice(0, k + 1), 2e-5, 2e-2), (slice(k + 1, None), 1e-4, 5e-2)):
            np.testing.assert_allclose(model.post_mean_beta[c][:, cols], fx[f"post_mean_beta_{c}"][:, cols], rtol=rtol,
                                       atol=atol)
            ref_pip = fx[f"pip_{c}"][:, cols]
            big = ref_pip > 0.05
            np.testing.assert_allclose(model.pip[c][:, cols][big], ref_pip[big], rtol=rtol)
        np.testing.assert_allclose(np.asarray(model.tau_beta[c], dtype=np.float64), fx[f"tau_beta_{c}"], rtol=2e-2)
        assert list(vr["Converged"]) == list(fx[f"converged_{c}"])


def assert_same_as_sequential(model, seq):
    """The lock-step fit `==` each chromosome's own `VIPRSGrid(...).fit(pathwise=True)`."""
    G = model.n_models
    for c, s in seq.items():
        ha, hb = model.history[c]["ELBO"], s.history["ELBO"]
        assert np.array_equal(ha, hb, equal_nan=True) and [type(v) for v in ha] == [type(v) for v in hb], c
        ra, rb = model.optim_results[c], s.optim_results
        assert [(r.nit, r.success, r.message) for r in ra] == [(r.nit, r.success, r.message) for r in rb], c
        assert np.array_equal(model.model_elbos[c], s.model_elbos) and model.model_elbos[c].dtype == s.model_elbos.dtype
        for name in ("var_gamma", "var_mu", "q", "var_tau", "pip", "post_mean_beta", "post_var_beta"):
            x, y = getattr(model, name)[c], getattr(s, name)[c]
            assert x.shape == y.shape == (model.shapes[c], G) and x.dtype == y.dtype and np.array_equal(x, y), (c, name)
        for name in ("pi", "tau_beta", "sigma_epsilon", "_sigma_g"):
            x, y = getattr(model, name)[c], getattr(s, name)
            assert x.dtype == y.dtype and np.array_equal(x, y), (c, name)
        assert model.validation_result[c].equals(s.validation_result), c


# ---- the fit against the reference and against the serial fits -----------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_lockstep_pathwise_cpu_matches_reference(name):
    fx, gdl = load(name)
    model = fit(fx, gdl)
    check_against_fixture(model, fx)
    # the chromosomes are on different grid points in the same round: their points stop at different iterations
    assert len({tuple(r.nit for r in rs) for rs in model.optim_results.values()}) == len(model.groups)


@pytest.mark.parametrize("name", FIXTURES)
def test_lockstep_pathwise_cpu_equals_sequential_fits(name):
    fx, gdl = load(name)
    model = fit(fx, gdl)
    assert_same_as_sequential(model, sequential(model, gdl, fx))
    for c in model.groups:               # iteration numbers run on across the points: one history entry per iteration + 1
        assert len(model.history[c]["ELBO"]) == 1 + sum(r.nit for r in model.optim_results[c])


def test_theta_0_per_chromosome_and_max_iter_per_point_cpu():
    fx, gdl = load(FIXTURES[0])
    chroms = [int(c) for c in fx["chroms"]]
    theta = {c: {"tau_beta": 5000.0 + 1000.0 * k} for k, c in enumerate(chroms)}
    model = fit(fx, gdl, max_iter=4, theta_0=theta)
    assert all(r.nit <= 4 for rs in model.optim_results.values() for r in rs)
    assert any("Maximum iterations" in r.message for rs in model.optim_results.values() for r in rs)
    assert_same_as_sequential(model, sequential(model, gdl, fx, max_iter=4, theta_0=theta))


# ---- selection and averaging per chromosome -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES[:2])
@pytest.mark.parametrize("criterion", ["ELBO", "pseudo_validation", "bma_softmax", "bma_sum"])
def test_selection_and_bma_per_chromosome_cpu(criterion, name):
    from viprs_amd.model import (bayesian_model_average, bayesian_model_average_per_chromosome, select_best_model,
                                 select_best_model_per_chromosome)
    fx, gdl = load(name)
    model = fit(fx, gdl)
    seq = sequential(model, gdl, fx)
    vb = {c: fx[f"validation_std_beta_{c}"] for c in model.groups}
    if criterion == "ELBO":
        for c in model.groups:
            assert np.array_equal(model.pseudo_validate(vb, chrom=c), seq[c].pseudo_validate({c: vb[c]}))
            np.testing.assert_allclose(model.pseudo_validate(vb, chrom=c), fx[f"pseudo_r2_{c}"], rtol=1e-2)
    if criterion.startswith("bma"):
        refs = {c: bayesian_model_average(s, normalization=criterion[4:]) for c, s in seq.items()}
        out = bayesian_model_average_per_chromosome(model, normalization=criterion[4:])
    else:
        refs = {c: select_best_model(s, {c: vb[c]}, criterion=criterion) for c, s in seq.items()}
        out = select_best_model_per_chromosome(model, vb, criterion=criterion)
    assert out.n_models == 1
    for c, ref in refs.items():
        if criterion.startswith("bma"):
            assert np.array_equal(out.model_weights[c], ref.model_weights)
        else:
            assert out.best_model_idx[c] == ref.best_model_idx
        for nm in ("pip", "post_mean_beta", "post_var_beta", "var_gamma", "var_mu", "var_tau", "q"):
            x, y = getattr(out, nm)[c], getattr(ref, nm)[c]
            assert x.shape == (model.shapes[c],) and np.array_equal(x, y), (c, nm)
        for nm in ("pi", "tau_beta", "sigma_epsilon", "_sigma_g"):
            assert np.float64(getattr(out, nm)[c]) == np.float64(getattr(ref, nm)), (c, nm)


# ---- a restart (VIPRS.py:1025-1037) of one chromosome ---------------------------------------------------------------------
def restart_case():
    """One chromosome's marginal effects blown up (test_per_chromosome.py), a pi-only grid: sigma_epsilon is free, the MSE
    of that chromosome turns negative."""
    from viprs_amd.data import ArrayDataLoader, SumstatsArrays
    from viprs_amd.model import HyperparameterGrid
    fx, gdl = load(FIXTURES[0])
    bad = int(fx["chroms"][1])
    ss = dict(gdl.sumstats_table)
    ss[bad] = SumstatsArrays(ss[bad].get_snp_pseudo_corr() * np.float32(5.0), ss[bad].n_per_snp)
    gdl = ArrayDataLoader(gdl.ld, ss)
    return fx, gdl, bad, HyperparameterGrid(n_snps=gdl.m, pi_steps=3)


def check_restart(model, seq, bad):
    assert seq[bad].fix_params.get("sigma_epsilon") == 0.95, "the test input no longer triggers the restart"
    for c, s in seq.items():
        assert (s.fix_params.get("sigma_epsilon") == 0.95) == (c == bad)
    assert_same_as_sequential(model, seq)
    assert np.all(model.sigma_epsilon[bad] == np.float32(0.95))


def test_negative_mse_restarts_only_that_chromosome_cpu():
    fx, gdl, bad, grid = restart_case()
    theta = {"sigma_epsilon": 0.8}
    model = fit(fx, gdl, grid=grid, max_iter=40, theta_0=theta)
    check_restart(model, sequential(model, gdl, fx, max_iter=40, theta_0=theta), bad)


# ---- LockstepEM: one iteration number per model, the move to a new grid point ---------------------------------------------
def _em(T=np.float32, G=3):
    from viprs_amd.model._lockstep import LockstepEM
    th = [dict(pi=T(0.01), sigma_epsilon=T(0.8), tau_beta=np.float64(200.0 + g), lam=T(0.0), fixed={"sigma_epsilon"})
          for g in range(G)]
    return LockstepEM(np.dtype(T), th, np.array([100, 120, 140]), np.array([1e4, 2e4, 3e4]), min_iter=3, patience=1)


def _sums(G, k):
    rng = np.random.default_rng(k)
    s = np.abs(rng.normal(size=(G, 11))) + 0.1
    s[:, 0] = 0.02
    s[:, 3] = 0.05
    s[:, 10] = 1e-3
    return s


def test_lockstep_iteration_array_equals_scalar():
    a, b = _em(), _em()
    idx = np.arange(3)
    for i in range(1, 7):
        s = _sums(3, i)
        assert np.array_equal(a.update(idx, s, i), b.update(idx, s, np.full(3, i)))
        assert np.array_equal(a.elbos, b.elbos) and np.array_equal(a.plateau_n, b.plateau_n)
    # per model: model 2 on iteration 2 of its history (min_iter not yet passed), the others late
    c = _em()
    c.update(idx, _sums(3, 1), np.array([10, 10, 2]))
    s = _sums(3, 2)
    s[:, 10] = 1e-9                       # max |eta_diff| below x_abs_tol: converged, but only after min_iter
    code = c.update(idx, s, np.array([11, 11, 3]))
    assert list(code[:2]) == [6, 6] and code[2] == 0


def test_lockstep_advance():
    from viprs_amd.model._lockstep import f64
    em = _em()
    idx = np.arange(3)
    em.update(idx, _sums(3, 1), 1)
    tau, sig_g = em.tau.copy(), em.sigma_g.copy()
    old = em.results[1]
    e0 = em.advance(1, {"pi": 0.05, "lambda_min": 0.25})
    assert em.results[1] is not old and old.nit == 1
    assert em.results[1].nit == 0 and em.results[1].fun == e0 and not em.results[1].stop_iteration
    assert em.prev_elbo[1] == e0 and em.prev_sigma_g[1] == sig_g[1]
    assert em.pi[1] == np.float32(0.05) and em.fx_pi[1] and em.fx_sig[1] and not em.fx_tau[1]
    assert em.lam1[1] == float(1.0 + np.float32(0.25))
    assert em.tau[1] == tau[1] and not em.tau_is32[1]          # not on the grid: value and dtype carry over
    pi, sig, tau1 = em.theta(1)
    assert type(sig) is np.float32 and type(tau1) is f64 and pi == np.float32(0.05)
    # the starting ELBO: the new point over the sums of the last iteration
    ref = _em()
    ref.update(idx, _sums(3, 1), 1)
    ref.pi[1], ref.fx_pi[1] = np.float32(0.05), True
    assert e0 == float(ref._elbo(np.array([1]), _sums(3, 1)[1:2])[0])
    # a fixed tau_beta is cast to the state precision and stays fixed; the streaks start again and count nothing on the
    # point's first iteration (a fresh ConditionStreak of a continued fit)
    em.plateau_n[:] = em.dropping_n[:] = 5
    em.advance(2, {"tau_beta": 300.0, "sigma_epsilon": 0.7})
    assert em.tau_is32[2] and em.fx_tau[2] and em.sig[2] == np.float32(0.7) and em.plateau_n[2] == em.dropping_n[2] == 0
    s = _sums(3, 2)
    s[2, 5] += 1e6                        # the ELBO drops far below the starting one
    em.update(idx, s, np.array([2, 2, 3]))
    assert em.dropping_n[2] == 0
    em.update(idx, s, np.array([3, 3, 4]))
    assert em.dropping_n[2] <= 1


def test_finish_subset():
    em = _em()
    em.update(np.arange(3), _sums(3, 1), 1)
    em.finish([1])
    assert em.results[1].stop_iteration and "Maximum iterations" in em.results[1].message
    assert not em.results[0].stop_iteration and not em.results[2].stop_iteration


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_cpu():
    from viprs_amd.model import HyperparameterGrid, VIPRSGridPathwisePerChromosome
    from viprs_amd.parallel import LocalComm
    fx, gdl = load(FIXTURES[0])
    model = VIPRSGridPathwisePerChromosome(gdl, make_grid(fx, gdl.m), **model_kwargs(fx))
    with pytest.raises(NotImplementedError, match="independent"):
        model.fit(pathwise=False)
    grids = {c: HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=3 if c != 21 else 2, n_snps=gdl.shapes[c])
             for c in gdl.chromosomes}
    with pytest.raises(ValueError, match="same number of grid points"):
        VIPRSGridPathwisePerChromosome(gdl, grids, **model_kwargs(fx))

    class TwoRanks(LocalComm):
        world_size = 2

    with pytest.raises(NotImplementedError, match="world_size"):
        VIPRSGridPathwisePerChromosome(gdl, make_grid(fx, gdl.m), comm=TwoRanks(), **model_kwargs(fx))
    # a {chromosome: grid} dict is taken as it is
    grids = {c: HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=2, n_snps=1000 * c) for c in gdl.chromosomes}
    m = VIPRSGridPathwisePerChromosome(gdl, grids, **model_kwargs(fx))
    assert all(np.allclose(m.grid_tables[c]["pi"].unique(), grids[c].pi) for c in gdl.chromosomes)
