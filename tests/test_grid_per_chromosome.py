"""`VIPRSGridPerChromosome`: one grid search per chromosome (the reference CLI's default with --hyp-search GS / BMA,
bin/viprs_fit:232-238, :373-390, :450-466, :534-551), all (chromosome, grid point) pairs in lock step, independent mode.

Fixtures (tests/golden/make_fitchr_grid_golden.py): each chromosome fitted ALONE by the reference,
``VIPRSGrid(sub_loader(c), grid_c).fit(pathwise=False)``.  The reference fits through e_step (fma, skip branch), the
lock-step fit through e_step_grid (neither): trajectories agree at the tolerances of
tests/test_grid.py::test_batched_grid_fit_matches_independent_reference_fits, not bit for bit."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_fit import loader_from_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["fitchr_grid_3chr_upper", "fitchr_grid_2chr_sym_lambda"]
MAX_ITER = 100


def load(name):
    fx = np.load(os.path.join(HERE, "golden", name + ".npz"))
    gdl = loader_from_fixture(fx)
    for c in gdl.chromosomes:
        if f"emp_lambda_min_{c}" in fx:                 # the LD's get_lambda_min of the fixture's chromosome
            gdl.ld[c]._lambda_min = float(fx[f"emp_lambda_min_{c}"])
    return fx, gdl


def make_grid(fx, n_snps):
    from viprs_amd.model import HyperparameterGrid
    steps = {k: int(fx[f"grid_{k}"]) for k in ("sigma_epsilon_steps", "pi_steps", "lambda_min_steps") if f"grid_{k}" in fx}
    return HyperparameterGrid(n_snps=n_snps, h2_est=float(fx["h2_est"]), h2_se=float(fx["h2_se"]), **steps)


def fit(fx, gdl, **kw):
    from viprs_amd.model import VIPRSGridPerChromosome
    model = VIPRSGridPerChromosome(gdl, make_grid(fx, gdl.m), low_memory=bool(fx["low_memory"]), **kw)
    return model.fit(pathwise=False, max_iter=MAX_ITER)


def check_against_reference(model, fx):
    for c in (int(c) for c in fx["chroms"]):
        vr = model.validation_result[c]
        np.testing.assert_allclose(vr["sigma_epsilon"], fx[f"grid_sigma_epsilon_{c}"], rtol=1e-12)
        np.testing.assert_allclose(vr["pi"], fx[f"grid_pi_{c}"], rtol=1e-12)
        if f"grid_lambda_min_{c}" in fx:
            np.testing.assert_allclose(vr["lambda_min"], fx[f"grid_lambda_min_{c}"], rtol=1e-12)
        elbo, ref = vr["ELBO"].to_numpy().astype(np.float64), fx[f"elbo_{c}"]
        assert np.all(elbo >= ref - 0.05) and np.all(elbo - ref < 8.0), (c, elbo - ref)
        assert model.pip[c].shape == fx[f"pip_{c}"].shape == (model.shapes[c], model.n_models)
        np.testing.assert_allclose(model.post_mean_beta[c], fx[f"post_mean_beta_{c}"], rtol=2e-2, atol=2e-5)
        # PIPs above 0.05 at rtol=2e-2, except the SNPs the reference's e_step left stale at their start gamma == pi through
        # its skip branch (e_step.hpp:410-413), which e_step_grid has not (test_grid.py): there the fixture's PIP equals the
        # column's pi exactly
        ref_pip = fx[f"pip_{c}"]
        stale = ref_pip == np.asarray(fx[f"grid_pi_{c}"], dtype=ref_pip.dtype)[None, :]
        big = (ref_pip > 0.05) & ~stale
        np.testing.assert_allclose(model.pip[c][big], ref_pip[big], rtol=2e-2)
        np.testing.assert_allclose(np.asarray(model.tau_beta[c], dtype=np.float64), fx[f"tau_beta_{c}"], rtol=2e-2)
        assert list(vr["Converged"]) == list(fx[f"converged_{c}"])


def assert_same_fit(a, b, c, G):
    """Two fits of chromosome c (a: VIPRSGridPerChromosome, b: same layout or VIPRSGrid) are `==`."""
    ra = a.optim_results[c]
    rb = b.optim_results[c] if isinstance(b.optim_results, dict) else b.optim_results
    assert [r.nit for r in ra] == [r.nit for r in rb]
    assert [r.message for r in ra] == [r.message for r in rb]
    ea = a.model_elbos[c]
    eb = b.model_elbos[c] if isinstance(b.model_elbos, dict) else b.model_elbos
    assert np.array_equal(ea, eb)
    for name in ("var_gamma", "var_mu", "q", "var_tau", "pip", "post_mean_beta", "post_var_beta"):
        x, y = getattr(a, name)[c], getattr(b, name)[c]
        assert x.shape == y.shape == (a.shapes[c], G) and np.array_equal(x, y), (c, name)
    for name in ("pi", "tau_beta", "sigma_epsilon", "_sigma_g"):
        x = getattr(a, name)[c]
        y = getattr(b, name)[c] if isinstance(getattr(b, name), dict) else getattr(b, name)
        assert np.array_equal(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)), (c, name)


def one_chromosome_loader(gdl, c):
    from viprs_amd.data import ArrayDataLoader
    return ArrayDataLoader({c: gdl.ld[c]}, {c: gdl.sumstats_table[c]})


# ---- CPU: the host logic with the oracle's e_step_grid ---------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_lockstep_fit_cpu_matches_reference(name):
    fx, gdl = load(name)
    model = fit(fx, gdl, e_step_fn=O.cpp_e_step_grid)
    check_against_reference(model, fx)
    # the pairs stop at different iterations: the pair mask is exercised
    nits = [r.nit for rs in model.optim_results.values() for r in rs]
    assert len(set(nits)) > 1
    assert all(len(model.history[c]["ELBO"][g]) == model.optim_results[c][g].nit
               for c in model.groups for g in range(model.n_models))


@pytest.mark.parametrize("name", FIXTURES)
def test_lockstep_fit_cpu_equals_per_chromosome_fits(name):
    """The lock-step fit == the same host logic run on each chromosome's loader alone (its own active list)."""
    fx, gdl = load(name)
    model = fit(fx, gdl, e_step_fn=O.cpp_e_step_grid)
    for c in model.groups:
        alone = fit(fx, one_chromosome_loader(gdl, c), e_step_fn=O.cpp_e_step_grid)
        assert alone.grid_tables[c].equals(model.grid_tables[c])
        assert_same_fit(model, alone, c, model.n_models)
        assert alone.history[c]["ELBO"] == model.history[c]["ELBO"]


def _as_viprs_grid(model, c, gdl):
    """A VIPRSGrid of chromosome c alone holding the lock-step fit's results for c (what select_best_model /
    bayesian_model_average read), for comparing the per-chromosome functions with the existing ones on the same inputs."""
    from viprs_amd.model import VIPRSGrid
    g = VIPRSGrid(one_chromosome_loader(gdl, c), model.grids[c], low_memory=True, e_step_fn=O.cpp_e_step)
    g.grid_table = model.grid_tables[c]
    for name in ("var_gamma", "var_mu", "var_tau", "q", "eta", "zeta", "pip", "post_mean_beta", "post_var_beta",
                 "_log_var_tau", "eta_diff"):
        setattr(g, name, {c: getattr(model, name)[c].copy()})
    g.pi, g.tau_beta = model.pi[c].copy(), model.tau_beta[c].copy()
    g.sigma_epsilon, g._sigma_g = model.sigma_epsilon[c].copy(), model._sigma_g[c].copy()
    g.model_elbos = model.model_elbos[c].copy()
    g.optim_results = list(model.optim_results[c])
    g.validation_result = model.validation_result[c].copy()
    g.lambda_min = g._T.type(g.lambda_min)
    return g


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("criterion", ["ELBO", "pseudo_validation", "bma_softmax", "bma_sum"])
def test_selection_and_bma_per_chromosome_cpu(criterion, name):
    from viprs_amd.model import (bayesian_model_average, bayesian_model_average_per_chromosome, select_best_model,
                                 select_best_model_per_chromosome)
    fx, gdl = load(name)
    model = fit(fx, gdl, e_step_fn=O.cpp_e_step_grid)
    vb = {c: fx[f"validation_std_beta_{c}"] for c in model.groups}
    refs = {}
    for c in model.groups:
        g = _as_viprs_grid(model, c, gdl)
        if criterion.startswith("bma"):
            refs[c] = bayesian_model_average(g, normalization=criterion[4:])
        else:
            refs[c] = select_best_model(g, {c: vb[c]}, criterion=criterion)
    if criterion.startswith("bma"):
        out = bayesian_model_average_per_chromosome(model, normalization=criterion[4:])
    else:
        out = select_best_model_per_chromosome(model, vb, criterion=criterion)
    assert out.n_models == 1
    for c, ref in refs.items():
        if not criterion.startswith("bma"):
            assert out.best_model_idx[c] == ref.best_model_idx
        else:
            assert np.array_equal(out.model_weights[c], ref.model_weights)
        for name in ("pip", "post_mean_beta", "post_var_beta", "var_gamma", "var_mu", "var_tau", "q"):
            x, y = getattr(out, name)[c], getattr(ref, name)[c]
            assert x.shape == (model.shapes[c],) and np.array_equal(x, y), (c, name)
        for name in ("pi", "tau_beta", "sigma_epsilon", "_sigma_g"):
            assert np.float64(getattr(out, name)[c]) == np.float64(getattr(ref, name)), (c, name)
    # the reference's pseudo-R^2 per grid point of each chromosome's fit
    if criterion == "ELBO":
        model = fit(fx, gdl, e_step_fn=O.cpp_e_step_grid)
        for c in model.groups:
            np.testing.assert_allclose(model.pseudo_validate(vb, chrom=c), fx[f"pseudo_r2_{c}"], rtol=1e-2)


def test_refusals_cpu():
    from viprs_amd.model import HyperparameterGrid, VIPRSGridPerChromosome
    fx, gdl = load("fitchr_grid_3chr_upper")
    model = VIPRSGridPerChromosome(gdl, make_grid(fx, gdl.m), low_memory=True, e_step_fn=O.cpp_e_step_grid)
    with pytest.raises(NotImplementedError, match="pathwise"):
        model.fit(pathwise=True)
    with pytest.raises(NotImplementedError, match="float32"):
        VIPRSGridPerChromosome(gdl, make_grid(fx, gdl.m), float_precision="float64", e_step_fn=O.cpp_e_step_grid)
    grids = {c: HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=3 if c != 21 else 2, n_snps=gdl.shapes[c])
             for c in gdl.chromosomes}
    with pytest.raises(ValueError, match="same number of grid points"):
        VIPRSGridPerChromosome(gdl, grids, e_step_fn=O.cpp_e_step_grid)
    # a {chromosome: grid} dict is taken as it is
    grids = {c: HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=2, n_snps=1000 * c) for c in gdl.chromosomes}
    m = VIPRSGridPerChromosome(gdl, grids, e_step_fn=O.cpp_e_step_grid)
    assert all(np.allclose(m.grid_tables[c]["pi"].unique(), grids[c].pi) for c in gdl.chromosomes)
