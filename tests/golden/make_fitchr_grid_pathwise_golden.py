#!/usr/bin/env python3
"""Generates tests/golden/fitchr_grid_pathwise_*.npz: the reference's grid search PER CHROMOSOME in the pathwise mode (the
CLI's default ``--grid-search-mode``, bin/viprs_fit:885, :501-504).

As make_fitchr_grid_golden.py, with ``fit(pathwise=True)``: every chromosome is fitted ALONE with the reference's own Python
layer, ``VIPRSGrid(sub_loader(c), grid_c).fit(pathwise=True)``, through the in-memory stubs of make_fit_golden.py
(oracle/_ref must have been built by ``build()``).  Besides the fitted grid, each chromosome's whole ELBO history and every
point's ``nit`` are stored.

Only the resulting ARRAYS are committed: per chromosome the inputs (in the keys tests/test_fit.py:loader_from_fixture
reads; LD other than AR(1) travels as its upper-triangular store), the grid columns and the fit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_fit_golden import install_stubs, make_loader, sub_loader      # noqa: E402
from oracle import oracle as O                                          # noqa: E402

CASES = [
    # fp32 AR(1) LD, upper-triangular form, a sigma_epsilon x pi grid; n and h2 differ per chromosome, so that the
    # chromosomes stop at different iterations
    dict(name="fitchr_grid_pathwise_3chr_upper", chrom_sizes={20: [280, 160], 21: [350], 22: [200, 120, 90]},
         low_memory=True, n_of={20: 1e5, 21: 8e4, 22: 2e5}, h2_of={20: 0.25, 21: 0.12, 22: 0.15},
         grid=dict(sigma_epsilon_steps=2, pi_steps=3), emp_lambda_min=None),
    # symmetric LD, a lambda_min grid scaled by each chromosome's own get_lambda_min
    dict(name="fitchr_grid_pathwise_2chr_sym_lambda", chrom_sizes={21: [260, 200], 22: [310]}, low_memory=False,
         n_of={21: 1e5, 22: 6e4}, h2_of={21: 0.2, 22: 0.1},
         grid=dict(sigma_epsilon_steps=2, pi_steps=2, lambda_min_steps=3), emp_lambda_min={21: 0.04, 22: 0.015}),
    # float64 state on int8 long-range LD (upper-triangular store, dequantised on the fly)
    dict(name="fitchr_grid_pathwise_f64_lr_int8", chrom_sizes={21: [200, 150], 22: [180]}, low_memory=True,
         n_of={21: 1e5, 22: 7e4}, h2_of={21: 0.2, 22: 0.12}, grid=dict(sigma_epsilon_steps=2, pi_steps=2),
         emp_lambda_min=None, ld_dtype=np.int8, ld_kind="longrange",
         model=dict(float_precision="float64", dequantize_on_the_fly=True)),
]
MAX_ITER = 100


def main():
    assert O.have_reference()
    GWADataLoader = install_stubs()
    sys.path.insert(0, "/root/reference")
    from viprs.model.gridsearch.HyperparameterGrid import HyperparameterGrid
    from viprs.model.gridsearch.VIPRSGrid import VIPRSGrid
    only = sys.argv[1:]
    for case in CASES:
        name = case["name"]
        if only and name not in only:
            continue
        chrom_sizes, model_kw = case["chrom_sizes"], case.get("model", {})
        ld_kind = case.get("ld_kind", "ar1")
        gdl, inputs = make_loader(GWADataLoader, chrom_sizes, case.get("ld_dtype", np.float32), seed=733, ld_kind=ld_kind,
                                  n_of=case["n_of"], h2_of=case["h2_of"])
        out = dict(chroms=np.array(sorted(chrom_sizes)), low_memory=case["low_memory"], max_iter=MAX_ITER, h2_est=0.2, h2_se=0.1,
                   ld_kind=ld_kind, float_precision=str(model_kw.get("float_precision", "float32")),
                   dequantize_on_the_fly=bool(model_kw.get("dequantize_on_the_fly", False)),
                   **{f"grid_{k}": v for k, v in case["grid"].items()})
        for c in sorted(chrom_sizes):
            sub = sub_loader(GWADataLoader, gdl, c)
            m_c = int(sum(chrom_sizes[c]))
            grid = HyperparameterGrid(n_snps=m_c, h2_est=0.2, h2_se=0.1, **case["grid"])
            if case["emp_lambda_min"] is not None:
                lam = case["emp_lambda_min"][c]
                sub.ld[c].get_lambda_min = lambda *a, _lam=lam, **k: _lam
                grid.generate_lambda_min_grid(steps=case["grid"]["lambda_min_steps"], emp_lambda_min=lam)
                out[f"emp_lambda_min_{c}"] = np.float64(lam)
            model = VIPRSGrid(sub, grid, low_memory=case["low_memory"], **model_kw)
            model.fit(pathwise=True, max_iter=MAX_ITER, disable_pbar=True)
            model.validation_std_beta = {c: inputs[c][2].validation_std_beta}
            vr = model.validation_result
            ld_sym, ld_up, ss = inputs[c]
            out.update({
                f"sizes_{c}": np.array(chrom_sizes[c]), f"rho_{c}": ld_sym.rho, f"std_beta_{c}": ss.std_beta,
                f"n_per_snp_{c}": ss.n_per_snp, f"validation_std_beta_{c}": ss.validation_std_beta,
                f"grid_sigma_epsilon_{c}": vr["sigma_epsilon"].to_numpy(), f"grid_pi_{c}": vr["pi"].to_numpy(),
                f"elbo_{c}": vr["ELBO"].to_numpy().astype(np.float64), f"converged_{c}": vr["Converged"].to_numpy(),
                f"messages_{c}": np.array(list(vr["Optimization_message"])),
                f"nit_{c}": np.array([r.nit for r in model.optim_results]),
                f"elbo_history_{c}": np.array(model.history["ELBO"], dtype=np.float64),
                f"pi_{c}": np.asarray(model.pi, dtype=np.float64), f"tau_beta_{c}": np.asarray(model.tau_beta, dtype=np.float64),
                f"sigma_epsilon_{c}": np.asarray(model.sigma_epsilon, dtype=np.float64),
                f"sigma_g_{c}": np.asarray(model._sigma_g, dtype=np.float64),
                f"pseudo_r2_{c}": np.asarray(model.pseudo_validate(), dtype=np.float64),
                f"pip_{c}": model.pip[c], f"post_mean_beta_{c}": model.post_mean_beta[c],
                f"post_var_beta_{c}": model.post_var_beta[c], f"q_{c}": model.q[c]})
            if ld_kind != "ar1":                         # AR(1) LD is rebuilt from rho; anything else travels
                out[f"ld_upper_indptr_{c}"] = ld_up.ld_indptr
                out[f"ld_upper_data_{c}"] = ld_up.ld_data
            if "lambda_min" in vr:
                out[f"grid_lambda_min_{c}"] = vr["lambda_min"].to_numpy()
            print(name, "chr", c, "nit", out[f"nit_{c}"], "ELBO", out[f"elbo_{c}"], "converged", out[f"converged_{c}"])
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


if __name__ == "__main__":
    main()
