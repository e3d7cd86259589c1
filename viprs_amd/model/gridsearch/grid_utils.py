"""Model selection / averaging over a fitted ``VIPRSGrid`` (viprs/model/gridsearch/grid_utils.py).

``select_best_model`` supports the reference's three criteria: the ELBO, pseudo-validation from summary statistics, and
`validation` -- the R^2 of every model's polygenic score (``predict`` on the validation loader's genotypes: on the device,
`viprs_amd.genotypes`) against the validation loader's phenotype (grid_utils.py:43-55).  Deviation, on purpose: models are ranked by
their own final ELBOs (``VIPRSGrid.model_elbos`` = the ``ELBO`` column of ``validation_result``).  The
reference calls ``VIPRS.elbo()`` on the (m, n_models) arrays (grid_utils.py:38), which sums the
variational terms over ALL models and therefore only differs between models through the
sigma_epsilon term.
"""
import copy

import numpy as np


def _validation_phenotype(validation_gdl):
    """The validation loader's genotypes and phenotype checked (grid_utils.py:45-47) -> (n,) float64 phenotype."""
    if validation_gdl is None:
        raise ValueError("criterion='validation' needs `validation_gdl`: a data loader with the validation samples' "
                         "genotypes and phenotype (ArrayDataLoader(..., genotype=..., phenotype=...)).")
    if getattr(validation_gdl, "genotype", None) is None:
        raise ValueError("criterion='validation': the validation loader holds no genotypes.  Remedy: "
                         "ArrayDataLoader(..., genotype={chromosome: .bed prefix | (packed_rows, n) | DeviceGenotypes}).")
    y = getattr(validation_gdl, "phenotype", None)
    if y is None:
        y = getattr(getattr(validation_gdl, "sample_table", None), "phenotype", None)
    if y is None and hasattr(validation_gdl, "_open_genotypes"):      # a .bed prefix brings the .fam phenotype with it
        for c in sorted(validation_gdl.genotype):
            validation_gdl._open_genotypes(c)
        y = validation_gdl.phenotype
    if y is None:
        raise ValueError("criterion='validation': the validation loader has no phenotype.  Remedy: "
                         "ArrayDataLoader(..., phenotype=<(n_samples,) array>), or a .fam file with a phenotype column.")
    return np.asarray(y, dtype=np.float64)


def _validation_r2(prs, y):
    """R^2 of every column of `prs` against `y` over the samples whose phenotype is known (a .fam file writes a missing
    phenotype as -9 or NA: NaN here); non-finite values count as 0."""
    from ...eval.continuous_metrics import r2
    if np.ndim(prs) < 1 or np.shape(prs)[0] != y.shape[0]:
        raise ValueError(f"criterion='validation': {y.shape[0]} phenotypes against scores of shape {np.shape(prs)}")
    prs = np.asarray(prs, dtype=np.float64).reshape(y.shape[0], -1)
    known = np.isfinite(y)
    if np.sum(known) < 3:
        raise ValueError(f"criterion='validation': only {int(np.sum(known))} of {y.shape[0]} validation samples have a "
                         "phenotype.  Remedy: ArrayDataLoader(..., phenotype=<(n_samples,) array>).")
    y, prs = y[known], prs[known]
    return np.nan_to_num(np.array([r2(y, prs[:, i]) for i in range(prs.shape[1])]), nan=0.0, neginf=0.0, posinf=0.0)


def pseudo_validation_std_beta(validation_gdl, model_gdl):
    """``{chromosome: standardized betas}`` of a validation loader's summary statistics (``sumstats_table[c]
    .get_snp_pseudo_corr()``, e.g. after ``perform_gwas()``: what the reference's ``pseudo_validate(validation_gdl)`` reads),
    laid out over the model loader's SNPs.  If both loaders have SNP tables the SNPs are aligned by SNP id (`_align` of
    `viprs_amd.genotypes`): SNPs the validation loader lacks get 0, exchanged alleles flip the sign -- exact for the
    correlation with ``2 - x`` -- and any other allele pair gets 0.  Without tables the SNP counts must agree."""
    from ...genotypes import _align
    val_tables, model_tables = getattr(validation_gdl, "snp_table", None), getattr(model_gdl, "snp_table", None)
    out = {}
    for c in sorted(validation_gdl.sumstats_table):
        r = np.asarray(validation_gdl.sumstats_table[c].get_snp_pseudo_corr(), dtype=np.float64)
        if val_tables and model_tables and c in val_tables and c in model_tables:
            # (the validation statistics laid out over the model's SNPs: the model's table is the target of the alignment)
            r, swapped = _align(val_tables[c], model_tables[c], r, c)
            r = np.where(swapped, -r, r)
        elif c in getattr(model_gdl, "shapes", {}) and model_gdl.shapes[c] != r.shape[0]:
            raise ValueError(f"chromosome {c}: {r.shape[0]} SNPs in the validation loader against {model_gdl.shapes[c]} of "
                             "the model (give both loaders SNP tables to have them aligned by SNP id)")
        out[c] = r
    return out


def _validation_std_beta(m, validation_gdl):
    """The standardized betas of the pseudo_validation criterion: a ``{chromosome: std_beta}`` dict, an object with that dict
    as ``.std_beta``, a loader with summary statistics (`pseudo_validation_std_beta`), else the model's own."""
    vb = validation_gdl if isinstance(validation_gdl, dict) else getattr(validation_gdl, "std_beta", None)
    if vb is None and getattr(validation_gdl, "sumstats_table", None):
        vb = pseudo_validation_std_beta(validation_gdl, m.gdl)
    if vb is None:
        vb = getattr(m, "validation_std_beta", None)
    if vb is None:
        raise ValueError("Validation GWADataLoader or standardized betas from a validation set must be "
                         "initialized for the pseudo_validation criterion.")
    return vb


def select_best_model(viprs_grid_model, validation_gdl=None, criterion="ELBO", validation_ld=None):
    """grid_utils.py:8-100.  `pseudo_validation`: the model with the highest summary-statistics pseudo-R^2 on
    held-out standardized betas -- `validation_gdl` may be a `{chromosome: std_beta}` dict (or an object with
    that dict as `.std_beta`), or a loader with summary statistics (``perform_gwas()``; `pseudo_validation_std_beta`); otherwise `viprs_grid_model.validation_std_beta` is used.  `validation`: the model with the
    highest R^2 of its polygenic score on `validation_gdl`'s genotypes against `validation_gdl.phenotype`
    (``validation_result["Validation_R2"]``; non-finite values count as 0).  `validation_ld` (a
    `{chromosome: LDPlan}` dict, or of `(left_bound, indptr, data, low_memory)` tuples) scores the models against the LD of
    an external validation panel instead of the training LD (`VIPRS.pseudo_validate`)."""
    if criterion not in ("ELBO", "validation", "pseudo_validation"):
        raise AssertionError(f"unknown criterion {criterion!r}")
    m = viprs_grid_model
    if criterion == "validation":
        y = _validation_phenotype(validation_gdl)
    ok = m.valid_terminated_models
    if np.sum(ok) < 2:
        raise ValueError("Less than two models converged successfully. Cannot perform model selection.")
    if criterion == "ELBO":
        score = np.array(m.model_elbos, dtype=np.float64)
    elif criterion == "validation":
        score = _validation_r2(m.predict(test_gdl=validation_gdl), y)
        m.validation_result["Validation_R2"] = score
    else:
        vb = _validation_std_beta(m, validation_gdl)
        score = np.nan_to_num(np.asarray(m.pseudo_validate(vb) if validation_ld is None else
                                         m.pseudo_validate(vb, validation_ld=validation_ld), dtype=np.float64), nan=0.0, neginf=0.0, posinf=0.0)
        m.validation_result["Pseudo_Validation_R2"] = score
    score = score.copy()
    score[~ok] = -np.inf
    best = int(np.argmax(score))
    for param in (m.pip, m.post_mean_beta, m.post_var_beta, m.var_gamma, m.var_mu, m.var_tau, m.eta, m.zeta, m.q,
                  m._log_var_tau):
        for c in param:
            param[c] = np.ascontiguousarray(param[c][:, best])      # (a strided view is no valid download target)
    for c in m.eta_diff:
        if m.eta_diff[c].ndim == 2:
            m.eta_diff[c] = np.ascontiguousarray(m.eta_diff[c][:, best])
    m.sigma_epsilon, m._sigma_g = m.sigma_epsilon[best], m._sigma_g[best]
    m.tau_beta, m.pi = m.tau_beta[best], m.pi[best]
    m.n_models = 1
    m.best_model_idx = best
    m.set_fixed_params(m.grid_table.iloc[best].to_dict())
    # the cached partial sums and the device state still belong to the last fitted grid point: drop the sums and
    # put the selected model's state on the device, so that elbo() / to_theta_table() / fit(continued=True) see it
    m._sums, m._sums_valid, m._host_stale = None, False, False
    if m._dstate:
        m._push_state()
    return m


def bayesian_model_average(viprs_grid_model, normalization="softmax"):
    m = viprs_grid_model
    if m.n_models < 2:
        return m
    if np.sum(m.valid_terminated_models) < 1:
        raise ValueError("No models converged successfully. Cannot average models.")
    keep = np.where(m.valid_terminated_models)[0]
    elbos = np.array(m.model_elbos, dtype=np.float64)[keep]
    if normalization == "softmax":
        w = np.exp(elbos - elbos.max())
        w /= w.sum()
    elif normalization == "sum":
        w = elbos - elbos.min() + 1.0
        w /= w.sum()
    else:
        raise KeyError(f"Normalization scheme not recognized. Valid options are: `softmax`, `sum`. Got: {normalization}")
    for param in (m.var_gamma, m.var_mu, m.var_tau, m.q):
        for c in param:
            param[c] = (param[c][:, keep] * w).sum(axis=1).astype(param[c].dtype)
    m.eta = m.compute_eta()
    m.zeta = m.compute_zeta()
    m.update_posterior_moments()
    m._log_var_tau = {c: np.log(m.var_tau[c]) for c in m.var_tau}
    m.eta_diff = {c: np.zeros_like(e) for c, e in m.eta.items()}
    m.model_weights = w
    # hyper-parameters implied by the averaged posterior (grid_utils.py:176-183)
    fixed = copy.deepcopy(m.fix_params)
    m.fix_params = {}
    m._host_stale = False
    m._sums_valid = False
    m.pi = m.sigma_epsilon = m.tau_beta = None
    m.lambda_min = np.float32(0.0) if not np.isscalar(m.lambda_min) else m.lambda_min
    m.m_step()
    m.fix_params = fixed
    m.n_models = 1
    return m


# ---- one grid per chromosome (VIPRSGridPerChromosome, VIPRSGridPathwisePerChromosome): the CLI selects or averages per
# chromosome (bin/viprs_fit:534-551) ----
def _per_chromosome_result(m):
    from ...utils.optim import OptimizeResult
    res = m.optim_result = OptimizeResult()
    res.nit = max(r.nit for rs in m.optim_results.values() for r in (rs if isinstance(rs, list) else [rs]))
    res.stop_iteration = True
    res.success = all(r.success for rs in m.optim_results.values() for r in (rs if isinstance(rs, list) else [rs]))
    m.n_models = 1
    return m


def select_best_model_per_chromosome(model, validation_gdl=None, criterion="ELBO", validation_ld=None):
    """`select_best_model` per chromosome of a fitted ``VIPRSGridPerChromosome`` or ``VIPRSGridPathwisePerChromosome``: every
    chromosome keeps ITS best grid point, the model ends in ``VIPRSPerChromosome``'s result layout (``pi[c]`` ... scalars,
    ``pip[c]`` ... of shape (m_c,), ``optim_results[c]`` one result, ``best_model_idx[c]``).  What `select_best_model` picks
    on each chromosome's own ``VIPRSGrid`` fit, the same arrays.  `validation_ld`: as in `select_best_model`.  `validation`:
    every chromosome's grid is ranked by the R^2 of the score of that chromosome's SNPs (``validation_result[c]["Validation_R2"]``)."""
    if criterion not in ("ELBO", "validation", "pseudo_validation"):
        raise AssertionError(f"unknown criterion {criterion!r}")
    m = model
    if criterion == "validation":
        # every chromosome's grid is ranked by the score of THAT chromosome's SNPs alone
        y = _validation_phenotype(validation_gdl)
        prs = m.predict(test_gdl=validation_gdl, per_chromosome=True)
    best, vb = {}, None
    for c in m.groups:
        ok = np.array([r.valid_optim_result for r in m.optim_results[c]])
        if np.sum(ok) < 2:
            raise ValueError(f"chromosome {c}: less than two models converged successfully. Cannot perform model selection.")
        if criterion == "ELBO":
            score = np.array(m.model_elbos[c], dtype=np.float64)
        elif criterion == "validation":
            if c not in prs:
                raise ValueError(f"chromosome {c}: the validation loader has no genotypes for it")
            score = _validation_r2(prs[c], y)
            m.validation_result[c]["Validation_R2"] = score
        else:
            if vb is None:                                     # (a loader's statistics are laid out once)
                vb = _validation_std_beta(m, validation_gdl)
            score = np.nan_to_num(np.asarray(m.pseudo_validate(vb, chrom=c) if validation_ld is None else
                                             m.pseudo_validate(vb, chrom=c, validation_ld=validation_ld), dtype=np.float64), nan=0.0, neginf=0.0, posinf=0.0)
            m.validation_result[c]["Pseudo_Validation_R2"] = score
        score = score.copy()
        score[~ok] = -np.inf
        best[c] = int(np.argmax(score))
    for param in (m.pip, m.post_mean_beta, m.post_var_beta, m.var_gamma, m.var_mu, m.var_tau, m.eta, m.zeta, m.q,
                  m._log_var_tau, m.eta_diff):
        for c in param:
            param[c] = np.ascontiguousarray(param[c][:, best[c]])
    for d in (m.sigma_epsilon, m._sigma_g, m.tau_beta, m.pi, m.model_elbos):
        for c in d:
            d[c] = d[c][best[c]]
    m.optim_results = {c: m.optim_results[c][best[c]] for c in m.groups}
    m.best_model_idx = best
    return _per_chromosome_result(m)


def bayesian_model_average_per_chromosome(model, normalization="softmax"):
    """`bayesian_model_average` per chromosome of a fitted ``VIPRSGridPerChromosome`` or ``VIPRSGridPathwisePerChromosome``:
    the grid points of every chromosome are averaged with weights from THEIR ELBOs and the chromosome's hyper-parameters
    follow from its averaged posterior (one M-step of that chromosome's model).  ``VIPRSPerChromosome``'s result layout; ``model_weights[c]``."""
    m = model
    if m.n_models < 2:
        return m
    if normalization not in ("softmax", "sum"):
        raise KeyError(f"Normalization scheme not recognized. Valid options are: `softmax`, `sum`. Got: {normalization}")
    weights = {}
    for c in m.groups:
        valid = np.array([r.valid_optim_result for r in m.optim_results[c]])
        if np.sum(valid) < 1:
            raise ValueError(f"chromosome {c}: no models converged successfully. Cannot average models.")
        keep = np.where(valid)[0]
        elbos = np.array(m.model_elbos[c], dtype=np.float64)[keep]
        if normalization == "softmax":
            w = np.exp(elbos - elbos.max())
        else:
            w = elbos - elbos.min() + 1.0
        w /= w.sum()
        weights[c] = w
        for param in (m.var_gamma, m.var_mu, m.var_tau, m.q):
            param[c] = (param[c][:, keep] * w).sum(axis=1).astype(param[c].dtype)
    m.eta = m.compute_eta()
    m.zeta = m.compute_zeta()
    m.update_posterior_moments()
    m._log_var_tau = {c: np.log(m.var_tau[c]) for c in m.var_tau}
    m.eta_diff = {c: np.zeros_like(e) for c, e in m.eta.items()}
    m.model_weights = weights
    # hyper-parameters implied by each chromosome's averaged posterior (grid_utils.py:176-183): the model's own M-step with
    # nothing fixed, run on that chromosome alone
    pi, tau, sig, sg = {}, {}, {}, {}
    for c in m.groups:
        pi[c], tau[c], sig[c], sg[c] = m.m_step_of_chromosome(c)
    m.pi, m.tau_beta, m.sigma_epsilon, m._sigma_g = pi, tau, sig, sg
    # (one record per chromosome: the fit of its grid point with the largest weight)
    m.optim_results = {c: m.optim_results[c][int(np.where([r.valid_optim_result for r in m.optim_results[c]])[0][np.argmax(weights[c])])]
                       for c in m.groups}
    return _per_chromosome_result(m)
