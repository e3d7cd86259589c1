"""``SuSiE`` -- fine-mapping by the sum of single effects on summary statistics, fitted on MI355X.

SuSiE-RSS (Wang et al. 2020; Zou et al. 2022): per LD block, ``z ~ N(R b, R)`` with ``b`` the sum of `L` single effects, each
with exactly one non-zero SNP.  Where the mean-field spike-and-slab of `VIPRS` splits the inclusion probability of a locus
arbitrarily between SNPs in tight LD, a single effect carries the whole distribution over "which SNP": its 95 % credible set
says "one of these five".  The LD of every chromosome lives in ONE device plan and every LD block is fitted on its own, all
blocks in lock step (``LDPlan.susie``); every block stops on its own change of `alpha`.

``z_j = sqrt(n_j) std_beta_j``; the posterior mean effect on the standardised scale is ``sum_l alpha_lj mu_lj / sqrt(n_j)``.

Not built: susieR's ``optim`` estimator of the prior variance and its null check, residual-variance estimation, the
n-adjusted z of ``susie_rss``, ``lambda`` regularisation, several ranks.  The reference has no such class.
(``fit_fn`` lets the CPU tests drive this host logic with `viprs_amd.stats.susie.susie_host`; it is never set by the package
itself: without it and without a GPU the constructor raises.)
"""
import warnings

import numpy as np

from ._merged_plan import MergedPlanModel


class SuSiE(MergedPlanModel):

    def __init__(self, gdl, L=10, prior_variance=50.0, estimate_prior_variance=True, prior_weights=None,
                 float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, fit_fn=None):
        """:param gdl: the data loader (summary statistics and LD matrices per chromosome).
        :param L: the number of single effects per LD block (1..32).
        :param prior_variance: the prior variance of an effect on the z scale (the start of the EM update).
        :param estimate_prior_variance: update every effect's prior variance by EM.
        :param prior_weights: ``{chromosome: array}`` or one array over all SNPs of non-negative weights; normalised
            inside every LD block; a zero excludes the SNP.  None: uniform.
        :param float_precision: precision of `alpha`, `mu` and the LD product, 'float32' or 'float64'.
        :param low_memory: load the upper-triangular form of the LD matrices.
        :param dequantize_on_the_fly: keep integer LD in its stored dtype on the device (threaded through the chromosomes
            as in `VIPRS`).
        :param device: HIP device index (default 0).
        :param fit_fn: test hook -- a callable with `viprs_amd.stats.susie.susie_host`'s signature that replaces the
            device fit.
        """
        self._set_loader(gdl)
        self.L = int(L)
        self.prior_variance = float(prior_variance)
        self.estimate_prior_variance = bool(estimate_prior_variance)
        self._fit_fn = fit_fn
        # (the credible sets' purity and the ELBO read the host arrays: they are kept beside the plan)
        self._load(float_precision, low_memory, dequantize_on_the_fly, device, fit_fn is not None,
                   "SuSiE needs a HIP device: pass fit_fn=viprs_amd.stats.susie.susie_host for a host fit", keep_ld=True,
                   std_beta=False)
        table = gdl.sumstats_table
        self._sqrt_n = {c: np.sqrt(np.asarray(table[c].n_per_snp, dtype=np.float64)) for c in self.chromosomes}
        self.z = {c: self._sqrt_n[c] * np.asarray(table[c].get_snp_pseudo_corr(), dtype=np.float64) for c in self.chromosomes}
        self.log_prior = self._log_prior(prior_weights)
        self.info = None
        self.post_mean_beta = None
        self.pip = None
        self._sets = None

    def _log_prior(self, prior_weights):
        if prior_weights is None:
            return None
        from ..stats.susie import block_starts
        chroms = self.chromosomes
        w = (np.concatenate([np.asarray(prior_weights[c], dtype=np.float64) for c in chroms])
             if isinstance(prior_weights, dict) else np.asarray(prior_weights, dtype=np.float64))
        if w.shape != (self.m,):
            raise ValueError(f"prior_weights: expected {self.m} weights, got shape {w.shape}")
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError("prior_weights must be finite and >= 0")
        starts = block_starts(self._ld[0], self._ld[1], self.low_memory)
        lp = np.full(self.m, -np.inf)
        for s, e in zip(starts[:-1], starts[1:]):
            tot = w[s:e].sum()
            if not tot > 0.0:
                raise ValueError(f"prior_weights are zero for every SNP of the LD block {int(s)}..{int(e) - 1}")
            on = w[s:e] > 0.0
            lp[s:e][on] = np.log(w[s:e][on]) - np.log(tot)
        return lp

    def fit(self, tol=1e-4, max_iter=100):
        """Fits every LD block; a block stops when no `alpha` moved by `tol` in an iteration, or after `max_iter`."""
        z = self._concat(self.z)
        lb, ip, data = self._ld
        if self._fit_fn is not None:
            info = self._fit_fn(lb, ip, data, self.low_memory, z, self.L, self.prior_variance, self.estimate_prior_variance,
                                self.log_prior, self.dequantize_scale, tol, max_iter, self.float_precision)
        else:
            info = self._plan.susie(z, self.L, self.prior_variance, self.estimate_prior_variance, self.log_prior,
                                    dq_scale=self.dequantize_scale, tol=tol, max_iter=max_iter,
                                    float_precision=self.float_precision)
        from ..stats.susie import pips
        self.info = info
        self._sets = None
        bbar = np.sum(np.asarray(info.alpha, dtype=np.float64) * np.asarray(info.mu, dtype=np.float64), axis=1)
        self.post_mean_beta = self._split((bbar / self._concat(self._sqrt_n)).astype(self._T))
        self.pip = self._split(pips(info))
        if not info.converged:
            warnings.warn("Maximum iterations reached without convergence.\n"
                          "You may need to run the model for more iterations.", RuntimeWarning, stacklevel=2)
        return self

    def _fitted(self):
        if self.info is None:
            raise Exception("The model is not fitted. Call `.fit()` first.")

    def get_pip(self):
        return self.pip

    def credible_sets(self, coverage=0.95, min_abs_corr=0.5, n_purity=100, seed=0):
        """`viprs_amd.stats.susie.credible_sets` of the fit; every set also names its `chromosome` and the SNPs' indices
        inside it (`index`)."""
        from ..stats.susie import credible_sets
        self._fitted()
        lb, ip, data = self._ld
        sets = credible_sets(self.info, lb, ip, data, self.low_memory, self.dequantize_scale, coverage, min_abs_corr,
                             n_purity, seed)
        for cs in sets:
            first = int(cs["snps"][0])
            cs["chromosome"] = next(c for c, (a, e) in self._seg.items() if a <= first < e)
            cs["index"] = cs["snps"] - self._seg[cs["chromosome"]][0]
        return sets

    def elbo(self):
        """The evidence lower bound of every LD block (`viprs_amd.stats.susie.susie_elbo`)."""
        from ..stats.susie import susie_elbo
        self._fitted()
        lb, ip, data = self._ld
        return susie_elbo(lb, ip, data, self.low_memory, self._concat(self.z), self.info, self.log_prior, self.dequantize_scale)

    def to_table(self, per_chromosome=False, **cs_kwargs):
        """The fit as a pandas table: CHR, the SNP's index, BETA, PIP and CS -- the number of the credible set
        (`credible_sets(**cs_kwargs)`, in its order, from 1) the SNP belongs to, 0 for none; a SNP in several sets gets the
        first."""
        import pandas as pd
        self._fitted()
        cs_of = {c: np.zeros(self.shapes[c], dtype=np.int64) for c in self.chromosomes}
        for k, cs in reversed(list(enumerate(self.credible_sets(**cs_kwargs)))):
            cs_of[cs["chromosome"]][cs["index"]] = k + 1
        tables = {c: pd.DataFrame({"CHR": c, "IDX": np.arange(self.shapes[c]), "BETA": self.post_mean_beta[c],
                                   "PIP": self.pip[c], "CS": cs_of[c]}) for c in self.chromosomes}
        return tables if per_chromosome else pd.concat([tables[c] for c in self.chromosomes])
