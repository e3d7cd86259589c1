"""``SBayesR`` -- the Gibbs sampler of Lloyd-Jones et al. (2019; GCTB ``--sbayes R``): the sampling counterpart of `VIPRSMix`,
with its sweep on MI355X.

The prior of every effect is a finite mixture of normals with a point mass at zero: component ``k = 1..K`` has variance
``gamma_k sigma2_beta`` and weight ``pi_k``, the null has weight ``pi_0``.  A chain draws each effect from its conditional
posterior, SNP after SNP over each LD block (`DeviceState.bayesr_sweep`: the mixture E-step's serial sweep with a draw where
the E-step stores an expectation; `viprs_amd.stats.bayesr` is its host definition and the CPU fallback), then re-draws the
hyper-parameters on the host from ``default_rng([seed, chain])``:

    pi ~ Dirichlet(counts + 1)
    sigma2_beta ~ (sum_k ssq_k / gamma_k + nu s2) / chi2(nu + m_nonzero),                         nu = 4
    sigma2_e ~ (nbar (1 - 2 sum beta_hat eta + sum eta^2 + sum q eta) + nu s2_e) / chi2(nbar + nu),    floored at 1e-6
    h2 = sum eta^2 + sum q eta

and averages the Rao-Blackwellised means ``sum_k gamma_k mu_k`` and the inclusion probabilities ``1 - gamma_0`` after the
burn-in (`DeviceState.bayesr_accumulate`).  The LD of every chromosome lives in one device plan; an iteration of a chain is one
draws launch, one sweep, one sums call, after the burn-in one accumulate launch, and one `prep_mixture`.  ``n_chains > 1``
runs several states on the one plan, swept one after the other; chain ``c`` takes the device draws of ``draw_index = c 2^32 +
iteration`` and its own host generator, so it does not depend on the number of chains.  A chain whose ``sum eta^2`` stops
being finite or exceeds ``sum beta_hat^2`` is ``diverged`` (`LDpred2`'s rule): reported, and left out of the mean.

Result layout, `predict`, `pseudo_validate` and `to_table` of `ClumpThreshold` (one model); `to_table` has a ``PIP`` column.
``grid_table`` has one row per chain: ``diverged``, ``n_sweeps`` (sweeps it ran), the means of the hyper-parameters.

A LIMIT OF THE SAMPLER AS SPECIFIED: more SNPs than samples.  When ``m`` exceeds ``n`` (diverged in every trial at m / n of 1.6
and above, never at 0.5 and below) the chain over-fits the sampling noise of the marginal effects: ``1 - 2 sum beta_hat eta +
sum eta^2 + sum q eta`` turns negative, ``sigma2_e`` falls through its floor, every SNP is then included without shrinkage,
``pi_0`` goes to zero within two sweeps and ``h2`` passes 1.  The divergence rule stops such a chain and the fit reports it;
the effects of a fit whose chains all diverged are zero.  This holds for data whose summary statistics are exactly consistent
with the LD, on the host backend as on the device; a higher floor does not cure it (the chain then lives on with ``h2`` > 1).
GCTB's robust parameterisation addresses this regime and is not built; `LDpred2(mode="auto")` runs there.  With windowed
(banded) LD blocks pass ``low_memory=False``: the band kernel of this sweep exists for the symmetric form only.

Not built: GCTB's ``--rsq`` / ``--p-value`` robustness filters and its robust parameterisation; more than 4 non-null
components; float64 states; several ranks; ``math_mode="fast"``; row-by-row kernels; per-chromosome hyper-parameters.  The
reference has no such class.
"""
import numpy as np

from ..stats import bayesr as B
from ._chain_engines import divergence_rule, tail_mean
from .ClumpThreshold import ClumpThreshold


class SBayesR(ClumpThreshold):

    def __init__(self, gdl, gamma=B.DEFAULT_GAMMA, pi=B.DEFAULT_PI, h2_init="ldsc", n_iter=1000, n_burnin=250, thin=1, n_chains=1,
                 seed=0, float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, backend=None,
                 sweep_fn=None, draws_fn=None, score_fn=None, keep_draws_log=False, comm=None):
        """:param gdl: the data loader (summary statistics and LD matrices per chromosome).
        :param gamma: the K <= 4 variance multipliers of the non-null components (GCTB: 0.01, 0.1, 1).
        :param pi: the K + 1 initial weights, the null first (GCTB: 0.95, 0.02, 0.02, 0.01).
        :param h2_init: 'ldsc' (the LD-score regression estimate over the model's own LD, as `LDpred2`) or a number.
        :param n_iter, n_burnin, thin: sweeps in all, sweeps before the means are accumulated, and every `thin`-th after.
        :param n_chains: independent chains, averaged.
        :param seed: of the device draws (Philox key) and, with the chain, of the host `Generator`.
        :param backend: 'device' (default with a GPU) or 'host' (`viprs_amd.stats.bayesr`).
        :param sweep_fn: host backend -- a callable with `viprs_amd.stats.bayesr.bayesr_sweep_host`'s signature in its place.
        :param draws_fn: host backend -- a callable ``(seed, draw_index, m) -> (U, z)`` in place of `bayesr_draws_host`.
        :param score_fn: as in `LDPredInf`: the LD scores of ``h2_init='ldsc'``.
        :param keep_draws_log: device backend -- `draws_log[draw_index]` keeps the ``(U, z)`` that sweep used (tests).
        """
        self._set_loader(gdl, comm)
        self._configure(gamma, pi, n_iter, n_burnin, thin, n_chains, seed, float_precision, backend, sweep_fn, draws_fn,
                        keep_draws_log)
        ldsc = isinstance(h2_init, str)
        if ldsc and h2_init != "ldsc":
            raise ValueError(f"h2_init: 'ldsc' or a number, got {h2_init!r}")
        lb, ip, data, corr = self._load(
            "float32", low_memory, dequantize_on_the_fly, device, self._sweep_fn is not None,
            "SBayesR needs a HIP device (backend='host' runs viprs_amd.stats.bayesr on the CPU)", ld_correction=ldsc,
            n_per_snp=True)
        self._set_h2_init(self._ldsc_h2(lb, ip, data, corr, score_fn) if ldsc else h2_init)

    def _set_h2_init(self, h2_init):
        self.h2_init = float(h2_init)
        if not self.h2_init > 0.0:
            raise ValueError(f"h2_init = {self.h2_init!r}: a positive heritability is needed")

    def _configure(self, gamma, pi, n_iter, n_burnin, thin, n_chains, seed, float_precision, backend, sweep_fn, draws_fn,
                   keep_draws_log):
        """What a fit needs beside the data: checked and stored by both constructors."""
        if np.dtype(float_precision) != np.float32:
            raise ValueError("SBayesR: float_precision must be 'float32' (the sweep has no float64 form)")
        self.gamma = np.atleast_1d(np.asarray(gamma, dtype=np.float64))
        self.pi_init = np.atleast_1d(np.asarray(pi, dtype=np.float64))
        K = int(self.gamma.shape[0])
        if not 1 <= K <= B.MAX_K or not np.all(self.gamma > 0):
            raise ValueError(f"gamma: 1 to {B.MAX_K} positive variance multipliers")
        if self.pi_init.shape != (K + 1,) or not np.all(self.pi_init > 0) or abs(self.pi_init.sum() - 1.0) > 1e-8:
            raise ValueError("pi: K + 1 positive weights that sum to 1, the null first")
        self.K = K
        self.n_iter, self.n_burnin, self.thin, self.n_chains = int(n_iter), int(n_burnin), int(thin), int(n_chains)
        if not (0 <= self.n_burnin < self.n_iter and self.thin >= 1 and self.n_chains >= 1):
            raise ValueError("0 <= n_burnin < n_iter, thin >= 1 and n_chains >= 1")
        if backend not in (None, "device", "host"):
            raise ValueError(f"backend: 'device' or 'host', got {backend!r}")
        host = backend == "host" or sweep_fn is not None
        self.seed = int(seed)
        self._sweep_fn = (sweep_fn or B.bayesr_sweep_host) if host else None
        self._draws_fn = draws_fn or B.bayesr_draws_host
        self._keep_draws_log = bool(keep_draws_log)
        self.draws_log = {}
        self.n_models = 1
        self.post_mean_beta = self.pip = None
        self.grid_table = self.validation_result = None
        self.best_model_idx = None
        self.diverged = self.n_sweeps = self.pi_est = self.sigma2_beta_est = self.sigma2_e_est = self.h2_est = None
        self.pi_history = self.h2_history = self.chain_beta = None

    @classmethod
    def from_plan(cls, plan, std_beta, n_per_snp, dq_scale, h2_init, gamma=B.DEFAULT_GAMMA, pi=B.DEFAULT_PI, n_iter=1000,
                  n_burnin=250, thin=1, n_chains=1, seed=0, keep_draws_log=False):
        """A model on an existing `LDPlan` (`MergedPlanModel._attach`: one chromosome; the LD may exist on the device only:
        synthetic plans, plans another model has built); `h2_init` a number.  Device backend only; the plan stays the
        caller's."""
        self = cls.__new__(cls)
        self._configure(gamma, pi, n_iter, n_burnin, thin, n_chains, seed, "float32", "device", None, None, keep_draws_log)
        self._attach(plan, dq_scale, std_beta, n_per_snp)
        self._set_h2_init(h2_init)
        return self

    # -- the two backends of a chain: a mixture state on the device, or arrays swept on the host --------------------------------
    class _Device:
        def __init__(self, model, beta):
            from ..plan import DeviceState
            self.model, self.dq = model, model.dequantize_scale
            self.st = DeviceState(model._plan, "float32", model="mixture", width=model.K, placement="off")
            self.st.upload("std_beta", beta)
            self.st.set_n_per_snp(model._n_per_snp)
            self.st.bayesr_reset_mean()

        def prep(self, pi, sigma2_beta, sigma2_e):
            self.st.prep_mixture(*B.bayesr_prep_args(pi, self.model.gamma, sigma2_beta, sigma2_e))

        def sweep(self, draw_index):
            self.st.bayesr_sweep(self.dq, seed=self.model.seed, draw_index=draw_index, sync=False)
            sums = self.st.bayesr_sums()
            if self.model._keep_draws_log:
                self.model.draws_log[draw_index] = (self.st.bayesr_download("unif"), self.st.bayesr_download("z"))
            return sums

        def accumulate(self):
            self.st.bayesr_accumulate()

        def means(self):
            return self.st.bayesr_download("mean_sum"), self.st.bayesr_download("pip_sum")

        def close(self):
            self.st.close()

    class _Host:
        def __init__(self, model, beta):
            self.model, self.beta, self.dq = model, beta, model.dequantize_scale
            m = model.m
            self.eta, self.q = np.zeros(m, dtype=np.float32), np.zeros(m, dtype=np.float32)
            self.mean, self.pip = np.zeros(m), np.zeros(m)
            self.inputs = self.gam = self.mu = None

        def prep(self, pi, sigma2_beta, sigma2_e):
            self.inputs = B.bayesr_prep_host(self.model._n_per_snp, pi, self.model.gamma, sigma2_beta, sigma2_e)

        def sweep(self, draw_index):
            lb, ip, data = self.model._ld
            unif, z = self.model._draws_fn(self.model.seed, draw_index, self.model.m)
            mm, sv, ul, lnp = self.inputs
            _, self.mu, self.gam, ks = self.model._sweep_fn(lb, ip, data, self.model.low_memory, self.beta, mm, sv, ul, lnp, unif,
                                                            z, self.eta, self.q, self.dq)
            return B.bayesr_sums_host(ks, self.eta, self.q, self.beta, self.model.K)

        def accumulate(self):
            B.bayesr_accumulate_host(self.gam, self.mu, self.mean, self.pip)

        def means(self):
            return self.mean.copy(), self.pip.copy()

        def close(self):
            pass

    def _run_chain(self, chain, beta_hat, diverges):
        """One chain: ``(mean_sum, pip_sum, n_samples, diverged, histories, sweeps run)``."""
        K, m = self.K, self.m
        rng = np.random.default_rng([self.seed, chain])
        nbar = float(np.mean(self._n_per_snp))
        h2 = min(max(self.h2_init, 1e-4), 0.95)
        pi = self.pi_init.copy()
        sigma2_beta = B.initial_sigma2_beta(h2, m, pi, self.gamma)
        sigma2_e = 1.0 - h2
        s2, s2_e = sigma2_beta * (B.NU - 2.0) / B.NU, sigma2_e * (B.NU - 2.0) / B.NU
        hist = {"pi": np.full((self.n_iter, K + 1), np.nan), "sigma2_beta": np.full(self.n_iter, np.nan),
                "sigma2_e": np.full(self.n_iter, np.nan), "h2": np.full(self.n_iter, np.nan)}
        n_samples, diverged, n_sweeps = 0, False, 0
        eng = (self._Host if self._sweep_fn is not None else self._Device)(self, beta_hat)
        try:
            eng.prep(pi, sigma2_beta, sigma2_e)
            for it in range(self.n_iter):
                s = eng.sweep((chain << 32) | it)
                n_sweeps += 1
                counts, ssq = s[:K + 1], s[K + 1:2 * K + 1]
                sum_q_eta, sum_eta2, sum_beta_eta = s[2 * K + 1:2 * K + 4]
                if diverges(sum_eta2):
                    diverged = True
                    break
                if it >= self.n_burnin and (it - self.n_burnin) % self.thin == 0:
                    eng.accumulate()
                    n_samples += 1
                pi = B.draw_pi(rng, counts)
                sigma2_beta = B.draw_sigma2_beta(rng, ssq, self.gamma, float(counts[1:].sum()), s2)
                sigma2_e = B.draw_sigma2_e(rng, nbar, sum_beta_eta, sum_eta2, sum_q_eta, s2_e)
                hist["pi"][it], hist["sigma2_beta"][it], hist["sigma2_e"][it] = pi, sigma2_beta, sigma2_e
                hist["h2"][it] = sum_eta2 + sum_q_eta
                if it + 1 < self.n_iter:
                    eng.prep(pi, sigma2_beta, sigma2_e)
            mean, pip = eng.means()
        finally:
            eng.close()
        return mean, pip, n_samples, diverged, hist, n_sweeps

    def fit(self):
        """The chains one after the other: `n_burnin` sweeps, then the sweeps whose Rao-Blackwellised means are averaged."""
        import pandas as pd
        m = self.m
        beta_hat, diverges = divergence_rule(self)
        C = self.n_chains
        self.draws_log = {}
        means, pips = np.zeros((m, C)), np.zeros((m, C))
        self.diverged = np.zeros(C, dtype=bool)
        self.n_sweeps = np.zeros(C, dtype=np.int64)
        hists = []
        for c in range(C):
            mean, pip, n, div, hist, self.n_sweeps[c] = self._run_chain(c, beta_hat, diverges)
            self.diverged[c] = div or n == 0
            if not self.diverged[c]:
                means[:, c], pips[:, c] = mean / n, pip / n
            hists.append(hist)
        keep = ~self.diverged
        est = lambda k: np.array([tail_mean(h[k], self.n_burnin, d) for h, d in zip(hists, self.diverged)])
        self.pi_est, self.sigma2_beta_est, self.sigma2_e_est, self.h2_est = est("pi"), est("sigma2_beta"), est("sigma2_e"), est("h2")
        self.pi_history = [h["pi"] for h in hists]
        self.h2_history = [h["h2"] for h in hists]
        final = (means[:, keep].mean(axis=1) if keep.any() else np.zeros(m)).astype(np.float32)
        pip = (pips[:, keep].mean(axis=1) if keep.any() else np.zeros(m)).astype(np.float32)
        self.chain_beta = self._split(means.astype(np.float32))
        self.post_mean_beta, self.pip = self._split(final), self._split(pip)
        self.best_model_idx = 0                                     # one model: nothing to select
        self.grid_table = pd.DataFrame(dict(chain=np.arange(C), diverged=self.diverged, n_sweeps=self.n_sweeps, h2=self.h2_est,
                                            sigma2_beta=self.sigma2_beta_est, sigma2_e=self.sigma2_e_est,
                                            **{f"pi_{k}": self.pi_est[:, k] for k in range(self.K + 1)}))
        self.validation_result = self.grid_table.copy()
        return self

    def to_table(self, per_chromosome=False):
        """The effects as a pandas table: CHR, the SNP's index, BETA and the posterior inclusion probability PIP."""
        import pandas as pd
        tables = ClumpThreshold.to_table(self, per_chromosome=True)
        for c in self.chromosomes:
            tables[c]["PIP"] = self.pip[c]
        return tables if per_chromosome else pd.concat([tables[c] for c in self.chromosomes])
