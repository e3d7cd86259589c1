"""``PRSCS`` -- the continuous-shrinkage Gibbs sampler of Ge, Chen, Ni, Feng and Smoller (2019), with a fixed or a learnt
("auto") global scale ``phi``: the baseline nearly every summary-statistics PRS paper reports, on the sweep of `LDpred2`.

Every effect has a scale of its own, ``beta_j ~ N(0, sigma2 / n psi_j)`` with ``psi_j ~ Gamma(a, delta_j)`` and ``delta_j ~
Gamma(b, phi)``.  Given the scales the conditional of one effect is Gaussian: the LDpred2 Gibbs sweep with ``mu_mult = psi /
(1 + psi)``, ``half_var_tau = n_j (1 + 1 / psi) / (2 sigma2)`` and an inclusion probability of exactly 1
(`DeviceState.gibbs_sweep`, untouched).  Between two sweeps `DeviceState.cs_update` draws ``delta`` and ``psi`` of every (SNP,
chain) on the device and rewrites those inputs (`viprs_amd.stats.cs` is the host definition); the two scalars of a chain,
``sigma2`` and ``phi``, are drawn on the host from six sums.  The LD of every chromosome lives in one device plan and every
chain -- one per entry of `phi` -- is a column of ONE grid state: an iteration is one draws launch, one sweep launch, two
sums calls, one variates and one update launch, whatever the number of chains.  Result layout, `predict`,
`pseudo_validate`, `select_best` and `to_table` are `ClumpThreshold`'s: model ``g`` is the chain of ``phi[g]``.

What differs from the PRS-CS program:
  * an effect is drawn given all the others, SNP after SNP (single-site Gibbs), where PRS-CS draws an LD block jointly
    through a Cholesky factor: the same stationary distribution, another path to it;
  * ONE ``sigma2`` and ONE ``phi`` per chain over the whole genome, where PRS-CS runs chromosome by chromosome;
  * the sample size ``n_j`` of every SNP where PRS-CS takes one ``n`` (``nbar = mean(n_j)`` in the draw of ``sigma2``);
  * the posterior mean averages the conditional means ``mu_j`` of the kept iterations (Rao-Blackwellised), not the draws.

Only ``a = 1, b = 1/2`` (the defaults everyone runs): the closed-form draws need them.  A chain whose ``sum eta^2`` stops being
finite or exceeds ``sum beta_hat^2`` is ``diverged``: zero from there on, and out of the sweeps.  Not built: other ``a``,
``b``; joint-block draws; per-chromosome scalars; float64 states; several ranks.  The reference has no such class.
(``sweep_fn`` lets the CPU tests run the chain on the host with `viprs_amd.stats.gibbs.gibbs_sweep_host`; ``draws_fn`` /
``variates_fn`` replace the random numbers; without ``sweep_fn`` and without a GPU the constructor raises.)
"""
import numpy as np

from ._chain_engines import DeviceChains, HostChains, divergence_rule, tail_mean
from .ClumpThreshold import ClumpThreshold


class PRSCS(ClumpThreshold):

    def __init__(self, gdl, phi=None, a=1.0, b=0.5, n_iter=1000, n_burnin=500, thin=5, seed=0, psi_max=1.0,
                 float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, sweep_fn=None,
                 draws_fn=None, variates_fn=None, keep_draws_log=False, comm=None):
        """:param gdl: the data loader (summary statistics and LD matrices per chromosome).
        :param phi: the global scale: None (learnt, PRS-CS-auto), a number, or a sequence of numbers and None -- one chain
            per entry, all in lock step (the usual ``(1e-6, 1e-4, 1e-2, 1, None)`` is five columns of one state).
        :param a, b: the exponents of the gamma-gamma prior; only 1 and 1/2.
        :param n_iter, n_burnin, thin: iterations in all, those dropped first, and the stride of the kept ones.
        :param seed: of the device draws (Philox key) and of the host `Generator` of each chain.
        :param psi_max: the upper bound of the local scales (PRS-CS: 1).
        :param sweep_fn: test hook -- a callable with `viprs_amd.stats.gibbs.gibbs_sweep_host`'s signature: the chain runs on
            the host (called once per sweep with the live columns as ``(m, n_live)`` arrays).
        :param draws_fn: host path -- ``(seed, draw_index, half_var_tau, cols) -> (U, noise)`` in place of
            `viprs_amd.stats.gibbs.gibbs_draws_host`.
        :param variates_fn: host path -- ``(seed, draw_index, m, cols) -> (ub, z1, z2, e)``, each ``(m, len(cols))``, in
            place of `viprs_amd.stats.cs.cs_variates_host`.
        :param keep_draws_log: device path -- `draws_log[k]` keeps the ``(U, noise)`` of sweep k and `variates_log[k]` the
            ``(ub, z1, z2, e)`` of update k, ``(m, G)`` each (tests).
        """
        self._set_loader(gdl, comm)
        if float(a) != 1.0 or float(b) != 0.5:
            raise NotImplementedError("PRSCS: only a = 1, b = 0.5 (the closed-form draws of delta and psi need them)")
        if np.dtype(float_precision) != np.float32:
            raise ValueError("PRSCS: float_precision must be 'float32' (the Gibbs sweep has no float64 form)")
        self.a, self.b = 1.0, 0.5
        self.n_iter, self.n_burnin, self.thin = int(n_iter), int(n_burnin), int(thin)
        if not (0 <= self.n_burnin < self.n_iter) or self.thin < 1 or (self.n_iter - self.n_burnin) // self.thin < 1:
            raise ValueError("0 <= n_burnin < n_iter, thin >= 1 and at least one kept iteration")
        self.psi_max = float(psi_max)
        if not (2.0 ** -40 < self.psi_max < np.inf):
            raise ValueError("psi_max must lie in (2^-40, inf)")
        entries = list(phi) if isinstance(phi, (list, tuple, np.ndarray)) else [phi]
        if not entries:
            raise ValueError("phi: at least one entry")
        self.phi = [None if v is None else float(v) for v in entries]
        if any(v is not None and not (np.isfinite(v) and v > 0) for v in self.phi):
            raise ValueError("phi: positive numbers or None")
        self.n_models = len(self.phi)
        self.seed = int(seed)
        self._sweep_fn, self._draws_fn, self._variates_fn = sweep_fn, draws_fn, variates_fn
        self._keep_draws_log = bool(keep_draws_log)
        self.draws_log, self.variates_log = [], []
        self._load("float32", low_memory, dequantize_on_the_fly, device, sweep_fn is not None,
                   "PRSCS needs a HIP device (viprs_amd.stats.gibbs.gibbs_sweep_host is the sweep on the host: "
                   "pass it as sweep_fn)",
                   n_per_snp=True)
        self.post_mean_beta = None
        self.grid_table = None
        self.validation_result = None
        self.best_model_idx = None
        self.phi_est = self.sigma2_est = self.phi_history = self.sigma2_history = None

    # -- the two engines of a fit (`_chain_engines`): what PRS-CS adds is the update of the scales between two sweeps ---------
    class _Device(DeviceChains):
        def prepare(self, params):
            self.st.cs_update(params, self.model.psi_max, prepare_only=True, sync=False)

        def sums(self, active):
            return self.st.enet_sums(active), self.st.cs_sums(active)

        def update(self, params, draw_index):
            self.st.cs_update(params, self.model.psi_max, seed=self.model.seed, draw_index=draw_index, sync=False)
            if self.model._keep_draws_log:
                self.model.variates_log.append(tuple(self.st.cs_download(k) for k in ("ub", "z1", "z2", "e")))

    class _Host(HostChains):
        def __init__(self, model, beta, G):
            from ..stats.cs import cs_variates_host
            super().__init__(model, beta, G)
            self.variates = model._variates_fn or cs_variates_host
            self.delta = np.zeros((model.m, G), dtype=np.float32, order="F")
            self.psi = np.ones((model.m, G), dtype=np.float32, order="F")

        def _update(self, params, variates, prepare_only):
            from ..stats.cs import cs_update_host
            cs_update_host(self.model._n_per_snp, self._eta, self.psi, self.delta, self.mm, self.hvt, self.ulog, params,
                           self.model.psi_max, variates, prepare_only)

        def prepare(self, params):
            self._update(params, None, True)

        def sums(self, active):
            from ..stats.cs import cs_sums_host
            return super().sums(active), cs_sums_host(self.model._n_per_snp, self._eta, self.psi, self.delta, cols=active)

        def update(self, params, draw_index):
            cols = np.asarray(params)[:, 0].astype(np.int64)
            full = [np.zeros(self.psi.shape, dtype=np.float32, order="F") for _ in range(4)]
            for dst, src in zip(full, self.variates(self.model.seed, draw_index, self.model.m, cols)):
                src = np.asarray(src)
                dst[:, cols] = src[:, cols] if src.shape == dst.shape else src      # (m, G) from a log, or (m, len(cols))
            self._update(params, full, False)

    def fit(self):
        """The chains in lock step: `n_iter` iterations of (sweep, sums, the two scalar draws, update); after `n_burnin`
        every `thin`-th iteration adds its conditional means to the posterior mean."""
        import pandas as pd
        from ..stats.cs import cs_phi_draw, cs_sigma2_draw
        m = self.m
        beta_hat, diverges = divergence_rule(self)
        nbar = float(np.mean(self._n_per_snp))
        G = self.n_models
        auto = np.array([v is None for v in self.phi])
        phi = np.array([1.0 if v is None else v for v in self.phi], dtype=np.float64)
        sigma2 = np.ones(G, dtype=np.float64)
        # one generator per chain: a chain depends on its own entry of `phi` and on its position, not on the other entries
        rngs = [np.random.default_rng([self.seed, g]) for g in range(G)]
        diverged = np.zeros(G, dtype=bool)
        phi_hist, s2_hist = np.full((self.n_iter, G), np.nan), np.full((self.n_iter, G), np.nan)
        n_kept = 0
        self.draws_log, self.variates_log = [], []
        eng = (self._Host if self._sweep_fn is not None else self._Device)(self, beta_hat, G)
        rows = lambda cols: np.stack([np.asarray(cols, dtype=np.float64), sigma2[cols], phi[cols]], axis=1)
        try:
            eng.prepare(rows(np.arange(G)))
            for it in range(self.n_iter):
                active = np.flatnonzero(~diverged).astype(np.int32)
                if active.shape[0] == 0:
                    break
                enet, cs = eng.sweep(active, it)
                still = []
                for g, row, c in zip(active, enet, cs):
                    if diverges(row[3]):
                        diverged[g] = True
                        eng.zero_column(int(g))
                        continue
                    still.append(int(g))
                    quad = row[3] + row[2] + c[0]
                    sigma2[g] = cs_sigma2_draw(rngs[g], nbar, m, row[1], quad, c[1])
                    if auto[g]:
                        phi[g] = cs_phi_draw(rngs[g], m, self.b, phi[g], c[2])
                    phi_hist[it, g], s2_hist[it, g] = phi[g], sigma2[g]
                still = np.asarray(still, dtype=np.int32)
                if still.shape[0]:
                    eng.update(rows(still), it)
                kept = it + 1 > self.n_burnin and (it + 1 - self.n_burnin) % self.thin == 0
                if kept:
                    n_kept += 1
                    if still.shape[0]:
                        eng.accumulate(still)
            mean = eng.mean_sum() / float(max(n_kept, 1))
        finally:
            eng.close()
        mean[:, diverged] = 0.0
        beta = mean.astype(np.float32)
        self.phi_history, self.sigma2_history = phi_hist, s2_hist
        self.phi_est = tail_mean(phi_hist, self.n_burnin, diverged)
        self.sigma2_est = tail_mean(s2_hist, self.n_burnin, diverged)
        self.grid_table = pd.DataFrame(dict(phi=[np.nan if v is None else v for v in self.phi], auto=auto, phi_est=self.phi_est,
                                            sigma2_est=self.sigma2_est, diverged=diverged))
        self.validation_result = self.grid_table.copy()
        if G == 1:
            self.post_mean_beta = self._split(beta[:, 0])
            self.best_model_idx = 0                                 # one model: nothing to select
        else:
            self.post_mean_beta = self._split(beta)
            self.best_model_idx = None
        return self
