"""``LDpred2`` -- the Gibbs sampler of Prive, Arbel and Vilhjalmsson (2020), ``-grid`` and ``-auto``: the baseline most
summary-statistics PRS papers report first, with its sweep on MI355X.

Every chain draws each effect from its conditional posterior under a point-normal prior (proportion of causal variants
``p``, heritability ``h2``), SNP after SNP over each LD block (`DeviceState.gibbs_sweep`: the grid-column E-step's serial
sweep with a draw where the E-step stores an expectation; `viprs_amd.stats.gibbs` is its host definition), and averages the
Rao-Blackwellised means ``gamma mu`` after the burn-in (`DeviceState.gibbs_accumulate`).  The LD of every chromosome lives
in one device plan and every chain is a column of ONE grid state: an iteration is one draws launch, one sweep launch, one
`enet_sums` call (the number of non-zero effects, ``sum q eta``, ``sum eta^2``) and, after the burn-in, one accumulate launch,
whatever the number of chains.

``mode="grid"``: one chain per ``(p, h2)`` pair (model ``i_h2 * n_p + i_p``), result layout, `predict`, `pseudo_validate`,
`select_best` and `to_table` of `ClumpThreshold`.  ``mode="auto"``: `n_chains` chains that re-draw ``p ~ Beta(1 + n_nonzero,
1 + m - n_nonzero)`` and set ``h2 = max(b'Rb, 1e-4)`` (``b'Rb = sum eta^2 + sum q eta``: q is kept in units of the
de-quantised LD) after every sweep; the effect is the mean over the chains that did not diverge and whose ``h2`` lies within
3 scaled MADs of the median.  A chain whose ``sum eta^2`` stops being finite or exceeds ``sum beta_hat^2`` is ``diverged``:
zero from there on, and out of the sweeps.

Not built: LDpred2's ``sparse`` option; ``allow_jump_sign`` / ``use_MLE`` / ``shrink_corr`` of later bigsnpr versions;
float64 and mixture states; several ranks; a ``math_mode="fast"`` variant.  The reference has no such class.  (``sweep_fn``
lets the CPU tests drive the host logic with `viprs_amd.stats.gibbs.gibbs_sweep_host`, ``draws_fn`` replaces the draws;
without ``sweep_fn`` and without a GPU the constructor raises.)
"""
import numpy as np

from ._chain_engines import DeviceChains, HostChains, divergence_rule, tail_mean
from .ClumpThreshold import ClumpThreshold

GRID_P = tuple(float(v) for v in np.exp(np.linspace(np.log(1e-4), 0.0, 17)))
GRID_H2_MULTIPLIERS = (0.3, 0.7, 1.0, 1.4)
MAD_SCALE = 1.4826                                  # MAD of a normal sample -> its standard deviation


class LDpred2(ClumpThreshold):

    def __init__(self, gdl, mode="grid", p=None, h2=None, h2_init="ldsc", burn_in=None, num_iter=None, n_chains=30, seed=0,
                 float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, sweep_fn=None,
                 draws_fn=None, score_fn=None, keep_draws_log=False, comm=None):
        """:param gdl: the data loader (summary statistics and LD matrices per chromosome).
        :param mode: 'grid' or 'auto'.
        :param p: grid: the proportions of causal variants (default: 17 log-spaced values from 1e-4 to 1); auto: the
            initial value of every chain (default: `n_chains` log-spaced values from 1e-4 to 0.2).
        :param h2: grid: the heritabilities (default: 0.3, 0.7, 1 and 1.4 times the `h2_init` estimate); auto: unused.
        :param h2_init: 'ldsc' (the LD-score regression estimate over the model's own LD, as `LDPredInf(h2=None)`) or a
            number: the centre of the default grid, the initial h2 of every auto chain.
        :param burn_in, num_iter: sweeps before and while the means are accumulated (grid: 50 / 100, auto: 500 / 200).
        :param n_chains: auto: the number of chains.
        :param seed: of the device draws (Philox key) and of the host `Generator` that draws p.
        :param sweep_fn: test hook -- a callable with `viprs_amd.stats.gibbs.gibbs_sweep_host`'s signature that replaces
            the device sweep (called once per sweep with the live columns as ``(m, n_live)`` arrays).
        :param draws_fn: host path -- a callable ``(seed, draw_index, half_var_tau, cols) -> (U, noise)`` in place of
            `viprs_amd.stats.gibbs.gibbs_draws_host`.
        :param score_fn: as in `LDPredInf`: the LD scores of ``h2_init='ldsc'``.
        :param keep_draws_log: device path -- `draws_log[k]` keeps the ``(U, noise)`` sweep k used (tests).
        """
        self._set_loader(gdl, comm)
        self._configure(mode, burn_in, num_iter, seed, float_precision, sweep_fn, draws_fn, keep_draws_log)
        ldsc = isinstance(h2_init, str)
        if ldsc and h2_init != "ldsc":
            raise ValueError(f"h2_init: 'ldsc' or a number, got {h2_init!r}")
        lb, ip, data, corr = self._load(
            "float32", low_memory, dequantize_on_the_fly, device, sweep_fn is not None,
            "LDpred2 needs a HIP device (viprs_amd.stats.gibbs.gibbs_sweep_host is the sweep on the host: "
            "pass it as sweep_fn)", ld_correction=ldsc, n_per_snp=True)
        self._set_chains(self._ldsc_h2(lb, ip, data, corr, score_fn) if ldsc else h2_init, p, h2, n_chains)

    def _configure(self, mode, burn_in, num_iter, seed, float_precision, sweep_fn, draws_fn, keep_draws_log):
        """What a fit needs beside the data and the chains: checked and stored by both constructors."""
        if np.dtype(float_precision) != np.float32:
            raise ValueError("LDpred2: float_precision must be 'float32' (the Gibbs sweep has no float64 form)")
        if mode not in ("grid", "auto"):
            raise ValueError(f"mode: 'grid' or 'auto', got {mode!r}")
        self.mode = mode
        self.burn_in = int(burn_in if burn_in is not None else (50 if mode == "grid" else 500))
        self.num_iter = int(num_iter if num_iter is not None else (100 if mode == "grid" else 200))
        if self.burn_in < 0 or self.num_iter < 1:
            raise ValueError("burn_in >= 0 and num_iter >= 1")
        self.seed = int(seed)
        self._sweep_fn, self._draws_fn = sweep_fn, draws_fn
        self._keep_draws_log = bool(keep_draws_log)
        self.draws_log = []
        self.post_mean_beta = None
        self.grid_table = None
        self.validation_result = None
        self.best_model_idx = None
        self.p_est = self.h2_est = self.p_history = self.h2_history = self.chain_beta = self.chains_kept = None

    def _set_chains(self, h2_init, p, h2, n_chains):
        """The ``(p, h2)`` every chain starts from (grid: stays at), around `h2_init`."""
        self.h2_init = float(h2_init)
        if not self.h2_init > 0.0:
            raise ValueError(f"h2_init = {self.h2_init!r}: a positive heritability is needed")
        if self.mode == "grid":
            self.p = np.atleast_1d(np.asarray(GRID_P if p is None else p, dtype=np.float64))
            self.h2 = np.atleast_1d(np.asarray([f * self.h2_init for f in GRID_H2_MULTIPLIERS] if h2 is None else h2,
                                               dtype=np.float64))
            if not (np.all((self.p > 0) & (self.p <= 1)) and np.all(self.h2 > 0)):
                raise ValueError("p: values in (0, 1]; h2: values > 0")
            self.chain_p = np.tile(self.p, self.h2.shape[0])
            self.chain_h2 = np.repeat(self.h2, self.p.shape[0])
            self.n_models = int(self.chain_p.shape[0])
        else:
            self.n_chains = int(n_chains)
            if self.n_chains < 1:
                raise ValueError("n_chains >= 1")
            self.chain_p = np.atleast_1d(np.asarray(
                np.exp(np.linspace(np.log(1e-4), np.log(0.2), self.n_chains)) if p is None else p, dtype=np.float64))
            if self.chain_p.shape != (self.n_chains,) or not np.all((self.chain_p > 0) & (self.chain_p <= 1)):
                raise ValueError("p: one initial value in (0, 1] per chain")
            self.chain_h2 = np.full(self.n_chains, self.h2_init)
            self.n_models = 1

    @classmethod
    def from_plan(cls, plan, std_beta, n_per_snp, dq_scale, h2_init, mode="grid", p=None, h2=None, burn_in=None, num_iter=None,
                  n_chains=30, seed=0, keep_draws_log=False):
        """A model on an existing `LDPlan` (`MergedPlanModel._attach`: one chromosome, the LD may exist on the device only);
        `h2_init` a number.  Device sweep only; the plan stays the caller's."""
        self = cls.__new__(cls)
        self._configure(mode, burn_in, num_iter, seed, "float32", None, None, keep_draws_log)
        self._attach(plan, dq_scale, std_beta, n_per_snp)
        self._set_chains(h2_init, p, h2, n_chains)
        return self

    # -- the two engines of a fit (`_chain_engines`): what LDpred2 adds is how (p, h2) become the inputs of a sweep ----------
    class _Device(DeviceChains):
        def prep(self, cols, p, h2):
            from ..stats.gibbs import gibbs_prep_rows
            self.st.prep_columns(gibbs_prep_rows(cols, self.model.m, p, h2))

    class _Host(HostChains):
        def prep(self, cols, p, h2):
            from ..stats.gibbs import gibbs_prep_host
            for g, pg, hg in zip(cols, p, h2):
                self.mm[:, g], self.hvt[:, g], self.ulog[:, g] = gibbs_prep_host(self.model._n_per_snp, self.model.m, pg, hg)

    def fit(self):
        """The chains in lock step: `burn_in` sweeps, then `num_iter` sweeps whose Rao-Blackwellised means are averaged."""
        import pandas as pd
        m = self.m
        beta_hat, diverges = divergence_rule(self)
        G = int(self.chain_p.shape[0])
        auto = self.mode == "auto"
        p, h2 = self.chain_p.copy(), self.chain_h2.copy()
        rng = np.random.default_rng(self.seed)
        total = self.burn_in + self.num_iter
        diverged = np.zeros(G, dtype=bool)
        p_hist, h2_hist = np.full((total, G), np.nan), np.full((total, G), np.nan)
        n_nonzero = np.zeros(G, dtype=np.int64)
        self.draws_log = []
        eng = (self._Host if self._sweep_fn is not None else self._Device)(self, beta_hat, G)
        try:
            eng.prep(np.arange(G), p, h2)
            for it in range(total):
                active = np.flatnonzero(~diverged).astype(np.int32)
                if active.shape[0] == 0:
                    break
                sums = eng.sweep(active, it)
                still = []
                for g, row in zip(active, sums):
                    if diverges(row[3]):
                        diverged[g] = True
                        eng.zero_column(int(g))
                        continue
                    still.append(int(g))
                    n_nonzero[g] = int(row[5])
                    if auto:                                        # (one draw per live chain and sweep, in chain order)
                        p[g] = min(max(rng.beta(1.0 + row[5], 1.0 + m - row[5]), 1e-12), 1.0)
                        h2[g] = max(float(row[3] + row[2]), 1e-4)
                    p_hist[it, g], h2_hist[it, g] = p[g], h2[g]
                still = np.asarray(still, dtype=np.int32)
                if it >= self.burn_in and still.shape[0]:
                    eng.accumulate(still)
                if auto and still.shape[0] and it + 1 < total:
                    eng.prep(still, p[still], h2[still])
            mean = eng.mean_sum() / float(self.num_iter)
        finally:
            eng.close()
        mean[:, diverged] = 0.0
        beta = mean.astype(np.float32)
        self.p_history, self.h2_history = p_hist, h2_hist
        self.p_est = tail_mean(p_hist, self.burn_in, diverged)
        self.h2_est = tail_mean(h2_hist, self.burn_in, diverged)
        rows = dict(p=self.chain_p if not auto else self.p_est, h2=self.chain_h2 if not auto else self.h2_est,
                    diverged=diverged, n_nonzero=np.where(diverged, 0, n_nonzero))
        if auto:
            keep = ~diverged
            if keep.any():
                med = float(np.median(self.h2_est[keep]))
                mad = MAD_SCALE * float(np.median(np.abs(self.h2_est[keep] - med)))
                keep &= np.abs(np.where(diverged, np.inf, self.h2_est) - med) <= 3.0 * mad
            self.chains_kept = keep
            self.chain_beta = self._split(beta)
            final = (mean[:, keep].mean(axis=1) if keep.any() else np.zeros(m)).astype(np.float32)
            self.post_mean_beta = self._split(final)
            rows["kept"] = keep
            self.best_model_idx = 0                                 # one model: nothing to select
        else:
            self.post_mean_beta = self._split(beta)
            self.best_model_idx = None
        self.grid_table = pd.DataFrame(rows)
        self.validation_result = self.grid_table.copy()
        return self
