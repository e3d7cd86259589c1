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

from ..data import merge_ld_arrays
from ._ld_loading import LoadedLD, ld_form, load_ld_in_order, open_plan
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
        if gdl.genotype is None and (gdl.ld is None or gdl.sumstats_table is None):
            raise AssertionError("The data loader must contain summary statistics and LD matrices.")
        if comm is not None and comm.world_size > 1:
            raise NotImplementedError("LDpred2 runs on one rank only (world_size > 1: the sweep is not sharded)")
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
        self.gdl = gdl
        self.float_precision = "float32"
        self._T = np.dtype(np.float32)
        self.low_memory = bool(low_memory)
        self._sweep_fn, self._draws_fn = sweep_fn, draws_fn
        self._keep_draws_log = bool(keep_draws_log)
        self.draws_log = []
        self.shapes = {c: int(n) for c, n in gdl.shapes.items()}
        chroms = self.chromosomes
        ld_mats = gdl.get_ld_matrices()
        corr = None
        if isinstance(h2_init, str):
            if h2_init != "ldsc":
                raise ValueError(f"h2_init: 'ldsc' or a number, got {h2_init!r}")
            from ..stats.ldsc import ld_correction
            corr = np.concatenate([ld_correction(ld_mats[c], self.shapes[c], where=f"chromosome {c}") for c in chroms])
        loaded, self.dequantize_on_the_fly, self.dequantize_scale = load_ld_in_order(
            ld_mats, chroms, self.low_memory, dequantize_on_the_fly, float_precision, expand_ld_on_device=False)
        self.std_beta = {c: np.asarray(gdl.sumstats_table[c].get_snp_pseudo_corr()).astype(self._T) for c in chroms}
        self._n_per_snp = np.concatenate([np.asarray(gdl.sumstats_table[c].n_per_snp, dtype=np.float64).ravel() for c in chroms])
        # one plan over the concatenated chromosomes (LD blocks never span chromosomes)
        lb, ip, data, self._seg = merge_ld_arrays(
            chroms, self.shapes, {c: ld.left_bound for c, ld in loaded.items()}, {c: ld.indptr for c, ld in loaded.items()},
            {c: ld.data for c, ld in loaded.items()})
        del loaded
        self._plan = None
        self._ld = (lb, ip, data)                               # (the host path of the sweep and of `pseudo_validate`)
        if sweep_fn is None:
            from .. import _lib
            if _lib.device_count() < 1:
                raise RuntimeError("LDpred2 needs a HIP device (viprs_amd.stats.gibbs.gibbs_sweep_host is the sweep on the host: "
                                   "pass it as sweep_fn)")
            self.device = int(device) if device is not None else 0
            self._plan = open_plan(LoadedLD(lb, ip, data, ld_form(self.low_memory)), self.device)
        self.h2_init = self._ldsc_h2(lb, ip, data, corr, score_fn) if isinstance(h2_init, str) else float(h2_init)
        if not self.h2_init > 0.0:
            raise ValueError(f"h2_init = {self.h2_init!r}: a positive heritability is needed")
        if self._plan is not None:
            self._ld = None
        if mode == "grid":
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
        self.post_mean_beta = None
        self.grid_table = None
        self.validation_result = None
        self.best_model_idx = None
        self.p_est = self.h2_est = self.p_history = self.h2_history = self.chain_beta = self.chains_kept = None

    def _ldsc_h2(self, lb, ip, data, corr, score_fn):
        from ..stats.ldsc import ld_scores_host, ldsc_estimate_over
        if self._plan is not None and score_fn is None:
            scores = self._plan.ld_scores(None, corr, dq_scale=self.dequantize_scale, float_precision="float32")
        else:
            scores = (score_fn or ld_scores_host)(lb, ip, data, self.low_memory, None, corr, self.dequantize_scale)
        self.ld_score = {c: np.asarray(scores[a:e], dtype=np.float64) for c, (a, e) in self._seg.items()}
        return float(ldsc_estimate_over(self.gdl.sumstats_table, self.ld_score, self.chromosomes))

    # -- the two engines of a fit: a grid state on the device, or arrays swept by the hook -----------------------------------
    class _Device:
        def __init__(self, model, beta, G):
            from ..plan import DeviceState
            self.model, self.dq = model, model.dequantize_scale
            self.st = DeviceState(model._plan, "float32", model="grid", width=G, placement="off")
            self.st.upload("std_beta", beta)
            self.st.set_n_per_snp(model._n_per_snp)
            self.st.gibbs_reset_mean()

        def prep(self, cols, p, h2):
            from ..stats.gibbs import gibbs_prep_rows
            self.st.prep_columns(gibbs_prep_rows(cols, self.model.m, p, h2))

        def sweep(self, active, draw_index):
            self.st.gibbs_sweep(self.dq, active_model_idx=active, seed=self.model.seed, draw_index=draw_index, sync=False)
            sums = self.st.enet_sums(active)
            if self.model._keep_draws_log:
                self.model.draws_log.append((self.st.gibbs_download("unif"), self.st.gibbs_download("noise")))
            return sums

        def accumulate(self, active):
            self.st.gibbs_accumulate(active)

        def mean_sum(self):
            return self.st.gibbs_download("mean_sum")

        def zero_column(self, g):
            for k in ("eta", "q"):
                a = self.st.download(k)
                a[:, g] = 0
                self.st.upload(k, a)

        def close(self):
            self.st.close()

    class _Host:
        def __init__(self, model, beta, G):
            from ..stats.gibbs import gibbs_draws_host
            self.model, self.beta, self.dq = model, beta, model.dequantize_scale
            self.draws = model._draws_fn or gibbs_draws_host
            shape = (model.m, G)
            self.mm, self.hvt, self.ulog, self._eta, self.q, self.ed, self.mu, self.gam = (
                np.zeros(shape, dtype=np.float32, order="F") for _ in range(8))
            self.mean = np.zeros(shape, dtype=np.float64, order="F")

        def prep(self, cols, p, h2):
            from ..stats.gibbs import gibbs_prep_host
            for g, pg, hg in zip(cols, p, h2):
                self.mm[:, g], self.hvt[:, g], self.ulog[:, g] = gibbs_prep_host(self.model._n_per_snp, self.model.m, pg, hg)

        def sweep(self, active, draw_index):
            from ..stats.enet import enet_sums_host
            lb, ip, data = self.model._ld
            unif, noise = self.draws(self.model.seed, draw_index, self.hvt, np.asarray(active))
            a = np.asarray(active)
            pick = lambda x: np.asfortranarray(x[:, a])
            eta, q = pick(self._eta), pick(self.q)
            res = self.model._sweep_fn(lb, ip, data, self.model.low_memory, self.beta, pick(self.mm), pick(self.hvt),
                                       pick(self.ulog), pick(unif), pick(noise), eta, q, self.dq)
            for dst, src in zip((self.ed, self.mu, self.gam, self._eta, self.q), tuple(res) + (eta, q)):
                dst[:, a] = src
            return enet_sums_host(self.beta, self.hvt, self._eta, self.q, self.ed, cols=active, grid=True)

        def accumulate(self, active):
            for g in active:
                self.mean[:, g] += self.gam[:, g].astype(np.float64) * self.mu[:, g].astype(np.float64)

        def mean_sum(self):
            return self.mean.copy()

        def zero_column(self, g):
            self._eta[:, g] = 0
            self.q[:, g] = 0

        def close(self):
            pass

    def fit(self):
        """The chains in lock step: `burn_in` sweeps, then `num_iter` sweeps whose Rao-Blackwellised means are averaged."""
        import pandas as pd
        m = self.m
        beta_hat = np.concatenate([self.std_beta[c] for c in self.chromosomes])
        limit = float(beta_hat.astype(np.float64) @ beta_hat.astype(np.float64))
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
                    if not np.isfinite(row[3]) or row[3] > limit:
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
        with np.errstate(invalid="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                self.p_est = np.where(diverged, np.nan, np.nanmean(p_hist[self.burn_in:], axis=0))
                self.h2_est = np.where(diverged, np.nan, np.nanmean(h2_hist[self.burn_in:], axis=0))
        rows = dict(p=self.chain_p if not auto else self.p_est, h2=self.chain_h2 if not auto else self.h2_est,
                    diverged=diverged, n_nonzero=np.where(diverged, 0, n_nonzero))
        if auto:
            keep = ~diverged
            if keep.any():
                med = float(np.median(self.h2_est[keep]))
                mad = MAD_SCALE * float(np.median(np.abs(self.h2_est[keep] - med)))
                keep &= np.abs(np.where(diverged, np.inf, self.h2_est) - med) <= 3.0 * mad
            self.chains_kept = keep
            self.chain_beta = {c: np.array(beta[a:e]) for c, (a, e) in self._seg.items()}
            final = (mean[:, keep].mean(axis=1) if keep.any() else np.zeros(m)).astype(np.float32)
            self.post_mean_beta = {c: np.array(final[a:e]) for c, (a, e) in self._seg.items()}
            rows["kept"] = keep
            self.best_model_idx = 0                                 # one model: nothing to select
        else:
            self.post_mean_beta = {c: np.array(beta[a:e]) for c, (a, e) in self._seg.items()}
            self.best_model_idx = None
        self.grid_table = pd.DataFrame(rows)
        self.validation_result = self.grid_table.copy()
        return self
