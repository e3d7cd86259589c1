"""``ClumpThreshold`` -- clumping and thresholding (C+T / P+T), the baseline of every PRS comparison, with its clumping on
MI355X.

For every LD threshold ``r2_g`` the SNPs are clumped greedily from the most significant down (`LDPlan.clump`,
`viprs_plan_clump`: all thresholds in ONE device call, one column each); model ``(r2_g, p_t)`` keeps the index SNPs of
column g with ``p <= p_t`` and gives them their standardised marginal effect, every other SNP 0.  The order of the one
clumping holds every SNP with ``p <= max(p_thresholds)``; greedy clumping is prefix-consistent in the order -- what a SNP
does depends only on the SNPs in front of it -- so the index SNPs with ``p <= p_t`` ARE the index SNPs of a clumping run
at ``p_t``.  p-values never appear: a threshold becomes the chi^2 cut-off ``scipy.stats.chi2.isf(p, 1)``.

The LD of every chromosome lives in one device plan, as for `LDPredInf`.  The reference has no such class; the layout of
the results follows its grid models (``post_mean_beta[c]`` of shape ``(m_c, n_models)``, ``grid_table``,
``validation_result``).  It runs on one rank only.  (``clump_fn`` lets the CPU tests drive the host logic with
`viprs_amd.stats.clump.clump_host`; without it and without a GPU the constructor raises.)
"""
import numpy as np

from ._merged_plan import MergedPlanModel


class ClumpThreshold(MergedPlanModel):

    def __init__(self, gdl, r2=(0.1, 0.2, 0.5, 0.8), p_thresholds=(5e-8, 1e-6, 1e-4, 1e-3, 1e-2, 0.05, 0.1, 0.5, 1.0),
                 float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, clump_fn=None,
                 comm=None):
        """:param gdl: the data loader (summary statistics and LD matrices per chromosome).
        :param r2: the LD thresholds of the clumping, 1..32 values: one clumping per value.
        :param p_thresholds: the p-value thresholds of the index SNPs; the grid is ``r2 x p_thresholds``, r2 outermost.
        :param float_precision: dtype of the effects, 'float32' or 'float64'.
        :param low_memory: load the upper-triangular form of the LD matrices (never expanded on the device, as `LDPredInf`).
        :param dequantize_on_the_fly: keep integer LD in its stored dtype on the device (threaded through the chromosomes
            in sorted order, as in `VIPRS`).
        :param device: HIP device index (default 0).
        :param clump_fn: test hook -- a callable with `viprs_amd.stats.clump.clump_host`'s signature that replaces the
            device clumping.
        """
        self._set_loader(gdl, comm, not_sharded="clumping")
        self.r2 = np.atleast_1d(np.asarray(r2, dtype=np.float64))
        self.p_thresholds = np.atleast_1d(np.asarray(p_thresholds, dtype=np.float64))
        if self.r2.ndim != 1 or not 1 <= self.r2.shape[0] <= 32 or not np.all(np.isfinite(self.r2)) or np.any(self.r2 < 0):
            raise ValueError("r2: 1..32 finite thresholds >= 0")
        if self.p_thresholds.ndim != 1 or self.p_thresholds.shape[0] < 1 or np.any(~(self.p_thresholds > 0)):
            raise ValueError("p_thresholds: at least one threshold, each > 0")
        self._clump_fn = clump_fn
        self._load(float_precision, low_memory, dequantize_on_the_fly, device, clump_fn is not None,
                   "ClumpThreshold needs a HIP device (viprs_amd.stats.clump.clump runs on the host)")
        self.n_models = int(self.r2.shape[0] * self.p_thresholds.shape[0])
        self.index_of = None
        self.post_mean_beta = None
        self.grid_table = None
        self.validation_result = None
        self.best_model_idx = None

    def _chisq(self):
        from ..stats.ldsc import chisq_statistic
        return np.concatenate([chisq_statistic(self.gdl.sumstats_table[c]) for c in self.chromosomes])

    def fit(self):
        """One clumping per `r2` value in one call over the merged plan, then the grid of effects: model ``g * n_p + t``
        keeps the index SNPs of column g with ``chi2 >= chi2.isf(p_thresholds[t], 1)``."""
        import pandas as pd
        from ..stats.clump import chisq_cutoff, clump_order
        chisq = self._chisq()
        cuts = np.array([chisq_cutoff(p) for p in self.p_thresholds])
        order = clump_order(chisq, cuts.min())
        if self._clump_fn is not None:
            lb, ip, data = self._ld
            index_of = self._clump_fn(lb, ip, data, self.low_memory, order, self.r2, None, self.dequantize_scale)
        else:
            index_of = self._plan.clump(order, self.r2, dq_scale=self.dequantize_scale)
        index_of = np.asarray(index_of).reshape(self.m, self.r2.shape[0])
        is_index = index_of == np.arange(self.m, dtype=index_of.dtype)[:, None]
        b = self._concat(self.std_beta)
        n_p = cuts.shape[0]
        beta = np.zeros((self.m, self.n_models), dtype=self._T)
        for g in range(self.r2.shape[0]):
            for t in range(n_p):
                keep = is_index[:, g] & (chisq >= cuts[t])
                beta[keep, g * n_p + t] = b[keep]
        self.index_of = self._split(index_of)
        self.post_mean_beta = self._split(beta)
        self.grid_table = pd.DataFrame({"r2": np.repeat(self.r2, n_p), "p_threshold": np.tile(self.p_thresholds, self.r2.shape[0]),
                                        "n_snps": np.count_nonzero(beta, axis=0)})
        self.validation_result = self.grid_table.copy()
        self.best_model_idx = None
        return self

    def pseudo_validate(self, validation_std_beta=None, validation_ld=None):
        """Pseudo-R^2 ``(r'b)^2 / (b'Rb)`` of every model against standardised marginal betas of an independent cohort
        (`viprs_amd.eval.pseudo_metrics`); ``R b`` is the LD product of the model's own plan, or of `validation_ld` (as in
        `VIPRS.pseudo_validate`).  A model without SNPs gives nan."""
        from ..eval.pseudo_metrics import pseudo_r2
        assert self.post_mean_beta is not None, "The effects are not set. Call `.fit()` first."
        vb = validation_std_beta if validation_std_beta is not None else getattr(self, "validation_std_beta", None)
        assert vb is not None, "standardized betas of a validation set are required"
        if validation_ld is not None:
            from .VIPRS import _pseudo_r2_external
            return _pseudo_r2_external(validation_ld, vb, self.post_mean_beta, device=getattr(self, "device", 0))
        chroms = self.chromosomes
        r = np.concatenate([np.asarray(vb[c], dtype=np.float64) for c in chroms])
        beta = self._concat(self.post_mean_beta)
        if self._plan is not None:
            return pseudo_r2(self._plan, r, beta, dq_scale=self.dequantize_scale)
        lb, ip, data = self._ld                                # (host path: R b in float64 from the arrays)
        dot = lambda _ld, b: _host_dot(lb, ip, data, self.low_memory, np.asarray(b, dtype=np.float64).reshape(self.m, -1),
                                       self.dequantize_scale).reshape(np.shape(b))
        return pseudo_r2(None, r, beta, dot_fn=dot)

    def select_best(self, validation_gdl=None, criterion="validation"):
        """Keeps the model with the highest R^2 of its polygenic score on `validation_gdl`'s genotypes against its
        phenotype (``criterion="validation"``) or the highest pseudo-R^2 against its summary statistics (``"pseudo_validation"``;
        `validation_gdl` as in `select_best_model`).  ``post_mean_beta[c]`` becomes ``(m_c,)``; ``validation_result`` keeps
        the scores of all models, ``best_model_idx`` the choice."""
        from .gridsearch.grid_utils import _validation_phenotype, _validation_r2, _validation_std_beta
        if criterion not in ("validation", "pseudo_validation"):
            raise AssertionError(f"unknown criterion {criterion!r}")
        assert self.post_mean_beta is not None, "The effects are not set. Call `.fit()` first."
        if self.best_model_idx is not None:
            return self
        if criterion == "validation":
            y = _validation_phenotype(validation_gdl)
            score = _validation_r2(self.predict(test_gdl=validation_gdl), y)
            self.validation_result["Validation_R2"] = score
        else:
            vb = _validation_std_beta(self, validation_gdl)
            score = np.nan_to_num(np.asarray(self.pseudo_validate(vb), dtype=np.float64), nan=0.0, neginf=0.0, posinf=0.0)
            self.validation_result["Pseudo_Validation_R2"] = score
        best = int(np.argmax(score))
        self.post_mean_beta = {c: np.ascontiguousarray(b[:, best]) for c, b in self.post_mean_beta.items()}
        self.best_model_idx = best
        self.n_models = 1
        return self

    def to_table(self, per_chromosome=False):
        """The effects as a pandas table: CHR, the SNP's index, then BETA (``BETA_0, BETA_1, ...`` for the grid)."""
        import pandas as pd
        if self.post_mean_beta is None:
            raise Exception("The effects are not set. Call `.fit()` first.")
        tables = {}
        for c in self.chromosomes:
            b = self.post_mean_beta[c]
            cols = {"CHR": c, "IDX": np.arange(b.shape[0])}
            cols.update({"BETA": b} if b.ndim == 1 else {f"BETA_{i}": b[:, i] for i in range(b.shape[1])})
            tables[c] = pd.DataFrame(cols)
        return tables if per_chromosome else pd.concat([tables[c] for c in self.chromosomes])


def _host_dot(lb, ip, data, low_memory, B, dq_scale):
    """``R B`` with the unit diagonal in float64 from the arrays (the layout of `LDPlan`): the host path of `pseudo_validate`."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    x = float(dq_scale) * np.asarray(data, dtype=np.float64)
    Y = B.copy()
    for j in range(lb.shape[0]):
        s, e = int(ip[j]), int(ip[j + 1])
        if e == s:
            continue
        cols = int(lb[j]) + np.arange(e - s)
        r = x[s:e]
        if not low_memory:
            keep = cols != j
            cols, r = cols[keep], r[keep]
        Y[j] += r @ B[cols]
        if low_memory:
            Y[cols] += r[:, None] * B[j]
    return Y
