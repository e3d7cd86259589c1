"""``MergedPlanModel`` -- what the summary-statistics models on ONE device plan share: `ClumpThreshold` (and on it `Lassosum`,
`LDpred2`, `PRSCS`, `SBayesR`), `LDPredInf` and `SuSiE`.

The LD of every chromosome is loaded in sorted order (`load_ld_in_order`: never expanded on the device), merged into one set of
arrays (`merge_ld_arrays`; LD blocks never span chromosomes) and, unless a host hook replaces the device work, put into one
`LDPlan`.  A constructor is three steps: `_set_loader` (the loader checks), its own parameter checks, `_load`.  `_attach` is
`_load` for an `LDPlan` that exists already (`from_plan`).
"""
import numpy as np

from ..data import merge_ld_arrays
from ._ld_loading import LoadedLD, ld_form, load_ld_in_order, open_plan


class MergedPlanModel:

    def _set_loader(self, gdl, comm=None, not_sharded="sweep"):
        """Refuses a loader without summary statistics and LD, and more than one rank; keeps the loader and its shapes."""
        if gdl.genotype is None and (gdl.ld is None or gdl.sumstats_table is None):
            raise AssertionError("The data loader must contain summary statistics and LD matrices.")
        if comm is not None and comm.world_size > 1:
            raise NotImplementedError(f"{type(self).__name__} runs on one rank only (world_size > 1: the {not_sharded} is not "
                                      "sharded)")
        self.gdl = gdl
        self.shapes = {c: int(n) for c, n in gdl.shapes.items()}

    def _load(self, float_precision, low_memory, dequantize_on_the_fly, device, host, no_device, keep_ld=False,
              ld_correction=False, std_beta=True, n_per_snp=False):
        """The LD of `_set_loader`'s loader in host memory and, unless `host`, in one plan on HIP device `device` (`no_device`:
        the error without one; `device` stays unset on the host path).  `_ld` keeps the merged arrays on the host path and
        with `keep_ld`, else None.  `ld_correction`: the sample-size corrections of the LD scores are taken before any LD is
        loaded.  Returns ``(left_bound, indptr, data, correction or None)``."""
        gdl, chroms = self.gdl, self.chromosomes
        self.float_precision = float_precision
        self._T = np.dtype(float_precision)
        self.low_memory = bool(low_memory)
        ld_mats = gdl.get_ld_matrices()
        corr = self._ld_correction(ld_mats) if ld_correction else None
        loaded, self.dequantize_on_the_fly, self.dequantize_scale = load_ld_in_order(
            ld_mats, chroms, self.low_memory, dequantize_on_the_fly, float_precision, expand_ld_on_device=False)
        if std_beta:
            self.std_beta = {c: np.asarray(gdl.sumstats_table[c].get_snp_pseudo_corr()).astype(self._T) for c in chroms}
        if n_per_snp:
            self._n_per_snp = np.concatenate([np.asarray(gdl.sumstats_table[c].n_per_snp, dtype=np.float64).ravel()
                                              for c in chroms])
        lb, ip, data, self._seg = merge_ld_arrays(
            chroms, self.shapes, {c: ld.left_bound for c, ld in loaded.items()}, {c: ld.indptr for c, ld in loaded.items()},
            {c: ld.data for c, ld in loaded.items()})
        del loaded
        self._plan = None
        if not host:
            from .. import _lib                    # (looked up now, as `LDPlan` in `open_plan`: tests replace both)
            if _lib.device_count() < 1:
                raise RuntimeError(no_device)
            self.device = int(device) if device is not None else 0
            self._plan = open_plan(LoadedLD(lb, ip, data, ld_form(self.low_memory)), self.device)
        self._ld = (lb, ip, data) if host or keep_ld else None
        return lb, ip, data, corr

    def _attach(self, plan, dq_scale, std_beta, n_per_snp=None):
        """`_set_loader` and `_load` for an existing `LDPlan` (one chromosome; the LD may exist on the device only): `std_beta`
        float32 ``(m,)``, `n_per_snp` ``(m,)`` where the model takes it, `dq_scale` the plan's de-quantisation scale.  The
        plan stays the caller's."""
        from .. import _lib
        m = int(plan.m)
        std_beta = np.ascontiguousarray(std_beta, dtype=np.float32)
        if std_beta.shape != (m,) or (n_per_snp is not None and np.shape(n_per_snp) != (m,)):
            raise ValueError(f"std_beta, n_per_snp: arrays of shape ({m},)")
        self.gdl = type("PlanLoader", (), {"m": m, "shapes": {1: m}})
        self.shapes, self._seg = {1: m}, {1: (0, m)}
        self.float_precision, self._T = "float32", np.dtype(np.float32)
        self.low_memory = bool(plan.info(_lib.INFO_LOW_MEMORY))
        self.dequantize_on_the_fly, self.dequantize_scale = True, float(dq_scale)
        self.std_beta = {1: std_beta}
        if n_per_snp is not None:
            self._n_per_snp = np.asarray(n_per_snp, dtype=np.float64)
        self._plan, self._ld, self.device = plan, None, int(plan.info(_lib.INFO_DEVICE))

    def _ld_correction(self, ld_mats):
        from ..stats.ldsc import ld_correction
        return np.concatenate([ld_correction(ld_mats[c], self.shapes[c], where=f"chromosome {c}") for c in self.chromosomes])

    def _ldsc_h2(self, lb, ip, data, corr, score_fn):
        """`simple_ldsc` over the model's own LD: corrected unit-weight scores of its plan (the host path: `score_fn` or
        `ld_scores_host`), kept as `ld_score`, then the estimate over all chromosomes."""
        from ..stats.ldsc import ld_scores_host, ldsc_estimate_over
        if self._plan is not None and score_fn is None:
            scores = self._plan.ld_scores(None, corr, dq_scale=self.dequantize_scale, float_precision=self.float_precision)
        else:
            scores = (score_fn or ld_scores_host)(lb, ip, data, self.low_memory, None, corr, self.dequantize_scale)
        self.ld_score = self._split(np.asarray(scores, dtype=np.float64))
        return ldsc_estimate_over(self.gdl.sumstats_table, self.ld_score, self.chromosomes)

    @property
    def chromosomes(self):
        return sorted(self.shapes)

    @property
    def m(self):
        return int(self.gdl.m)

    n_snps = m

    def _split(self, x):
        """``{chromosome: its rows of x}``, copies, for an array over all SNPs."""
        return {c: np.array(x[a:e]) for c, (a, e) in self._seg.items()}

    def _concat(self, per_chromosome):
        """The inverse of `_split`: one array over all SNPs, the chromosomes in sorted order."""
        return np.concatenate([per_chromosome[c] for c in self.chromosomes])

    def get_posterior_mean_beta(self):
        return self.post_mean_beta

    def predict(self, test_gdl=None, **kw):
        """Polygenic scores of the training loader's genotyped samples, or of `test_gdl`'s, from the posterior mean effects
        (``(n, n_models)`` for a grid of models): `viprs_amd.genotypes.model_predict`."""
        from ..genotypes import model_predict
        return model_predict(self, test_gdl, **kw)
