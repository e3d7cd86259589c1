"""``LDPredInf`` -- the infinitesimal (ridge) PRS model with its solve on MI355X.

The reference's class (viprs/model/LDPredInf.py) assembles one block-diagonal sparse matrix over all chromosomes and hands
``(R + lam I) beta = beta_hat`` to scipy's ``minres``.  Here the LD of every chromosome lives in ONE device plan and the
system is solved LD block by LD block, all blocks in lock step (``LDPlan.solve_ridge``): the converged solution is the
same, every block stops on its own residual.

One deviation from the reference, on purpose: the right-hand side is the vector of STANDARDISED marginal effects
(``get_snp_pseudo_corr()``), as for every model of this package -- the reference passes ``marginal_beta``, which is on the
scale of ``R`` only for standardised genotypes.

``h2=None`` estimates the heritability as the reference does (LDPredInf.py:32-33, ``simple_ldsc``): the LD scores of the
model's own plan (``LDPlan.ld_scores`` with the sample-size correction), then ``viprs_amd.stats.ldsc``'s estimate.

There is no CPU fallback: without ``libviprs_hip.so`` and a GPU ``fit()`` raises.  (``solve_fn`` lets the CPU tests drive
this host logic with the host model of the solver; it is never set by the package itself.)
"""
import warnings

import numpy as np

from ..data import merge_ld_arrays
from ._ld_loading import LoadedLD, ld_form, load_ld_in_order, open_plan


class LDPredInf:

    def __init__(self, gdl, h2=None, float_precision="float32", low_memory=True, dequantize_on_the_fly=False,
                 device=None, solve_fn=None, comm=None, score_fn=None):
        """:param gdl: the data loader (summary statistics and LD matrices per chromosome).
        :param h2: heritability of the trait (a number in (0, 1]); None: the LD-score regression estimate
            (`viprs_amd.stats.ldsc.simple_ldsc` with corrected LD scores; needs the LD objects' ``sample_size``).
        :param float_precision: precision of the solve, 'float32' or 'float64'.
        :param low_memory: load the upper-triangular form of the LD matrices.  The LD is never expanded on the device:
            with ``low_memory=False`` a matrix that holds only the upper-triangular store raises its ValueError.
        :param dequantize_on_the_fly: keep integer LD in its stored dtype on the device.  Threaded through the chromosomes
            in sorted order, as in `VIPRS`: the first float-stored chromosome turns it off for all later ones, and
            ``dequantize_scale`` comes from the FIRST chromosome's matrix.
        :param device: HIP device index (default 0).
        :param solve_fn: test hook -- a callable ``(lb, ip, data, low_memory, b, shift, dq_scale, rtol, maxiter, x0) ->
            (x, info)`` that replaces the device solve.
        :param score_fn: test hook -- a callable with `viprs_amd.stats.ldsc.ld_scores_host`'s signature that computes the
            LD scores of ``h2=None`` (the default on the host path: `ld_scores_host` itself).
        """
        if gdl.genotype is None and (gdl.ld is None or gdl.sumstats_table is None):
            raise AssertionError("The data loader must contain summary statistics and LD matrices.")
        if comm is not None and comm.world_size > 1:
            raise NotImplementedError("LDPredInf runs on one rank only (world_size > 1: the solve is not sharded)")
        self.gdl = gdl
        self.h2 = h2
        self.float_precision = float_precision
        self._T = np.dtype(float_precision)
        self.low_memory = bool(low_memory)
        self._solve_fn = solve_fn
        self.shapes = {c: int(s) for c, s in gdl.shapes.items()}
        self._sample_size = max(float(np.max(s.n_per_snp)) for s in gdl.sumstats_table.values())

        ld_mats = gdl.get_ld_matrices()
        chroms = self.chromosomes
        corr = None
        if h2 is None:
            from ..stats.ldsc import ld_correction
            try:
                corr = np.concatenate([ld_correction(ld_mats[c], self.shapes[c], where=f"chromosome {c}") for c in chroms])
            except ValueError as e:
                raise ValueError("LDPredInf(h2=None) estimates h2 by LD-score regression (the reference's default, "
                                 f"magenpy.stats.h2.ldsc.simple_ldsc) -- {e}  Or pass h2.") from e
        loaded, self.dequantize_on_the_fly, self.dequantize_scale = load_ld_in_order(
            ld_mats, chroms, self.low_memory, dequantize_on_the_fly, float_precision, expand_ld_on_device=False)
        self.std_beta = {c: np.asarray(gdl.sumstats_table[c].get_snp_pseudo_corr()).astype(self._T) for c in chroms}
        # one plan over the concatenated chromosomes (LD blocks never span chromosomes)
        lb, ip, data, self._seg = merge_ld_arrays(
            chroms, self.shapes, {c: ld.left_bound for c, ld in loaded.items()}, {c: ld.indptr for c, ld in loaded.items()},
            {c: ld.data for c, ld in loaded.items()})
        del loaded
        self._plan = None
        if solve_fn is None:
            from .. import _lib
            if _lib.device_count() < 1:
                raise RuntimeError("LDPredInf needs a HIP device: the solve has no CPU fallback")
            self.device = int(device) if device is not None else 0
            self._plan = open_plan(LoadedLD(lb, ip, data, ld_form(self.low_memory)), self.device)
        else:
            self._ld = (lb, ip, data)
        if h2 is None:
            self.h2 = self._estimate_h2(lb, ip, data, corr, score_fn)
        self.lam = None
        self.post_mean_beta = None
        self.solve_info = None

    def _estimate_h2(self, lb, ip, data, corr, score_fn):
        """`simple_ldsc` over the model's own LD: corrected unit-weight scores of its plan (the host path: `score_fn` or
        `ld_scores_host`), then the estimate over all chromosomes."""
        from ..stats.ldsc import ld_scores_host, ldsc_estimate_over
        if self._plan is not None and score_fn is None:
            scores = self._plan.ld_scores(None, corr, dq_scale=self.dequantize_scale, float_precision=self.float_precision)
        else:
            scores = (score_fn or ld_scores_host)(lb, ip, data, self.low_memory, None, corr, self.dequantize_scale)
        self.ld_score = {c: np.asarray(scores[a:e], dtype=np.float64) for c, (a, e) in self._seg.items()}
        h2 = ldsc_estimate_over(self.gdl.sumstats_table, self.ld_score, self.chromosomes)
        if not 0.0 < h2 <= 1.0:
            raise ValueError(f"LDPredInf(h2=None): the LD-score regression estimate h2 = {h2!r} is not in (0, 1]; pass h2")
        return h2

    @property
    def chromosomes(self):
        return sorted(self.shapes)

    @property
    def m(self):
        return int(self.gdl.m)

    n_snps = m

    @property
    def n(self):
        return self._sample_size

    def get_heritability(self):
        return self.h2

    def get_posterior_mean_beta(self):
        return self.post_mean_beta

    def predict(self, test_gdl=None, **kw):
        """Polygenic scores of the training loader's genotyped samples, or of `test_gdl`'s (BayesPRSModel.py:229-250):
        `viprs_amd.genotypes.model_predict`."""
        from ..genotypes import model_predict
        return model_predict(self, test_gdl, **kw)

    def fit(self, solver="minres", rtol=None, maxiter=None, x0=None, **solver_kwargs):
        """Solves ``(R + lam I) beta = beta_hat`` with ``lam = M / (N h2)`` (LDPredInf.py:81-86) for the standardised
        effects.  `x0`: a start vector, ``{chromosome: array}`` or one array over all SNPs."""
        if solver_kwargs:
            raise TypeError(f"fit() got unexpected keyword arguments {sorted(solver_kwargs)}: the device solver takes "
                            "rtol, maxiter and x0")
        if solver == "lsqr":
            raise NotImplementedError("solver='lsqr' is not available: use 'minres' (on this symmetric system lsqr solves "
                                      "the same equations with two LD products per step)")
        if solver != "minres":
            raise ValueError(f"unknown solver {solver!r}: 'minres'")
        chroms = self.chromosomes
        self.lam = self.n_snps / (self.n * self.h2)
        b = np.concatenate([self.std_beta[c] for c in chroms])
        if isinstance(x0, dict):
            x0 = np.concatenate([np.asarray(x0[c]) for c in chroms])
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=self._T)
        if self._solve_fn is not None:
            lb, ip, data = self._ld
            x, info = self._solve_fn(lb, ip, data, self.low_memory, b, self.lam, self.dequantize_scale, rtol, maxiter, x0)
        else:
            x, info = self._plan.solve_ridge(b, self.lam, dq_scale=self.dequantize_scale, rtol=rtol, maxiter=maxiter,
                                             x0=x0)
        self.solve_info = info
        self.post_mean_beta = {c: np.array(x[a:e]) for c, (a, e) in self._seg.items()}
        if not info.converged:
            warnings.warn("Maximum iterations reached without convergence.\n"
                          "You may need to run the model for more iterations.", RuntimeWarning, stacklevel=2)
        return self
