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

from ._merged_plan import MergedPlanModel


class LDPredInf(MergedPlanModel):

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
        self._set_loader(gdl, comm, not_sharded="solve")
        self.h2 = h2
        self._solve_fn = solve_fn
        self._sample_size = max(float(np.max(s.n_per_snp)) for s in gdl.sumstats_table.values())
        lb, ip, data, corr = self._load(float_precision, low_memory, dequantize_on_the_fly, device, solve_fn is not None,
                                        "LDPredInf needs a HIP device: the solve has no CPU fallback", ld_correction=h2 is None)
        if h2 is None:
            self.h2 = self._ldsc_h2(lb, ip, data, corr, score_fn)
            if not 0.0 < self.h2 <= 1.0:
                raise ValueError(f"LDPredInf(h2=None): the LD-score regression estimate h2 = {self.h2!r} is not in (0, 1]; "
                                 "pass h2")
        self.lam = None
        self.post_mean_beta = None
        self.solve_info = None

    def _ld_correction(self, ld_mats):
        try:
            return super()._ld_correction(ld_mats)
        except ValueError as e:
            raise ValueError("LDPredInf(h2=None) estimates h2 by LD-score regression (the reference's default, "
                             f"magenpy.stats.h2.ldsc.simple_ldsc) -- {e}  Or pass h2.") from e

    @property
    def n(self):
        return self._sample_size

    def get_heritability(self):
        return self.h2

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
        b = self._concat(self.std_beta)
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
        self.post_mean_beta = self._split(x)
        if not info.converged:
            warnings.warn("Maximum iterations reached without convergence.\n"
                          "You may need to run the model for more iterations.", RuntimeWarning, stacklevel=2)
        return self
