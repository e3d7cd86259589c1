"""``PerChromosomeGroups`` -- what the per-chromosome lock-step fits of every model family share (``VIPRSPerChromosome``,
``VIPRSMixPerChromosome``, ``VIPRSGridPerChromosome``, ``VIPRSGridPathwisePerChromosome``): the chromosomes as SNP groups of
one device state, and the pieces of a fit that do not depend on the family."""
import logging

import numpy as np

from ..utils.optim import OptimizeResult
from .VIPRS import _is_numeric

logger = logging.getLogger(__name__)

# tracked parameter -> its place in (pi, sigma_epsilon, tau_beta, sigma_g, max_eta_diff) of one model; "heritability" is
# formed from them
_TRACKED = {"pi": 0, "sigma_epsilon": 1, "tau_beta": 2, "sigma_g": 3, "max_eta_diff": 4}


class PerChromosomeGroups:
    """Mixed in FRONT of the model class: the chromosomes as SNP groups of the one device state, their sample sizes / SNP
    counts / lambda_min, the convergence mask over LD blocks, the per-chromosome result tables."""

    _always_merge = True

    def __init__(self, gdl, lambda_min=None, **kwargs):
        """Arguments of the model class; ``lambda_min='infer'`` gives every chromosome the value of ITS LD matrix (each of the
        reference's per-chromosome models infers its own, VIPRS.py:186-191); ``lambda_min='compute'`` the value computed on
        the device from ITS LD blocks."""
        compute = isinstance(lambda_min, str) and lambda_min == "compute"
        infer = lambda_min is not None and not _is_numeric(lambda_min) and not compute
        super().__init__(gdl, lambda_min=None if infer else lambda_min, **kwargs)
        self.groups = sorted(self._all_shapes)                     # one model per chromosome of the data loader
        self._gindex = {c: g for g, c in enumerate(self.groups)}
        ss = gdl.sumstats_table
        self._n_group = np.array([float(np.max(ss[c].n_per_snp)) for c in self.groups])      # BayesPRSModel.py:75
        self._m_group = np.array([int(self._all_shapes[c]) for c in self.groups], dtype=np.int64)
        if infer:
            ld = gdl.get_ld_matrices()
            self._lambda_group = [ld[c].get_lambda_min(min_max_ratio=1e-3) for c in self.groups]
        elif compute:
            self._lambda_group = [self.lambda_min_computed[c] for c in self.groups]
            self.lambda_min = 0.0                                  # (as with 'infer': the groups carry the values)
        else:
            self._lambda_group = [self.lambda_min] * len(self.groups)
        self.optim_results = {}
        self._em = None
        if self._e_step_fn is None:
            if not self._merged:
                raise NotImplementedError(type(self).__name__ + " runs on the device-resident one-plan layout "
                                          "(device_resident=True, merge_chromosomes=True)")
            ds, plan = self._dstate["*"], self._plans["*"]
            sizes = [int(self.shapes.get(c, 0)) for c in self.groups]
            self._group_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            ds.set_groups(self._group_start)
            starts, _ = plan.blocks()
            # (`right`: a chromosome without local SNPs shares its start with the next one, which owns the block)
            self._block_group = np.searchsorted(self._group_start, starts[:-1], side="right") - 1
            self._active_mask = None

    def _set_active(self, active_groups):
        """The chromosomes whose models still iterate: the LD blocks of the others leave the sweep."""
        if self._e_step_fn is not None:
            return
        flags = np.zeros(len(self.groups), dtype=bool)
        flags[active_groups] = True
        mask = flags[self._block_group]
        self._plans["*"].set_active_blocks(None if mask.all() else mask)

    def _narrow(self, a, keep):
        """The chromosomes `a[keep]` iterate on: the next round's active set, out of the sweep whoever left."""
        if not keep.all():
            self._set_active(a[keep])
        return a[keep]

    def _theta0_for(self, c, theta_0):
        """The theta_0 of chromosome c's model from one dict for all or ``{chromosome: dict}``: a copy (`_merge_theta` writes
        into its argument), or None."""
        t0 = theta_0
        if isinstance(theta_0, dict) and theta_0 and all(k in self._gindex for k in theta_0):
            t0 = theta_0.get(c)                                    # {chromosome: theta_0}
        return dict(t0) if t0 else None

    def _all_rank_sums(self, s, reduced=False):
        """A table of sums, one row per model, over all ranks: the sum of every column but the last (max |eta_diff|), whose
        maximum it is.  `reduced`: the device has already reduced it across ranks."""
        if self.comm.world_size > 1 and not reduced:
            tot = self.comm.allreduce_sum(np.ascontiguousarray(s[:, :-1]).ravel()).reshape(s.shape[0], -1)
            mx = self.comm.allreduce_max(np.ascontiguousarray(s[:, -1]))
            s = np.column_stack([tot, mx])
        return s

    def _var_tau_of(self, c, lam, sig_e, tau_e):
        """var_tau of chromosome c as its model's LAST E-step built it, from that E-step's (lambda_min, sigma_epsilon,
        tau_beta) (VIPRS.py:520-523)."""
        return (self.n_per_snp[c] * (1.0 + lam) / sig_e) + tau_e

    def _append_tracked(self, h, theta, sigma_g, max_eta_diff):
        """The tracked parameters of one model, with hyper-parameters `theta` = (pi, sigma_epsilon, tau_beta), onto its
        history `h` (`VIPRS.update_theta_history`)."""
        vals = (*theta, sigma_g, max_eta_diff)
        for t in self.tracked_params:
            if callable(t):
                raise NotImplementedError("callable tracked_params are not supported by the per-chromosome fit")
            if t == "heritability":
                h[t].append(sigma_g / (sigma_g + theta[1]))
            elif t in _TRACKED:                            # (any other name keeps its empty list, as in `VIPRS`)
                v = vals[_TRACKED[t]]
                h[t].append(np.sum(v) if t == "pi" and np.ndim(v) else v)       # a mixture's K-vector: the sum of pi

    def _publish_results(self, results, fun):
        """`results` = {chromosome: OptimizeResult} and the aggregated ``optim_result`` (`fun`: the sum of the final ELBOs),
        the posterior moments, a warning per chromosome that did not converge."""
        self.optim_results = results
        res = self.optim_result = OptimizeResult()
        res.nit = max(r.nit for r in results.values())
        res.success = all(r.success for r in results.values())
        res.stop_iteration = True
        res.fun = fun
        failed = [c for c in self.groups if not results[c].success]
        res.message = "All chromosomes converged." if not failed else \
            "Not converged: chromosome(s) " + ", ".join(str(c) for c in failed)
        self.update_posterior_moments()
        self._gather_posterior()
        for c in failed:
            logger.warning("\tchromosome %s: %s", c, results[c].message)
        return self

    def get_heritability(self):
        return {c: self._sigma_g[c] / (self._sigma_g[c] + self.sigma_epsilon[c]) for c in self.groups}

    def to_history_table(self):
        import pandas as pd
        return pd.concat([pd.DataFrame(h).assign(Chromosome=c) for c, h in self.history.items()])
