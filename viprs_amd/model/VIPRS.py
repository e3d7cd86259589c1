"""``VIPRS`` -- variational EM for the spike-and-slab PRS model with the E-step on MI355X.

Keeps the constructor, ``fit()``, ``e_step()``, ``m_step()``, ``elbo()`` surface and the
dict-of-arrays attributes of the reference class (viprs/model/VIPRS.py) so that code written
against it keeps working, but is organised around the GPU:

* ``__init__`` uploads every chromosome's LD once (``LDPlan`` = the reference's "load LD matrices to
  memory", VIPRS.py:151-172) and keeps the variational state in HBM (``DeviceState``);
* ``e_step()`` does the O(m) host prep of VIPRS.py:400-418, launches the HIP sweep of every
  chromosome (each on its own stream) and mirrors the state back into the NumPy attributes;
* ``m_step()`` / ``elbo()`` are written over one vector of per-rank partial sums, so that with
  several GPUs (chromosomes sharded over ranks) the only communication per EM iteration is ONE small
  float64 all-reduce (viprs_amd.parallel).

There is no CPU fallback: without ``libviprs_hip.so`` and a GPU the E-step raises.  (``e_step_fn``
lets the CPU test-suite drive this host logic with the oracle's kernels; it is never set by the
package itself.)
"""
import logging
import math

from types import SimpleNamespace

import numpy as np

from ..parallel import BlockShard, LocalComm, broadcast_from_root, shard_blocks
from ..utils.optim import ConditionStreak, OptimizeResult
from ._ld_loading import LoadedLD, empty_ld, ld_form, load_ld_in_order, open_plan

logger = logging.getLogger(__name__)

_DOUBLE_RES = np.finfo(np.float64).resolution      # clip for gamma in the ELBO (VIPRS.py:509-518)


def _isclose(a, b, atol, rtol=0.0):
    """`np.isclose(a, b, atol=atol, rtol=rtol)` for two scalars (the stopping rules call it twice per iteration and model;
    NumPy's takes 25 us a call): |a - b| <= atol + rtol |b| for finite operands, equality when one is infinite, False for NaN."""
    if not (math.isfinite(a) and math.isfinite(b)):
        return bool(a == b)
    return bool(abs(a - b) <= atol + rtol * abs(b))


def _is_numeric(x):
    return isinstance(x, (int, float, np.number, np.ndarray))


def _is_compute(lambda_min):
    """lambda_min='compute': the extremal eigenvalues of the LD the model holds, by Lanczos on its device."""
    return isinstance(lambda_min, str) and lambda_min == "compute"


def _pseudo_r2_external(validation_ld, std_beta, beta, device=0):
    """`viprs_amd.eval.pseudo_r2` of `beta` against an external panel: plans are made from ``(left_bound, indptr, data,
    low_memory)`` tuples and closed again, plans that are handed in stay open."""
    from ..eval.pseudo_metrics import pseudo_r2
    plans, own = {}, []
    try:
        for c in beta:
            if c not in validation_ld:
                raise ValueError(f"validation_ld has no LD for chromosome {c}")
            ld = validation_ld[c]
            if isinstance(ld, (tuple, list)):
                lb, ip, data, low_memory = ld
                ld = open_plan(LoadedLD.from_arrays(lb, ip, data, ld_form(low_memory)), device)
                own.append(ld)
            plans[c] = ld
        return pseudo_r2(plans, std_beta, beta)
    finally:
        for ld in own:
            ld.close()


class VIPRS:

    _always_merge = False        # subclasses that need the one-plan layout even for a single local chromosome

    def __init__(self, gdl, fix_params=None, tracked_params=None, lambda_min=None, float_precision="float32",
                 order="F", low_memory=True, dequantize_on_the_fly=False, threads=1,
                 device=None, comm=None, math_mode="exact", e_step_fn=None, device_resident=True,
                 merge_chromosomes=True, expand_ld_on_device=None, h2_init=None, score_fn=None):
        """Same arguments as the reference (VIPRS.py:68-77) plus:

        :param device: HIP device index (default: ``comm.rank`` modulo the visible devices).
        :param comm: ``viprs_amd.parallel`` communicator; chromosomes are sharded over its ranks.
        :param math_mode: 'exact' (bit-for-bit the reference's arithmetic) or 'fast'.
        :param e_step_fn: test hook -- a callable with ``cpp_e_step``'s positional signature that
            replaces the HIP kernels (used by the CPU tests with the oracle).
        :param device_resident: keep the whole EM iteration on the GPU (host prep, zeta, M-step / ELBO
            sums as device kernels; only ~11 scalars per chromosome cross PCIe per iteration).  The
            NumPy state attributes are refreshed when ``fit()`` returns or on ``sync_host()``.
        :param merge_chromosomes: device-resident mode only -- put the LD blocks of all local chromosomes
            into ONE device plan (blocks are independent, chromosomes only matter for the ``update_pi``
            mean, kept through per-SNP weights): one set of launches and one reduction per EM iteration
            instead of one per chromosome.
        :param expand_ld_on_device: ``low_memory=False`` only -- load the compact upper-triangular store
            and mirror it into the symmetric windows on the GPU (``LDPlan.from_upper``) instead of asking
            the LD matrix for ``load(return_symmetric=True)``: the symmetric copy never exists in host
            memory and half the bytes cross PCIe.  ``None`` (default): only when the LD matrix cannot
            hand out the symmetric form itself.  The host attributes ``ld_data / ld_indptr /
            ld_left_bound`` then hold the upper-triangular arrays.

        The stages, in order: `_check_arguments`, `_load_ld` (every chromosome -> `_ld_loading.LoadedLD`),
        `_resolve_lambda_min`, `_deal_blocks` (several ranks), `_keep_local`, then `_build_device` (plans and states
        through `_ld_loading.open_plan`) or, with ``e_step_fn``, the host model of the expansion.
        """
        if gdl.genotype is None and (gdl.ld is None or gdl.sumstats_table is None):
            raise AssertionError("The data loader must contain summary statistics and LD matrices.")
        self.gdl = gdl
        self.float_precision = float_precision
        self._T = np.dtype(float_precision)
        self.float_eps = np.finfo(self._T).eps
        self.comm = comm if comm is not None else LocalComm()
        self.threads = threads
        self.fix_params = fix_params or {}
        self.tracked_params = tracked_params or []
        self.order = order
        self.low_memory = low_memory
        self.math_mode = math_mode
        self._e_step_fn = e_step_fn
        self._check_arguments(lambda_min, h2_init)
        self.h2_init = h2_init
        self._score_fn = score_fn
        self.h2_ldsc = None

        # ---- inputs + LD: load, shard at LD-block granularity, then make device-resident ---------
        # (BayesPRSModel.py:118-142, VIPRS.py:151-191).  With several ranks every LD block -- the
        # independent unit of the E-step -- is assigned to one rank (chain-aware LPT over the blocks of
        # ALL chromosomes, `parallel.shard_blocks`), so a single-chromosome fit shards as well; each rank
        # keeps only the rows / per-SNP entries of its blocks, re-indexed to a local SNP numbering.
        # All host loads finish before the first plan exists.
        self._all_shapes = dict(gdl.shapes)
        self._n_chroms_total = len(self._all_shapes)
        self._sample_size = max(float(np.max(s.n_per_snp)) for s in gdl.sumstats_table.values())
        ld_mats = gdl.get_ld_matrices()
        loaded = self._load_ld(ld_mats, dequantize_on_the_fly, expand_ld_on_device)
        self._resolve_lambda_min(lambda_min, ld_mats)
        self._deal_blocks(loaded)
        self._keep_local(loaded)
        self._plans, self._dstate = {}, {}
        self._resident = self._merged = self._device_reduce = False
        if e_step_fn is None:
            self._build_device(device, device_resident, merge_chromosomes, ld_mats)
            if _is_compute(lambda_min):
                self._compute_lambda_min()
        elif self._expanded:                     # test hook: the host model of the device-side expansion
            from ..data import mirror_upper_ld
            for c in self.chromosomes:
                self.ld_left_bound[c], self.ld_indptr[c], self.ld_data[c] = mirror_upper_ld(
                    self.ld_indptr[c], self.ld_data[c])
            self._expanded = False
        self._host_stale = False
        self._last_prep = None

        # ---- model state -------------------------------------------------------------------------
        self.var_gamma, self.var_mu, self.var_tau, self._log_var_tau = {}, {}, {}, {}
        self.eta, self.zeta, self.eta_diff, self.q = {}, {}, {}, {}
        self.sigma_epsilon = self.tau_beta = self.pi = self._sigma_g = None
        self.pip = self.post_mean_beta = self.post_var_beta = None
        self.optim_result = OptimizeResult()
        self.history = {}
        self._sums = None
        self._sums_valid = False
        self._max_eta_diff = 0.0

    # ---- the stages of the constructor, in the order it runs them -------------------------------------
    def _check_arguments(self, lambda_min, h2_init):
        if self.math_mode == "fast" and (self._T == np.float64 or getattr(self, "K", 1) > 8):
            # (LDPlan.effective_math_mode() reports what a sweep really ran in)
            import warnings
            warnings.warn("math_mode='fast' has no kernels for " + ("float_precision='float64'" if self._T == np.float64 else
                          f"mixtures of {self.K} components (> 8)") + ": this model runs in EXACT arithmetic", stacklevel=3)
        if _is_compute(lambda_min) and self._e_step_fn is not None:
            raise RuntimeError("lambda_min='compute' needs a HIP device: the Lanczos recurrence has no CPU fallback")
        if _is_compute(lambda_min) and self.comm.world_size > 1:
            raise NotImplementedError("lambda_min='compute' runs on one rank only (world_size > 1: annotate the LD "
                                      "matrices with viprs_amd.stats.spectrum.annotate_spectrum and use 'infer')")
        if not (h2_init is None or _is_numeric(h2_init) or (isinstance(h2_init, str) and h2_init == "ldsc")):
            raise ValueError(f"h2_init: None, 'ldsc' or a number, got {h2_init!r}")
        if isinstance(h2_init, str) and self.comm.world_size > 1:
            raise NotImplementedError("h2_init='ldsc' runs on one rank only (world_size > 1: compute the estimate with "
                                      "viprs_amd.stats.ldsc.simple_ldsc and pass it as a number)")

    def _load_ld(self, ld_mats, dequantize_on_the_fly, expand_ld_on_device):
        """``{chromosome: LoadedLD}`` of ALL chromosomes (`load_ld_in_order`: `dequantize_on_the_fly` threaded through the
        sorted chromosomes, `dequantize_scale` from the first one's matrix; with several ranks a store that can hand out
        row ranges is read only as far as its index).  `_expanded`: some chromosome's upper store is to be mirrored."""
        loaded, self.dequantize_on_the_fly, self.dequantize_scale = load_ld_in_order(
            ld_mats, sorted(self._all_shapes), self.low_memory, dequantize_on_the_fly, self.float_precision,
            expand_ld_on_device=expand_ld_on_device, index_only=self.comm.world_size > 1)
        self._expanded = any(ld.form == "upper_to_expand" for ld in loaded.values())
        return loaded

    def _resolve_lambda_min(self, lambda_min, ld_mats):
        """None: 0; a number: itself; 'compute': 0 until the LD is on the device (`_compute_lambda_min`); 'infer': what the
        LD matrices answer -- the reference keeps the LAST chromosome's value (:186-191)."""
        self.lambda_min = 0.0
        if _is_numeric(lambda_min):
            self.lambda_min = lambda_min
        elif lambda_min is not None and not _is_compute(lambda_min):
            for c in sorted(self._all_shapes):
                try:
                    self.lambda_min = ld_mats[c].get_lambda_min(min_max_ratio=1e-3)
                except NotImplementedError as e:     # (a store whose ridge formula this build cannot verify: say where, and the remedy)
                    raise type(e)(f"lambda_min='infer', chromosome {c}: {e}  Remedy: VIPRS(..., lambda_min=<number>), or "
                                  "set `lambda_min_formula` on the LD matrix object.") from e

    def _deal_blocks(self, loaded):
        """Several ranks: `_shard` (this rank's blocks of every chromosome) and `_block_owner` (chromosome -> (block
        starts, owning rank of every block)), identical on every rank.  The block starts come from the index alone
        (`plan_blocks`, in the upper form when `low_memory` or expanded), the element size of the cost model from the first
        chromosome's load dtype."""
        self._shard, self._block_owner = {}, {}
        if self.comm.world_size == 1:
            return
        from ..plan import plan_blocks
        chroms = sorted(loaded)
        upper_form = bool(self.low_memory) or self._expanded
        starts = {c: plan_blocks(loaded[c].left_bound, loaded[c].indptr, upper_form)[0] for c in chroms}
        sizes = np.concatenate([np.diff(starts[c]) for c in chroms])
        owner = shard_blocks(sizes, self.comm.world_size, np.dtype(loaded[chroms[0]].dtype).itemsize)
        k = 0
        for c in chroms:
            nb = len(starts[c]) - 1
            mine = [b for b in range(nb) if owner[k + b] == self.comm.rank]
            self._block_owner[c] = (starts[c], np.asarray(owner[k:k + nb]))
            k += nb
            self._shard[c] = BlockShard(starts[c], mine)

    def _keep_local(self, loaded):
        """The host attributes of the chromosomes this rank holds: everything with one rank, else the rows of its blocks
        -- sliced from the loaded arrays, or read from a store of which only the index was loaded.  Empties `loaded`."""
        ss = self.gdl.sumstats_table
        self.shapes, self.n_per_snp, self.std_beta = {}, {}, {}
        self.ld_data, self.ld_indptr, self.ld_left_bound = {}, {}, {}
        for c in sorted(loaded):
            ld = loaded.pop(c)
            sh = self._shard.get(c)
            if sh is None:
                self.shapes[c] = int(self._all_shapes[c])
                self.ld_left_bound[c], self.ld_indptr[c], self.ld_data[c] = ld.left_bound, ld.indptr, ld.data
                self.n_per_snp[c] = ss[c].n_per_snp
                self.std_beta[c] = ss[c].get_snp_pseudo_corr().astype(self._T)
            elif sh.m > 0:
                self.shapes[c] = sh.m
                self.ld_left_bound[c], self.ld_indptr[c], self.ld_data[c] = (
                    sh.read_ld(ld.ld_mat, ld.dtype) if ld.data is None else sh.slice_ld(ld.left_bound, ld.indptr, ld.data))
                self.n_per_snp[c] = sh.take(ss[c].n_per_snp)
                self.std_beta[c] = sh.take(ss[c].get_snp_pseudo_corr()).astype(self._T)

    def _build_device(self, device, device_resident, merge_chromosomes, ld_mats):
        """Plans and states, in sorted chromosome order.  Per chromosome: `set_n_per_snp` runs after all plans exist.
        Merged: ``upload("std_beta")``, `set_n_per_snp`, `set_snp_weights`, `set_comm`.  (The state placement probe times
        allocations: their order is part of what the benchmark measures.)"""
        from .. import _lib
        ndev = _lib.device_count()
        if ndev < 1:
            raise RuntimeError("VIPRS needs a HIP device: the E-step has no CPU fallback")
        self.device = int(device) if device is not None else self.comm.rank % ndev
        self._resident = bool(device_resident) and self._supports_resident()
        form = ld_form(self.low_memory, self._expanded)
        chroms = self.chromosomes
        # several ranks: ONE plan per rank whatever the number of local chromosomes (one collective per EM
        # iteration, per-SNP weights 1 / m_c of the FULL chromosome for the update_pi mean)
        self._merged = (self._resident and bool(merge_chromosomes) and self._supports_merged()
                        and (len(chroms) > 1 or self.comm.world_size > 1 or self._always_merge))
        if self._merged:
            # one plan over the concatenated chromosomes: windows and row offsets shifted into place
            from ..data import merge_ld_arrays
            if chroms:
                merged = merge_ld_arrays(chroms, self.shapes, self.ld_left_bound, self.ld_indptr, self.ld_data)
                ld, self._seg = LoadedLD(*merged[:3], form), merged[3]
                del merged
            else:                                # (its `data`: the stored dtype when dequantising, else the model's)
                first = ld_mats[min(self._all_shapes)]
                ld, self._seg = empty_ld(first.stored_dtype if self.dequantize_on_the_fly else self._T, form), {}
            self._plans["*"] = open_plan(ld, self.device, self.math_mode)
            del ld
            ds = self._dstate["*"] = self._make_device_state(self._plans["*"])
            cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
            ds.upload("std_beta", cat([self.std_beta[c] for c in chroms], self._T))
            ds.set_n_per_snp(cat([np.asarray(self.n_per_snp[c], dtype=np.float64).ravel() for c in chroms], np.float64))
            ds.set_snp_weights(cat([np.full(self.shapes[c], 1.0 / self._all_shapes[c]) for c in chroms], np.float64))
            if getattr(self.comm, "device_side", False):
                ds.set_comm(self.comm)           # sums_begin / sums_end return the all-rank sums (RCCL, C ABI)
                self._device_reduce = True
            return
        for c in chroms:
            self._plans[c] = open_plan(LoadedLD(self.ld_left_bound[c], self.ld_indptr[c], self.ld_data[c], form),
                                       self.device, self.math_mode)
            self._dstate[c] = self._make_device_state(self._plans[c])
            self._dstate[c].upload("std_beta", self.std_beta[c])
        if self._resident:
            for c in chroms:
                self._dstate[c].set_n_per_snp(self.n_per_snp[c])

    def _compute_lambda_min(self):
        """lambda_min='compute': |min(smallest eigenvalue, 0)| of every chromosome's LD, from the extremal eigenvalues of
        its LD blocks (`LDPlan.extremal_eigenvalues` on the plans of this model: the matrix the E-step multiplies with, in
        the model's precision).  No min / max ratio, hence none of the unpinned formulas.  `lambda_min` itself is the LAST
        chromosome's value, as with 'infer' (the reference, VIPRS.py:186-191); `lambda_min_computed` keeps every
        chromosome's, `spectrum` what they were derived from."""
        from ..stats.spectrum import lambda_min_from_extremes, plan_spectrum
        kw = dict(dq_scale=self.dequantize_scale, float_precision=self.float_precision)
        if self._merged:
            self.spectrum = plan_spectrum(self._plans["*"], self._seg, **kw)
        else:
            self.spectrum = {c: plan_spectrum(self._plans[c], **kw)[None] for c in self.chromosomes}
        self.lambda_min_computed = {c: lambda_min_from_extremes(s["min"], s["max"]) for c, s in self.spectrum.items()}
        self.lambda_min = self.lambda_min_computed[sorted(self.lambda_min_computed)[-1]]

    _h2_clip = (0.01, 0.99)              # the reference's clip of the LD-score estimate (VIPRS.py:286)

    def _ldsc_h2(self):
        """h2_init='ldsc': the LD scores of the LD this model holds -- `LDPlan.ld_scores` on its plans, unit weights, in the
        model's precision; on the host (`score_fn` or `ld_scores_host`) with ``e_step_fn`` or ``score_fn`` -- and the
        estimates `viprs_amd.stats.ldsc.ldsc_estimate` derives from them: ``h2_ldsc["*"]`` over all chromosomes, as the
        reference's ``simple_ldsc(gdl)``, and ``h2_ldsc[c]`` of every chromosome on its own.  The sample-size correction
        applies when every LD object knows its ``sample_size``.  Computed once; ``ld_score`` keeps the scores."""
        if self.h2_ldsc is not None:
            return self.h2_ldsc
        from ..stats.ldsc import ld_correction, ld_scores_host, ldsc_estimate_over
        ld_mats, ss = self.gdl.get_ld_matrices(), self.gdl.sumstats_table
        chroms = sorted(self.shapes)
        corrected = all(getattr(ld_mats[c], "sample_size", None) is not None for c in chroms)
        corr = {c: ld_correction(ld_mats[c], self.shapes[c], where=f"chromosome {c}") if corrected else None for c in chroms}
        if self._e_step_fn is None and self._score_fn is None:
            kw = dict(dq_scale=self.dequantize_scale, float_precision=self.float_precision)
            if self._merged:
                flat = self._plans["*"].ld_scores(None, np.concatenate([corr[c] for c in chroms]) if corrected else None, **kw)
                scores = {c: flat[a:e] for c, (a, e) in self._seg.items()}
            else:
                scores = {c: self._plans[c].ld_scores(None, corr[c], **kw) for c in chroms}
        else:
            fn = self._score_fn or ld_scores_host
            upper = bool(self.low_memory) or self._expanded
            scores = {c: fn(self.ld_left_bound[c], self.ld_indptr[c], self.ld_data[c], upper, None, corr[c],
                            self.dequantize_scale) for c in chroms}
        self.ld_score = {c: np.asarray(scores[c], dtype=np.float64) for c in chroms}
        est = {c: ldsc_estimate_over(ss, self.ld_score, [c]) for c in chroms}
        est["*"] = ldsc_estimate_over(ss, self.ld_score, chroms)
        self.h2_ldsc = est
        return est

    def _h2_start(self, chrom=None):
        """The clipped heritability `initialize_theta` starts from (None: the random draw): of the model over all
        chromosomes, or of chromosome `chrom`'s own model."""
        if self.h2_init is None:
            return None
        h2 = self._ldsc_h2()["*" if chrom is None else chrom] if isinstance(self.h2_init, str) else float(self.h2_init)
        if not np.isfinite(h2):
            raise ValueError(f"h2_init={self.h2_init!r}: the heritability estimate is {h2!r}")
        return float(np.clip(h2, *self._h2_clip))

    # ---- sizes ------------------------------------------------------------------------------------
    @property
    def chromosomes(self):
        return sorted(self.shapes.keys())

    @property
    def m(self):
        return int(self.gdl.m)

    n_snps = m

    @property
    def n(self):
        return self._sample_size

    def _shape(self, c):
        return self.shapes[c]

    def _make_device_state(self, plan):
        from ..plan import DeviceState
        return DeviceState(plan, self.float_precision, "spike_slab")

    def _supports_resident(self):
        return True

    def _supports_merged(self):
        return True

    # ---- initialisation (VIPRS.py:213-359) -------------------------------------------------------
    def initialize(self, theta_0=None, param_0=None):
        self.initialize_theta(theta_0)
        self.initialize_variational_parameters(param_0)
        self.init_optim_meta()

    def init_optim_meta(self):
        self.history = {"ELBO": []}
        for t in self.tracked_params:
            self.history[t if isinstance(t, str) else t.__name__] = []
        self.optim_result.reset()

    def _merge_theta(self, theta_0):
        if theta_0 is not None and self.fix_params is not None:
            theta_0.update(self.fix_params)
        elif self.fix_params is not None:
            theta_0 = self.fix_params
        elif theta_0 is None:
            theta_0 = {}
        return theta_0

    def _sync_theta(self):
        """Several ranks: everyone takes rank 0's hyper-parameters (the random draws of initialize_theta
        would otherwise differ per rank).  One small collective, called symmetrically on every rank."""
        if self.comm.world_size == 1:
            return
        pi, tau = np.atleast_1d(np.asarray(self.pi, dtype=np.float64)), np.atleast_1d(np.asarray(self.tau_beta, dtype=np.float64))
        v = broadcast_from_root(self.comm, np.concatenate([pi, tau, [float(self.sigma_epsilon)]]))
        pi_b, tau_b = v[:pi.size], v[pi.size:pi.size + tau.size]
        self.pi = pi_b.reshape(np.shape(self.pi)) if np.ndim(self.pi) else float(pi_b[0])
        self.tau_beta = tau_b.reshape(np.shape(self.tau_beta)) if np.ndim(self.tau_beta) else float(tau_b[0])
        self.sigma_epsilon = float(v[-1])

    def _cast_theta(self):
        self._sync_theta()
        t = self._T.type
        self.sigma_epsilon, self.pi, self.lambda_min = t(self.sigma_epsilon), t(self.pi), t(self.lambda_min)
        self._sigma_g = t(0.0)

    @staticmethod
    def _theta_values(th, n_snps, h2_start=None):
        """(pi, sigma_epsilon, tau_beta) of VIPRS.py:260-310 for a model over `n_snps` variants, before the casts.
        `h2_start`: a callable giving the heritability to start from where neither sigma_epsilon nor tau_beta is given
        (None, or a callable returning None: the reference's fallback draw)."""
        if "pi" in th:
            pi = th["pi"]
        else:                                                      # VIPRS.py:260-265
            pi = np.random.uniform(low=max(10.0 / n_snps, 1e-5), high=min(0.2, 1e4 / n_snps))
        if "sigma_epsilon" in th:                                  # :301-310
            sigma_epsilon = th["sigma_epsilon"]
            tau_beta = th["tau_beta"] if "tau_beta" in th else (pi * n_snps) / np.maximum(0.01, 1.0 - sigma_epsilon)
        elif "tau_beta" in th:                                     # :295-300
            tau_beta = th["tau_beta"]
            sigma_epsilon = np.clip(1.0 - pi * n_snps / tau_beta, 1e-4, 1.0 - 1e-4)
        else:                                                      # :279-292
            h2 = h2_start() if h2_start is not None else None
            if h2 is None:
                h2 = np.random.uniform(low=0.01, high=0.1)
            sigma_epsilon = 1.0 - h2
            tau_beta = pi * n_snps / max(h2, 0.01)
        return pi, sigma_epsilon, tau_beta

    def initialize_theta(self, theta_0=None):
        th = self._merge_theta(theta_0)
        self.pi, self.sigma_epsilon, self.tau_beta = self._theta_values(th, self.n_snps, self._h2_start)
        self._cast_theta()

    def get_pi(self, chrom=None):
        return self.pi[chrom] if (chrom is not None and isinstance(self.pi, dict)) else self.pi

    def get_tau_beta(self, chrom=None):
        return self.tau_beta[chrom] if (chrom is not None and isinstance(self.tau_beta, dict)) else self.tau_beta

    def get_null_pi(self, chrom=None):
        return 1.0 - self.get_pi(chrom)

    def get_sigma_epsilon(self):
        return self.sigma_epsilon

    def initialize_variational_parameters(self, param_0=None):
        p0 = param_0 or {}
        T = self._T
        self.var_mu, self.var_tau, self.var_gamma = {}, {}, {}
        for c in self.chromosomes:
            shp = self._shape(c)
            self.var_tau[c] = p0["tau"][c] if "tau" in p0 else (self.n_per_snp[c] / self.sigma_epsilon) + self.tau_beta
            self.var_mu[c] = p0["mu"][c].astype(T, order=self.order) if "mu" in p0 else np.zeros(shp, T, order=self.order)
            if "gamma" in p0:
                self.var_gamma[c] = p0["gamma"][c].astype(T, order=self.order)
            else:
                self.var_gamma[c] = (self.get_pi(c) * np.ones(shp, dtype=T, order=self.order)).astype(T, order=self.order)
        self.eta = self.compute_eta()
        self.zeta = self.compute_zeta()
        self.eta_diff = {c: np.zeros_like(e, dtype=T) for c, e in self.eta.items()}
        self.q = {c: np.zeros_like(e, dtype=T) for c, e in self.eta.items()}
        self._log_var_tau = {c: np.log(self.var_tau[c]) for c in self.var_tau}
        self._sums_valid = False
        self._host_stale = False
        self._push_state()

    def set_fixed_params(self, fix_params):
        assert isinstance(fix_params, dict)
        self.fix_params.update(fix_params)
        t = self._T.type
        for k, v in fix_params.items():
            if k in ("sigma_epsilon", "tau_beta", "pi", "lambda_min"):
                setattr(self, k, t(v))

    # ---- device mirror ------------------------------------------------------------------------------
    _STATE = ("var_gamma", "var_mu", "eta", "q", "eta_diff")

    def _push_state(self):
        if self._merged:
            ds = self._dstate["*"]
            for name in self._STATE:
                ds.upload(name, np.concatenate([np.ascontiguousarray(getattr(self, name)[c]) for c in self.chromosomes]))
            return
        for c, ds in self._dstate.items():
            for name in self._STATE:
                ds.upload(name, np.ascontiguousarray(getattr(self, name)[c]))

    def _pull_state(self):
        if self._merged:
            ds = self._dstate["*"]
            for name in self._STATE:
                full = ds.download(name)
                for c, (a, b) in self._seg.items():
                    getattr(self, name)[c][...] = full[a:b]
            return
        for c, ds in self._dstate.items():
            for name in self._STATE:
                ds.download(name, out=getattr(self, name)[c])

    def sync_host(self):
        """Refresh the NumPy state attributes from the GPU (device-resident mode)."""
        if self._resident and self._host_stale:
            self._pull_state()
            if self._last_prep is not None:
                sigma_epsilon, tau_beta, lam = self._last_prep
                for c in self.chromosomes:
                    self.var_tau[c] = (self.n_per_snp[c] * (1.0 + lam) / sigma_epsilon) + tau_beta
                    np.log(self.var_tau[c], out=self._log_var_tau[c])
            self.zeta = self.compute_zeta()
            self._host_stale = False

    # ---- E-step -------------------------------------------------------------------------------------
    def _prep(self, c):
        """Host prep of VIPRS.py:396-418 (float64, cast to the state precision at the end)."""
        tau_beta, pi = self.get_tau_beta(c), self.get_pi(c)
        self.var_tau[c] = (self.n_per_snp[c] * (1.0 + self.lambda_min) / self.sigma_epsilon) + tau_beta
        np.log(self.var_tau[c], out=self._log_var_tau[c])
        T = self._T
        mu_mult = (self.n_per_snp[c] / (self.var_tau[c] * self.sigma_epsilon)).astype(T)
        u_logs = (np.log(pi) - np.log(1.0 - pi) + 0.5 * (np.log(tau_beta) - self._log_var_tau[c])).astype(T)
        shvt = np.sqrt(0.5 * self.var_tau[c]).astype(T)
        return u_logs, shvt, mu_mult

    def e_step(self):
        """One coordinate-ascent sweep over every LD block of every local chromosome."""
        if self._e_step_fn is not None:
            for c in self.chromosomes:
                u_logs, shvt, mu_mult = self._prep(c)
                self._e_step_fn(self.ld_left_bound[c], self.ld_indptr[c], self.ld_data[c], self.std_beta[c],
                                self.var_gamma[c], self.var_mu[c], self.eta[c], self.q[c], self.eta_diff[c],
                                u_logs, shvt, mu_mult, self.dequantize_scale, self.threads, self.low_memory)
        elif self._resident:
            # whole iteration on the device: prep kernel + sweep per chromosome, nothing crosses PCIe
            pi, tau_beta = self.pi, self.tau_beta
            logit_pi = float(np.log(pi) - np.log(1.0 - pi))          # scalar dtype semantics of VIPRS.py:405
            for ds in self._dstate.values():         # one plan per chromosome, or one for all of them
                ds.prep(logit_pi, float(np.log(tau_beta)), self.sigma_epsilon, tau_beta, 1.0 + self.lambda_min)
                ds.e_step(self.dequantize_scale, sync=False)
            self._last_prep = (self.sigma_epsilon, tau_beta, self.lambda_min)
            self._host_stale = True
            self._sums_valid = False
            return
        else:
            for c in self.chromosomes:               # launch everything (one stream per chromosome) ...
                u_logs, shvt, mu_mult = self._prep(c)
                ds = self._dstate[c]
                ds.upload("u_logs", u_logs)
                ds.upload("sqrt_half_var_tau", shvt)
                ds.upload("mu_mult", mu_mult)
                ds.e_step(self.dequantize_scale, sync=False)
            self._pull_state()                       # ... then mirror the state back (syncs each stream)
        self.zeta = self.compute_zeta()
        self._sums_valid = False

    # ---- posterior summaries (VIPRS.py:875-907) ---------------------------------------------------
    def compute_pip(self):
        return self.var_gamma.copy()

    def compute_eta(self):
        return {c: g * self.var_mu[c] for c, g in self.var_gamma.items()}

    def compute_zeta(self):
        return {c: np.multiply(g, self.var_mu[c].astype(np.float64) ** 2 + 1.0 / self.var_tau[c].astype(np.float64))
                for c, g in self.var_gamma.items()}

    def update_posterior_moments(self):
        self.pip = self.compute_pip()
        self.post_mean_beta = {c: e.copy() for c, e in self.eta.items()}
        self.post_var_beta = {c: z - self.eta[c] ** 2 for c, z in self.zeta.items()}

    def _gather_posterior(self):
        """Several ranks: every rank ends up with the posterior of ALL SNPs (pip / post_mean_beta /
        post_var_beta and q keyed by every chromosome, full length) -- one exchange at the end of fit(),
        the only time per-SNP vectors travel.  The variational state itself stays sharded."""
        if self.comm.world_size == 1:
            return
        chroms = sorted(self._all_shapes)

        world = self.comm.world_size
        # SNP index set of every rank's shard, per chromosome (the block assignment is the same on every rank)
        index = {c: [BlockShard(self._block_owner[c][0], np.nonzero(self._block_owner[c][1] == r)[0]).index
                     for r in range(world)] for c in chroms}

        def gather(local):
            tail = next((np.shape(a)[1:] for a in local.values()), None)
            tail_v = self.comm.allreduce_max(np.array([float(tail[0]) if tail else 0.0]))    # grid models: (m, G)
            tail = (int(tail_v[0]),) if tail_v[0] > 0 else ()
            width = int(np.prod(tail)) if tail else 1
            # ONE all-gather of every rank's own SNPs (padded to the largest shard): m x width values travel in total,
            # not world x m x width as with a sum of zero-padded full-length vectors
            n_max = max(sum(len(index[c][r]) for c in chroms) for r in range(world)) * width
            send = np.zeros(n_max, dtype=np.float64)
            off = 0
            for c in chroms:
                sh = self._shard[c]
                if sh.m > 0:
                    send[off:off + sh.m * width] = np.asarray(local[c], dtype=np.float64).reshape(-1)
                off += sh.m * width
            recv = self.comm.allgather(send)
            out = {}
            offs = [0] * world
            for c in chroms:
                full = np.zeros((self._all_shapes[c], width), dtype=self._T)
                for r in range(world):
                    n = len(index[c][r]) * width
                    full[index[c][r]] = recv[r, offs[r]:offs[r] + n].reshape(-1, width)
                    offs[r] += n
                out[c] = full.reshape((self._all_shapes[c],) + tail)
            return out

        self.pip, self.post_mean_beta, self.post_var_beta = gather(self.pip), gather(self.post_mean_beta), \
            gather(self.post_var_beta)
        self.q_full = gather(self.q)

    # ---- posterior tables and pseudo-validation (BayesPRSModel.py:333-410) --------------------------
    def to_table(self, col_subset=("CHR", "SNP", "POS", "A1", "A2"), per_chromosome=False):
        """Posterior estimates as a pandas table: the data loader's SNP columns (``gdl.to_snp_table``
        when it has one -- a magenpy loader does --, otherwise CHR + the SNP's index) followed by
        BETA / PIP / VAR_BETA (``BETA_0, BETA_1, ...`` for grid models, as the reference names them)."""
        import pandas as pd
        if self.post_mean_beta is None:
            raise Exception("The posterior means for BETA are not set. Call `.fit()` first.")
        if hasattr(self.gdl, "to_snp_table"):
            tables = self.gdl.to_snp_table(col_subset=col_subset, per_chromosome=True)
        else:
            tables = {c: pd.DataFrame({"CHR": c, "IDX": np.arange(len(self.post_mean_beta[c]))})
                      for c in sorted(self.post_mean_beta)}

        def cols(name, a):
            a = np.asarray(a)
            if a.ndim == 1:
                return {name: a}
            return {f"{name}_{i}": a[:, i] for i in range(a.shape[1])}

        chroms = sorted(self.post_mean_beta)
        for c in chroms:
            add = dict(cols("BETA", self.post_mean_beta[c]))
            if self.pip is not None:
                add.update(cols("PIP", self.pip[c]))
            if self.post_var_beta is not None:
                add.update(cols("VAR_BETA", self.post_var_beta[c]))
            tables[c] = pd.concat([tables[c], pd.DataFrame(add, index=tables[c].index)], axis=1)
        return tables if per_chromosome else pd.concat([tables[c] for c in chroms])

    def predict(self, test_gdl=None, **kw):
        """Polygenic scores from the posterior mean effects (BayesPRSModel.py:229-250): of the training loader's genotyped
        samples, or of `test_gdl`'s -- ``(n,)``, one column per grid model ``(n, n_models)`` for a fitted grid.  ValueError
        before `fit()` and for a loader without genotypes.  The scoring runs on the device (`DeviceGenotypes.score`; on the
        host without one); SNP alignment, `per_chromosome` and `dose`: `viprs_amd.genotypes.model_predict`."""
        from ..genotypes import model_predict
        return model_predict(self, test_gdl, **kw)

    def pseudo_validate(self, validation_std_beta=None, validation_ld=None):
        """Pseudo-R^2 of the fitted effects against standardized marginal betas of an independent
        cohort: (r'b)^2 / (b'Rb), one value per model for grid fits.

        ``validation_ld=None``: the cohort shares this LD reference, R b = q + b of the fit
        (BayesPRSModel.py:397-410, pseudo_metrics.py `_streamlined_pseudo_r2`).

        ``validation_ld``: the LD of an external validation panel, ``{chromosome: LDPlan}`` or
        ``{chromosome: (left_bound, indptr, data, low_memory)}`` (plans are made from the tuples and closed again):
        R_val b is the device LD product of every model's effects in one pass (`viprs_amd.eval.pseudo_r2`,
        pseudo_metrics.py:52-70, 98-127).  The panel's SNPs are taken as matched to the model's.  Several ranks:
        NotImplementedError (the product is not sharded)."""
        vb = validation_std_beta if validation_std_beta is not None else getattr(self, "validation_std_beta", None)
        assert self.post_mean_beta is not None, "The posterior means for BETA are not set. Call `.fit()` first."
        assert vb is not None, "standardized betas of a validation set are required"
        chroms = sorted(self.post_mean_beta)
        if validation_ld is not None:
            if self.comm.world_size > 1:
                raise NotImplementedError("pseudo_validate(validation_ld=...) runs on one rank only")
            return _pseudo_r2_external(validation_ld, vb, {c: self.post_mean_beta[c] for c in chroms},
                                       device=getattr(self, "device", 0))
        q = self.q_full if self.comm.world_size > 1 else self.q       # several ranks: gathered at the end of fit()
        cat = lambda d: np.concatenate([np.asarray(d[c]) for c in chroms], axis=0)
        r, b = cat(vb), cat(self.post_mean_beta)
        rb_w = cat({c: q[c] + self.post_mean_beta[c] for c in chroms})
        rb = np.sum((b.T * r).T, axis=0)
        bsb = np.sum(b * rb_w, axis=0)
        return rb ** 2 / bsb

    # ---- partial sums: everything the M-step, the ELBO and the stopping rules need ------------------
    def _partial_sums(self):
        """Per-rank sums over the local SNPs; summed over ranks by one all-reduce.

        layout: [0] sum_c mean(gamma_c)   [1] sum zeta            [2] sum((1+lambda) zeta + q eta)
                [3] sum_c std_beta_c.eta_c [4] sum eta^2           [5..8] ELBO sums
                (max|eta_diff| travels in a separate max-reduction)"""
        lam = self.lambda_min
        if self._resident and self._host_stale:
            s = np.zeros(10, dtype=np.float64)
            self._dev_max_eta_diff = 0.0
            for ds in self._dstate.values():         # every plan's reduction in flight ...
                ds.sums_begin(1.0 + lam)
            for c, ds in self._dstate.items():       # ... then collected in order
                v = ds.sums_end()
                s[0] += v[0] if self._merged else v[0] / self._all_shapes[c]     # merged: weights 1 / m_c on the device
                s[1:5] += v[1:5]
                s[5:9] += v[5:9]
                s[9] += v[9]
                self._dev_max_eta_diff = max(self._dev_max_eta_diff, float(v[10]))
            return s
        return self._host_partial_sums(self.chromosomes)

    def _host_partial_sums(self, chroms):
        """The sums over the NumPy state of the given local chromosomes (layout above, 10 entries)."""
        lam = self.lambda_min
        s = np.zeros(9, dtype=np.float64)
        for c in chroms:
            g, z = self.var_gamma[c], self.zeta[c]
            s[0] += np.sum(g, axis=0) / self._all_shapes[c]              # update_pi: mean of per-chromosome means (:446-453)
            s[1] += z.sum()
            s[2] += np.sum((1.0 + lam) * z + np.multiply(self.q[c], self.eta[c]), axis=0)
            s[3] += self.std_beta[c].dot(self.eta[c])
            s[4] += (self.eta[c].astype(np.float64) ** 2).sum()
            gc = np.clip(g.astype(np.float64), _DOUBLE_RES, 1.0 - _DOUBLE_RES)
            ng = np.clip(1.0 - g.astype(np.float64), _DOUBLE_RES, 1.0 - _DOUBLE_RES)
            s[5] += (gc * np.log(gc)).sum()
            s[6] += (ng * np.log(ng)).sum()
            s[7] += gc.sum()
            s[8] += ng.sum()
        extra = np.zeros(1)
        for c in chroms:
            extra[0] += (np.clip(self.var_gamma[c].astype(np.float64), _DOUBLE_RES, 1 - _DOUBLE_RES)
                         * self._log_var_tau[c]).sum()
        return np.concatenate([s, extra])

    def _reduce(self, force=False):
        if self._sums is not None and self._sums_valid and not force:
            return self._sums
        self._sums_valid = True
        on_device = self._resident and self._host_stale
        part = self._partial_sums()
        if on_device and self._device_reduce:
            # the device sums were all-gathered and reduced in rank order on the plan's stream (RCCL through
            # the C ABI, `DeviceState.set_comm`): ONE collective per EM iteration, max |eta_diff| included
            self._sums = part
            self._max_eta_diff = float(self._dev_max_eta_diff)
            return self._sums
        local_max = self._dev_max_eta_diff if on_device else \
            max([float(np.max(np.abs(d))) if d.size else 0.0 for d in self.eta_diff.values()] or [0.0])
        if self.comm.world_size == 1:
            self._sums, self._max_eta_diff = np.asarray(part, dtype=np.float64), float(local_max)
            return self._sums
        # host transport (CPU tests over gloo): the max travels as one more slot of the same exchange
        both = self.comm.allreduce_sum(np.concatenate([part, [0.0]]))
        self._sums = both[:-1]
        self._max_eta_diff = float(self.comm.allreduce_max(np.array([local_max]))[0])
        return self._sums

    # ---- M-step (VIPRS.py:426-484) -----------------------------------------------------------------
    def m_step(self):
        s = self._reduce()
        T = self._T.type
        if "pi" not in self.fix_params:
            self.pi = T(s[0] / self._n_chroms_total)                                  # :434
        if "tau_beta" not in self.fix_params:
            self.tau_beta = self.pi * self.n_snps / s[1]                              # :444
        self._sigma_g = s[2]                                                           # :454-457
        if "sigma_epsilon" not in self.fix_params:
            self.sigma_epsilon = 1.0 + T(-2.0 * s[3]) + self._sigma_g                  # :466-471

    def update_pi(self):
        self._reduce()
        if "pi" not in self.fix_params:
            self.pi = self._T.type(self._sums[0] / self._n_chroms_total)

    # ---- objective (VIPRS.py:497-581) ----------------------------------------------------------------
    def elbo(self, sum_axis=None):
        s = self._current_sums()
        pi, null_pi, tau_beta = self.pi, self.get_null_pi(), self.tau_beta
        e = -np.log(2.0 * np.pi * self.sigma_epsilon)
        if "sigma_epsilon" not in self.fix_params:
            e -= 1.0
        else:
            e -= (1.0 / self.sigma_epsilon) * (1.0 - 2.0 * s[3] + self._sigma_g)
        e *= 0.5 * self.n
        e -= s[5] - np.log(pi) * s[7]
        e -= s[6] - np.log(null_pi) * s[8]
        e += 0.5 * ((1.0 + np.log(tau_beta)) * s[7] - s[9])
        e -= 0.5 * tau_beta * s[1]
        return float(e)

    objective = elbo

    def mse(self, sum_axis=None):                                                      # :689-704
        s = self._current_sums()
        return 1.0 - 2.0 * s[3] + (self._sigma_g - s[1] + s[4])

    # ---- the ELBO's parts (VIPRS.py:583-687), from the same partial sums as `elbo` -----------------------
    def _current_sums(self):
        return self._sums if (self._sums is not None and self._sums_valid) else self._reduce()

    def entropy(self, sum_axis=None):
        """Entropy of the variational distribution (VIPRS.py:583-612)."""
        s = self._current_sums()
        return float(0.5 * self.n_snps * (np.log(2.0 * np.pi) + 1.0) - s[5] - s[6] - 0.5 * s[9])

    def loglikelihood(self):
        """Expected log-likelihood of the summary statistics (VIPRS.py:614-628)."""
        s = self._current_sums()
        return float(-0.5 * self.n * (np.log(2.0 * np.pi * self.sigma_epsilon)
                                      + (1.0 / self.sigma_epsilon) * (1.0 - 2.0 * s[3] + self._sigma_g)))

    def log_prior(self, sum_axis=None):
        """Expected log prior under the variational density (VIPRS.py:630-676)."""
        s = self._current_sums()
        lp = 0.5 * np.log(self.tau_beta) * s[7] + np.log(self.pi) * s[7] + np.log(self.get_null_pi()) * s[8]
        lp -= 0.5 * self.tau_beta * s[1]
        return float(lp - 0.5 * self.n_snps * np.log(2.0 * np.pi))

    def complete_loglikelihood(self):
        return self.loglikelihood() + self.log_prior()

    def get_heritability(self):
        return self._sigma_g / (self._sigma_g + self.sigma_epsilon)

    def get_proportion_causal(self):
        return self.pi

    def get_average_effect_size_variance(self):
        """Average per-SNP prior variance of the effect sizes, sum(pi / tau_beta) (VIPRS.py:764-778)."""
        return float(np.sum(np.asarray(self.pi, dtype=np.float64) / np.asarray(self.tau_beta, dtype=np.float64)))

    # ---- reporting (VIPRS.py:787-835) ------------------------------------------------------------------
    def to_theta_table(self):
        import pandas as pd
        rows = [("ELBO", self.elbo()), ("Residual_variance", self.sigma_epsilon), ("Heritability", self.get_heritability()),
                ("Proportion_causal", self.get_proportion_causal()),
                ("Average_effect_variance", self.get_average_effect_size_variance())]
        if np.isscalar(self.lambda_min):
            rows.append(("Lambda_min", self.lambda_min))
        taus = np.atleast_1d(np.asarray(self.tau_beta, dtype=np.float64))
        if taus.size == 1:
            rows.append(("tau_beta", float(taus[0])))
        else:
            rows += [(f"tau_beta_{i + 1}", float(t)) for i, t in enumerate(taus)]
        return pd.DataFrame([{"Parameter": k, "Value": v} for k, v in rows])

    def to_history_table(self):
        import pandas as pd
        return pd.DataFrame(self.history)

    def write_inferred_theta(self, f_name, sep="\t"):
        self.to_theta_table().to_csv(f_name, sep=sep, index=False)

    def update_theta_history(self):
        self._reduce()
        self.history["ELBO"].append(self.elbo())
        for t in self.tracked_params:
            if t == "pi":
                self.history["pi"].append(self.get_proportion_causal())
            elif t == "heritability":
                self.history["heritability"].append(self.get_heritability())
            elif t == "sigma_epsilon":
                self.history["sigma_epsilon"].append(self.sigma_epsilon)
            elif t == "tau_beta":
                self.history["tau_beta"].append(self.tau_beta)
            elif t == "sigma_g":
                self.history["sigma_g"].append(self._sigma_g)
            elif t == "max_eta_diff":
                self.history["max_eta_diff"].append(self._max_eta_diff)
            elif callable(t):
                self.sync_host()
                self.history[t.__name__].append(t(self))

    # ---- one EM iteration behind its E-step (VIPRS.py:995-1094) -------------------------------------------
    def _new_fit_progress(self, prev_elbo=-np.inf):
        """What the stopping rules carry from one iteration to the next."""
        return SimpleNamespace(prev_elbo=prev_elbo, prev_sigma_g=self._sigma_g, plateau=ConditionStreak(),
                               dropping=ConditionStreak())

    def _restart_state(self, theta_0, param_0):
        self.initialize_theta(theta_0)
        self.initialize_variational_parameters(param_0)

    def _after_e_step(self, i, st, theta_0, param_0, min_iter, f_abs_tol, x_abs_tol, patience):
        """M-step, history and the stopping rules of iteration `i`; the outcome goes to `self.optim_result`."""
        res = self.optim_result
        self.m_step()
        self.update_theta_history()
        max_eta_diff = self._max_eta_diff                                              # :997
        elbo = self.history["ELBO"][-1]
        prev_elbo = st.prev_elbo
        st.plateau.update((i > min_iter) and _isclose(self._sigma_g, st.prev_sigma_g, atol=x_abs_tol, rtol=0.0)
                          and max_eta_diff < x_abs_tol * 10, i)                        # :1003-1008
        st.dropping.update((elbo < prev_elbo) and not _isclose(elbo, prev_elbo, atol=1e3 * f_abs_tol, rtol=1e-4), i)

        stop = None                                                                    # (success, message)
        if self.mse() < 0.0:                                                           # :1025-1044
            if "sigma_epsilon" not in self.fix_params:
                logger.info("Iteration %d | MSE is negative; restarting with sigma_epsilon fixed.", i)
                self._restart_state(theta_0, param_0)
                self.fix_params["sigma_epsilon"] = self.sigma_epsilon = 0.95
                return
            stop = (False, f"The MSE is negative ({self.mse():.6f}).")
        elif not np.isfinite(elbo):
            stop = (False, "Objective (ELBO) is undefined.")
        elif self.sigma_epsilon < 0.0:
            stop = (False, "Residual variance estimate is negative.")
        elif self.get_heritability() > 1.0 or self.get_heritability() < 0.0:
            stop = (False, "Estimated heritability is out of bounds.")
        elif (i > min_iter) and _isclose(prev_elbo, elbo, atol=f_abs_tol, rtol=0.0):
            stop = (True, "Objective (ELBO) converged successfully.")
        elif (i > min_iter) and max_eta_diff < x_abs_tol:
            stop = (True, "Variational parameters converged successfully.")
        elif st.plateau.counter > patience:
            stop = (True, "LD-weighted variational parameters converged successfully.")
        elif st.dropping.counter > patience:
            stop = (False, "The objective (ELBO) is decreasing.")

        if stop is None:
            res.update(elbo)
        else:
            res.update(elbo, stop_iteration=True, success=stop[0], message=stop[1])
        st.prev_elbo, st.prev_sigma_g = elbo, self._sigma_g

    # ---- EM loop (VIPRS.py:909-1124): same stopping rules, evaluated on the reduced sums ------------
    def fit(self, max_iter=1000, theta_0=None, param_0=None, continued=False, disable_pbar=True, min_iter=3,
            f_abs_tol=1e-6, x_abs_tol=1e-6, patience=10, on_iteration=None, **kwargs):
        """`on_iteration(i)`: optional callback at the end of every EM iteration (progress reporting, timing)."""
        if not continued:
            self.initialize(theta_0, param_0)
            first = 1
            self.update_theta_history()
            prev_elbo = -np.inf
        else:
            first = len(self.history["ELBO"]) + 1
            self._reduce()
            self.optim_result.update(self.elbo(), increment=False)
            prev_elbo = self.elbo()
        st = self._new_fit_progress(prev_elbo)
        res = self.optim_result

        for i in range(first, first + max_iter):
            if res.stop_iteration:
                break
            self.e_step()
            self._after_e_step(i, st, theta_0, param_0, min_iter, f_abs_tol, x_abs_tol, patience)
            if on_iteration is not None:
                on_iteration(i)

        self.sync_host()
        self.update_posterior_moments()
        self._gather_posterior()
        if not res.stop_iteration:
            res.update(self.elbo(), stop_iteration=True, success=False, increment=False,
                       message="Maximum iterations reached without convergence.\n"
                               "You may need to run the model for more iterations.")
        if not res.success:
            logger.warning("\t%s", res.message)
        return self
