"""Python handles over the C ABI: ``LDPlan`` (device-resident LD + block schedule) and
``DeviceState`` (device-resident variational state).

``LDPlan`` replaces the "load LD matrices to memory" step of ``VIPRS.__init__``
(viprs/model/VIPRS.py:151-172 in the reference): the LD arrays are validated, partitioned into
independent LD blocks, uploaded and re-laid-out for the panel kernels once; every later E-step
only moves per-SNP vectors.
"""
import ctypes
import os
import weakref

import numpy as np

from . import _lib as L

_LIB = L                       # (for the methods that take an argument named L)

_FLOAT_CODE = {np.dtype(np.float32): L.F32, np.dtype(np.float64): L.F64}
_LD_CODE = {np.dtype(np.int8): L.LD_I8, np.dtype(np.int16): L.LD_I16, np.dtype(np.int32): L.LD_I32,
            np.dtype(np.int64): L.LD_I64, np.dtype(np.float32): L.LD_F32, np.dtype(np.float64): L.LD_F64}
_IP_CODE = {np.dtype(np.int32): L.IP_I32, np.dtype(np.int64): L.IP_I64}


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _check_index_arrays(ld_left_bound, ld_indptr):
    # same errors the Cython memoryviews raise (e_step_cpp.pyx:91-93: int[::1], indptr_type[::1])
    if not isinstance(ld_left_bound, np.ndarray) or ld_left_bound.dtype != np.int32:
        raise ValueError("Buffer dtype mismatch, expected 'int' but got "
                         f"'{getattr(ld_left_bound, 'dtype', type(ld_left_bound))}' (ld_left_bound)")
    if not isinstance(ld_indptr, np.ndarray) or ld_indptr.dtype not in _IP_CODE:
        raise ValueError("Buffer dtype mismatch, expected int32/int64 ld_indptr but got "
                         f"'{getattr(ld_indptr, 'dtype', type(ld_indptr))}'")
    for name, a in (("ld_left_bound", ld_left_bound), ("ld_indptr", ld_indptr)):
        if a.ndim != 1:
            raise ValueError(f"Buffer has wrong number of dimensions (expected 1, got {a.ndim}) ({name})")
        if not a.flags.c_contiguous:
            raise ValueError(f"ndarray is not C-contiguous ({name})")
    if ld_indptr.shape[0] != ld_left_bound.shape[0] + 1:
        raise ValueError("ld_indptr must have len(ld_left_bound) + 1 entries")


def plan_blocks(ld_left_bound, ld_indptr, low_memory):
    """Host-only block discovery (no GPU needed).  Returns ``(block_start, block_kind)`` with
    ``block_start`` of length ``n_blocks + 1``."""
    _check_index_arrays(ld_left_bound, ld_indptr)
    m = ld_left_bound.shape[0]
    n = ctypes.c_int64(0)
    starts = np.zeros(m + 1, dtype=np.int64)
    kinds = np.zeros(max(m, 1), dtype=np.int32)
    L.check(L.lib.viprs_plan_blocks(m, _ptr(ld_left_bound), _ptr(ld_indptr), _IP_CODE[ld_indptr.dtype],
                                    int(bool(low_memory)), ctypes.byref(n), _ptr(starts), _ptr(kinds)))
    return starts[: n.value + 1].copy(), kinds[: n.value].copy()


class RidgeInfo:
    """What a ridge solve reports: per LD block (SNP order) `iterations`, `relres` (the solver's own estimate of
    ||b - A x|| / ||b||) and `status` (0 converged, 1 stopped at maxiter, 2 zero right-hand side); `converged`: no block
    stopped at maxiter; `ms`: device time of the solve."""
    CONVERGED, MAXITER, ZERO_RHS = 0, 1, 2

    def __init__(self, iterations, relres, status, ms=0.0):
        self.iterations = np.asarray(iterations, dtype=np.int32)
        self.relres = np.asarray(relres, dtype=np.float64)
        self.status = np.asarray(status, dtype=np.int32)
        self.ms = float(ms)

    @property
    def converged(self):
        return bool(np.all(self.status != self.MAXITER))

    def __repr__(self):
        return (f"RidgeInfo(blocks={self.status.shape[0]}, converged={self.converged}, "
                f"max_iterations={int(self.iterations.max(initial=0))}, ms={self.ms:.3f})")


class SusieInfo:
    """What a SuSiE fit reports (`LDPlan.susie`, `viprs_amd.stats.susie.susie_host`): `alpha`, `mu` ``(m, L)``; per LD
    block (SNP order) `prior_variance`, `post_var` ``(n_blocks, L)``, `iterations`, `delta` (the last iteration's
    max |alpha - alpha_old|) and `status` (0 converged, 1 stopped at max_iter); `block_start` (``n_blocks + 1`` SNP offsets);
    `converged`: no block stopped at max_iter; `ms`: device time of the call."""
    CONVERGED, MAXITER = 0, 1

    def __init__(self, alpha, mu, prior_variance, post_var, iterations, delta, status, block_start, ms=0.0):
        self.alpha = np.asarray(alpha)
        self.mu = np.asarray(mu)
        self.prior_variance = np.asarray(prior_variance, dtype=np.float64)
        self.post_var = np.asarray(post_var, dtype=np.float64)
        self.iterations = np.asarray(iterations, dtype=np.int32)
        self.delta = np.asarray(delta, dtype=np.float64)
        self.status = np.asarray(status, dtype=np.int32)
        self.block_start = np.asarray(block_start, dtype=np.int64)
        self.ms = float(ms)

    @property
    def converged(self):
        return bool(np.all(self.status != self.MAXITER))

    def __repr__(self):
        return (f"SusieInfo(blocks={self.status.shape[0]}, L={self.alpha.shape[1] if self.alpha.ndim == 2 else 0}, "
                f"converged={self.converged}, max_iterations={int(self.iterations.max(initial=0))}, ms={self.ms:.3f})")


def susie_inputs(m, n_blocks, z, L, prior_variance, log_prior):
    """The arrays of a SuSiE call as the C ABI takes them: ``(z, prior_variance array or None, prior_variance0, log_prior or
    None)``.  Shapes are checked here; the values are the library's to refuse."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    if z.shape != (m,):
        raise ValueError(f"z: expected shape ({m},), got {z.shape}")
    v = np.asarray(prior_variance, dtype=np.float64)
    if v.ndim == 0:
        v, v0 = None, float(v)
    else:
        if v.shape != (n_blocks, int(L)):
            raise ValueError(f"prior_variance: expected a scalar or shape ({n_blocks}, {int(L)}), got {v.shape}")
        v, v0 = np.ascontiguousarray(v), 0.0
    lp = None
    if log_prior is not None:
        lp = np.ascontiguousarray(log_prior, dtype=np.float64)
        if lp.shape != (m,):
            raise ValueError(f"log_prior: expected shape ({m},), got {lp.shape}")
    return z, v, v0, lp


class SpectrumInfo:
    """What `LDPlan.extremal_eigenvalues` reports, per LD block (SNP order): `lambda_min` / `lambda_max` (the extreme Ritz
    values), `resid_min` / `resid_max` (absolute bounds of their distance to the nearest eigenvalue), `iterations`, `status`
    (0 converged, 1 stopped at maxiter); `converged`: no block stopped at maxiter; `ms`: time of the call on the device's
    clock, `host_ms`: the part the host spent on the tridiagonal eigenproblems."""
    CONVERGED, MAXITER = 0, 1

    def __init__(self, lambda_min, lambda_max, resid_min, resid_max, iterations, status, ms=0.0, host_ms=0.0):
        self.lambda_min = np.asarray(lambda_min, dtype=np.float64)
        self.lambda_max = np.asarray(lambda_max, dtype=np.float64)
        self.resid_min = np.asarray(resid_min, dtype=np.float64)
        self.resid_max = np.asarray(resid_max, dtype=np.float64)
        self.iterations = np.asarray(iterations, dtype=np.int32)
        self.status = np.asarray(status, dtype=np.int32)
        self.ms = float(ms)
        self.host_ms = float(host_ms)

    @property
    def converged(self):
        return bool(np.all(self.status == self.CONVERGED))

    def __repr__(self):
        lo = float(self.lambda_min.min()) if self.lambda_min.size else float("nan")
        hi = float(self.lambda_max.max()) if self.lambda_max.size else float("nan")
        return (f"SpectrumInfo(blocks={self.status.shape[0]}, min={lo:.6g}, max={hi:.6g}, converged={self.converged}, "
                f"max_iterations={int(self.iterations.max(initial=0))}, ms={self.ms:.3f})")


class LDPlan:
    """Device-resident LD matrix of one chromosome (or any set of LD blocks)."""

    def __init__(self, ld_left_bound, ld_indptr, ld_data, low_memory, device=0, math_mode="exact"):
        _check_index_arrays(ld_left_bound, ld_indptr)
        if not isinstance(ld_data, np.ndarray) or ld_data.dtype not in _LD_CODE:
            raise ValueError("Buffer dtype mismatch for ld_data: "
                             f"'{getattr(ld_data, 'dtype', type(ld_data))}' is not a supported LD dtype")
        if ld_data.ndim != 1 or not ld_data.flags.c_contiguous:
            raise ValueError("ld_data must be a C-contiguous 1-d array")
        self.m = int(ld_left_bound.shape[0])
        if self.m and int(ld_indptr[-1]) != ld_data.shape[0]:
            raise ValueError("ld_indptr[-1] must equal len(ld_data)")
        self.low_memory = bool(low_memory)
        self.ld_dtype = ld_data.dtype
        self.device = int(device)
        self._h = ctypes.c_void_p()
        L.check(L.lib.viprs_plan_create(ctypes.byref(self._h), self.m, _ptr(ld_left_bound), _ptr(ld_indptr),
                                        _IP_CODE[ld_indptr.dtype], _ptr(ld_data), _LD_CODE[ld_data.dtype],
                                        int(self.low_memory), self.device))
        self.set_math_mode(math_mode)

    @classmethod
    def from_upper(cls, ld_indptr, ld_data, diag_value=None, device=0, math_mode="exact"):
        """Symmetric plan (``low_memory=False`` arithmetic) from the compact upper-triangular store
        (row j = correlations with SNPs j+1 .. j+len_j): uploaded once and mirrored into the symmetric
        windows on the device -- the host never builds ``ld_mat.load(return_symmetric=True)``
        (VIPRS.py:167-172).  ``diag_value`` defaults to 1 for float LD and to the quantisation maximum
        (``np.iinfo(dtype).max``) for integer LD."""
        if not isinstance(ld_indptr, np.ndarray) or ld_indptr.dtype not in _IP_CODE:
            raise ValueError("Buffer dtype mismatch, expected int32/int64 ld_indptr but got "
                             f"'{getattr(ld_indptr, 'dtype', type(ld_indptr))}'")
        if ld_indptr.ndim != 1 or not ld_indptr.flags.c_contiguous or ld_indptr.shape[0] < 1:
            raise ValueError("ld_indptr must be a C-contiguous 1-d array with m + 1 entries")
        if not isinstance(ld_data, np.ndarray) or ld_data.dtype not in _LD_CODE:
            raise ValueError("Buffer dtype mismatch for ld_data: "
                             f"'{getattr(ld_data, 'dtype', type(ld_data))}' is not a supported LD dtype")
        if ld_data.ndim != 1 or not ld_data.flags.c_contiguous:
            raise ValueError("ld_data must be a C-contiguous 1-d array")
        self = cls.__new__(cls)
        self.m = int(ld_indptr.shape[0]) - 1
        if self.m and int(ld_indptr[-1]) != ld_data.shape[0]:
            raise ValueError("ld_indptr[-1] must equal len(ld_data)")
        if diag_value is None:
            diag_value = float(np.iinfo(ld_data.dtype).max) if np.issubdtype(ld_data.dtype, np.integer) else 1.0
        self.low_memory = False
        self.ld_dtype = ld_data.dtype
        self.device = int(device)
        self._h = ctypes.c_void_p()
        L.check(L.lib.viprs_plan_create_expanded(ctypes.byref(self._h), self.m, _ptr(ld_indptr),
                                                 _IP_CODE[ld_indptr.dtype], _ptr(ld_data), _LD_CODE[ld_data.dtype],
                                                 float(diag_value), self.device))
        self.set_math_mode(math_mode)
        return self

    @classmethod
    def synthetic(cls, ld, device=0, math_mode="exact"):
        """Plan of a `viprs_amd.utils.synthetic` "longrange" workload whose LD entries are GENERATED ON THE DEVICE
        (`viprs_plan_create_synthetic`): `ld` is the `SyntheticLD` skeleton (`make_ld(..., kind="longrange",
        data=False)`; a full one works too, its `ld_data` is ignored).  Bit-identical to `LDPlan(ld.ld_left_bound,
        ld.ld_indptr, make_ld(...).ld_data, ...)` (tests/test_synth_device.py); measurement support, not on the
        reference's path."""
        from .utils import synthetic as syn
        if ld.kind != "longrange" or ld.params is None:
            raise ValueError("LDPlan.synthetic: a 'longrange' SyntheticLD with its block parameters is needed")
        dt = np.dtype(ld.ld_dtype if ld.ld_data is None else ld.ld_data.dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.int8), np.dtype(np.int16)):
            raise ValueError("LDPlan.synthetic: float32, int8 or int16 LD")
        sizes = np.ascontiguousarray(np.diff(ld.block_start), dtype=np.int64)
        vecs = syn.longrange_device_params(sizes, ld.rho, ld.params)
        self = cls.__new__(cls)
        self.m = int(sizes.sum())
        self.low_memory = bool(ld.low_memory)
        self.ld_dtype = dt
        self.device = int(device)
        self._h = ctypes.c_void_p()
        L.check(L.lib.viprs_plan_create_synthetic(ctypes.byref(self._h), int(sizes.shape[0]), _ptr(sizes),
                                                  *[_ptr(v) for v in vecs], _LD_CODE[dt], int(self.low_memory),
                                                  self.device))
        self.set_math_mode(math_mode)
        return self

    def windows(self):
        """``(ld_left_bound int32, ld_indptr int64)`` of the plan's rows."""
        lb = np.zeros(self.m, dtype=np.int32)
        ip = np.zeros(self.m + 1, dtype=np.int64)
        L.check(L.lib.viprs_plan_get_windows(self.handle, _ptr(lb), _ptr(ip)))
        return lb, ip

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            # a DeviceState dereferences its plan when it is destroyed (closing the plan first would be a
            # use-after-free on the C side): the plan closes the states that are still open before it goes
            for st in list(getattr(self, "_states", ())):
                st.close()
            L.lib.viprs_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise ValueError("LDPlan is closed")
        return self._h

    # -- queries ------------------------------------------------------------------------------
    def info(self, key):
        v = ctypes.c_int64(0)
        L.check(L.lib.viprs_plan_info(self.handle, key, ctypes.byref(v)))
        return v.value

    @property
    def n_blocks(self):
        return self.info(L.INFO_N_BLOCKS)

    @property
    def nnz(self):
        return self.info(L.INFO_NNZ)

    def blocks(self):
        n = self.n_blocks
        starts = np.zeros(n + 1, dtype=np.int64)
        kinds = np.zeros(max(n, 1), dtype=np.int32)
        L.check(L.lib.viprs_plan_get_blocks(self.handle, _ptr(starts), _ptr(kinds)))
        return starts, kinds[:n]

    def set_active_blocks(self, active):
        """Which LD blocks the following sweeps visit: a boolean per block in SNP order (`blocks()`), None = all of them
        (`viprs_plan_set_active_blocks`).  Every kernel family sweeps the active subset, the batched grid kernel included."""
        if active is None:
            L.check(L.lib.viprs_plan_set_active_blocks(self.handle, None, 0))
            return
        a = np.ascontiguousarray(active, dtype=np.uint8)
        L.check(L.lib.viprs_plan_set_active_blocks(self.handle, _ptr(a), int(a.shape[0])))

    def set_math_mode(self, mode):
        code = {"exact": L.MATH_EXACT, "fast": L.MATH_FAST}.get(mode, mode)
        L.check(L.lib.viprs_plan_set_math_mode(self.handle, int(code)))
        self.math_mode = "exact" if code == L.MATH_EXACT else "fast"

    def last_kernel_ms(self, which=0):
        ms = ctypes.c_double(0.0)
        L.check(L.lib.viprs_plan_last_kernel_ms(self.handle, int(which), ctypes.byref(ms)))
        return ms.value

    def timing_reset(self):
        L.check(L.lib.viprs_plan_timing_reset(self.handle))

    def timing_history(self, which=0, capacity=256):
        """HIP-event durations (ms) of the most recent sweeps, oldest first (which: 0 = whole sweep,
        1 = panel kernel(s) only, 2 = host ms inside that kernel's event bracket; a sweep that brackets no such kernel
        reports 0 for 1 and 2)."""
        buf = (ctypes.c_double * capacity)()
        n = ctypes.c_int(0)
        L.check(L.lib.viprs_plan_timing_history(self.handle, int(which), buf, capacity, ctypes.byref(n)))
        return [buf[i] for i in range(n.value)]

    def effective_math_mode(self):
        """'exact' / 'fast' / 'mixed': what the kernels of the last sweep really computed in (fast has no instantiation for
        mixtures of 9+ components or float64 states: those run exact whatever `set_math_mode` was given); None before
        the first sweep."""
        mask = ctypes.c_int(0)
        L.check(L.lib.viprs_plan_last_math_modes(self.handle, ctypes.byref(mask)))
        return {0: None, 1: "exact", 2: "fast", 3: "mixed"}[mask.value & 3]

    def last_skipped(self):
        n = ctypes.c_int64(0)
        L.check(L.lib.viprs_plan_last_skipped(self.handle, ctypes.byref(n)))
        return n.value

    # -- LD product ---------------------------------------------------------------------------
    def dot(self, B, dq_scale=1.0, include_diagonal=True):
        """``R @ B`` over every block of the plan (`viprs_plan_dot`; the reference's ``ld.dot(B)``): `B` is ``(m,)`` or
        ``(m, G)``, float32 or float64, in either memory order; the result has the caller's shape and dtype.  `R` has a
        unit diagonal and off-diagonal entries ``dq_scale * stored``; ``include_diagonal=False`` leaves the diagonal out
        (the ``q`` of a given ``eta``).  `set_active_blocks` does not filter the product."""
        B = np.asarray(B)
        if B.dtype not in _FLOAT_CODE:
            raise ValueError(f"Buffer dtype mismatch for B: expected float32 or float64, got {B.dtype}")
        if B.ndim not in (1, 2) or B.shape[0] != self.m or (B.ndim == 2 and B.shape[1] < 1):
            raise ValueError(f"B: expected shape ({self.m},) or ({self.m}, G), got {B.shape}")
        b = np.asfortranarray(B)
        y = np.empty(b.shape, dtype=b.dtype, order="F")
        n_cols = 1 if b.ndim == 1 else int(b.shape[1])
        if self.m == 0:
            return y
        L.check(L.lib.viprs_plan_dot(self.handle, _FLOAT_CODE[b.dtype], n_cols, _ptr(b), _ptr(y), float(dq_scale),
                                     int(bool(include_diagonal))))
        return y

    def last_dot_ms(self):
        """HIP-event time (ms) of the kernels of the last product on this plan (`dot`, `DeviceState.dot`)."""
        ms = ctypes.c_double(0.0)
        L.check(L.lib.viprs_plan_last_dot_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    # -- LD scores ----------------------------------------------------------------------------
    def ld_scores(self, weights=None, correction=None, dq_scale=1.0, float_precision="float32"):
        """LD scores ``l[j, g] = sum_k A[k, g] r_jk^2`` over every block of the plan (`viprs_plan_ld_scores`; magenpy's
        ``compute_ld_scores``).  `weights`: None (one column of ones, the unstratified scores; the result is ``(m,)`` in
        `float_precision`) or an ``(m,)`` / ``(m, G)`` float32 / float64 array of annotations (the result has its shape and
        dtype).  `correction`: None or ``(m,)`` values ``c_j`` -- every off-diagonal ``r^2`` becomes ``r^2 - (1 - r^2) c_j``
        (``c = 1 / (n_LD - 2)``: the adjusted r^2 of LD-score regression).  `R` as in `dot`: unit diagonal, off-diagonal
        entries ``dq_scale * stored``.  `set_active_blocks` does not filter the call."""
        if weights is None:
            dt = np.dtype(float_precision)
            if dt not in _FLOAT_CODE:
                raise ValueError(f"float_precision: expected float32 or float64, got {float_precision}")
            a = None
            y = np.empty(self.m, dtype=dt)
            n_cols = 1
        else:
            A = np.asarray(weights)
            if A.dtype not in _FLOAT_CODE:
                raise ValueError(f"Buffer dtype mismatch for weights: expected float32 or float64, got {A.dtype}")
            if A.ndim not in (1, 2) or A.shape[0] != self.m or (A.ndim == 2 and A.shape[1] < 1):
                raise ValueError(f"weights: expected shape ({self.m},) or ({self.m}, G), got {A.shape}")
            a = np.asfortranarray(A)
            dt = a.dtype
            y = np.empty(a.shape, dtype=dt, order="F")
            n_cols = 1 if a.ndim == 1 else int(a.shape[1])
        c = None
        if correction is not None:
            c = np.ascontiguousarray(correction, dtype=np.float64)
            if c.shape != (self.m,):
                raise ValueError(f"correction: expected shape ({self.m},), got {c.shape}")
        if self.m == 0:
            return y
        L.check(L.lib.viprs_plan_ld_scores(self.handle, _FLOAT_CODE[dt], n_cols, _ptr(a), _ptr(c), _ptr(y), float(dq_scale)))
        return y

    def last_ld_score_ms(self):
        """HIP-event time (ms) of the kernels of the last `ld_scores` on this plan."""
        ms = ctypes.c_double(0.0)
        L.check(L.lib.viprs_plan_last_ld_score_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    # -- LD clumping --------------------------------------------------------------------------
    def clump(self, order, r2, member=None, dq_scale=1.0):
        """Greedy LD clumping over every block of the plan (`viprs_plan_clump`): `order` holds distinct SNP indices, most
        significant first; each SNP of it that is still available becomes an index SNP and claims the available SNPs in LD
        with it at ``(dq_scale * stored)^2 >= r2``.  Returns ``index_of``: int32 ``(m,)`` for a scalar `r2`, ``(m, G)``
        (column-major) for a sequence of up to 32 thresholds, one independent clumping per column; -1 where no index SNP
        claimed the SNP.  `member`: ``(m,)`` booleans, the SNPs that may belong to a clump (None: all); every SNP of `order`
        must be one.  `set_active_blocks` does not filter the call."""
        scalar = np.ndim(r2) == 0
        thr = np.ascontiguousarray(np.atleast_1d(r2), dtype=np.float64)
        if thr.ndim != 1:
            raise ValueError(f"r2: expected a scalar or a 1-d sequence, got shape {thr.shape}")
        o = np.asarray(order)
        if o.ndim != 1 or (o.size and not np.issubdtype(o.dtype, np.integer)):
            raise ValueError(f"order: expected a 1-d integer array, got {o.dtype} of shape {o.shape}")
        if o.size and (int(o.min()) < 0 or int(o.max()) >= self.m):
            raise ValueError(f"order: SNP indices must be in [0, {self.m})")
        o = np.ascontiguousarray(o, dtype=np.int32)
        mem = None
        if member is not None:
            mem = np.ascontiguousarray(np.asarray(member) != 0, dtype=np.uint8)
            if mem.shape != (self.m,):
                raise ValueError(f"member: expected shape ({self.m},), got {mem.shape}")
        n_cols = int(thr.shape[0])
        out = np.full((self.m, n_cols), -1, dtype=np.int32, order="F")
        L.check(L.lib.viprs_plan_clump(self.handle, int(o.shape[0]), _ptr(o), _ptr(mem), n_cols, _ptr(thr), float(dq_scale),
                                       _ptr(out)))
        return out[:, 0] if scalar else out

    def last_gibbs_draws_ms(self):
        """Event time (ms) of the last Gibbs draws kernel on this plan (`viprs_plan_last_gibbs_draws_ms`)."""
        ms = ctypes.c_double()
        L.check(L.lib.viprs_plan_last_gibbs_draws_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def last_bayesr_draws_ms(self):
        """Event time (ms) of the last SBayesR draws kernel (`viprs_plan_last_bayesr_draws_ms`)."""
        ms = ctypes.c_double()
        L.check(L.lib.viprs_plan_last_bayesr_draws_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def last_cs_ms(self):
        """Event times (ms) of the last PRS-CS variates kernel and of the last update kernel on this plan
        (`viprs_plan_last_cs_ms`; 0 for one that has not run)."""
        v, u = ctypes.c_double(), ctypes.c_double()
        L.check(L.lib.viprs_plan_last_cs_ms(self.handle, ctypes.byref(v), ctypes.byref(u)))
        return v.value, u.value

    def last_clump_ms(self):
        """HIP-event time (ms) of the kernels of the last `clump` on this plan."""
        ms = ctypes.c_double(0.0)
        L.check(L.lib.viprs_plan_last_clump_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    # -- ridge solve -----------------------------------------------------------------------------
    def solve_ridge(self, b, shift, dq_scale=1.0, rtol=None, maxiter=None, x0=None, check_every=4):
        """``(R + diag(shift)) x = b`` by one MINRES per LD block, all blocks in lock step (`viprs_plan_solve_ridge`; what
        the reference's ``LDPredInf.fit`` asks of scipy over one assembled matrix).  `b`: ``(m,)`` float32 or float64, `x`
        has its dtype; `shift`: a scalar or ``(m,)``; `R` as in `dot` with the diagonal.  Defaults: ``rtol`` 1e-5
        (float32) / 1e-10 (float64), ``maxiter`` 5 x the largest block (scipy's ``5 n``, per block).  Returns
        ``(x, info)``: `info.iterations / relres / status` per block in SNP order (`RidgeInfo`), `info.converged`, `info.ms`.
        `set_active_blocks` does not filter the solve."""
        b = np.asarray(b)
        if b.dtype not in _FLOAT_CODE:
            raise ValueError(f"Buffer dtype mismatch for b: expected float32 or float64, got {b.dtype}")
        if b.shape != (self.m,):
            raise ValueError(f"b: expected shape ({self.m},), got {b.shape}")
        b = np.ascontiguousarray(b)
        sh = np.asarray(shift, dtype=np.float64)
        if sh.ndim == 0:
            sh = np.full(self.m, float(sh))
        if sh.shape != (self.m,):
            raise ValueError(f"shift: expected a scalar or shape ({self.m},), got {sh.shape}")
        sh = np.ascontiguousarray(sh)
        if x0 is not None:
            x0 = np.ascontiguousarray(x0)
            if x0.dtype != b.dtype or x0.shape != b.shape:
                raise ValueError(f"x0: expected {b.dtype} of shape {b.shape}, got {x0.dtype} of shape {x0.shape}")
        if rtol is None:
            rtol = 1e-5 if b.dtype == np.float32 else 1e-10
        starts = self.blocks()[0]
        n_blocks = len(starts) - 1
        if maxiter is None:
            maxiter = 5 * int(np.max(np.diff(starts))) if n_blocks else 1
        x = np.empty_like(b)
        iters = np.zeros(n_blocks, dtype=np.int32)
        relres = np.zeros(n_blocks, dtype=np.float64)
        status = np.zeros(n_blocks, dtype=np.int32)
        L.check(L.lib.viprs_plan_solve_ridge(self.handle, _FLOAT_CODE[b.dtype], _ptr(b), _ptr(sh), _ptr(x0), _ptr(x),
                                             float(dq_scale), float(rtol), int(maxiter), int(check_every),
                                             _ptr(iters), _ptr(relres), _ptr(status)))
        ms = self.last_solve_ms()[0] if self.m else 0.0
        return x, RidgeInfo(iters, relres, status, ms)

    def last_solve_ms(self):
        """``(ms, iterations)`` of the last `solve_ridge` on this plan: HIP-event time from its first to its last kernel and
        the iterations it launched (the largest per-block count, rounded up to the next read-back of the loop)."""
        ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
        L.check(L.lib.viprs_plan_last_solve_ms(self.handle, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    # -- SuSiE fine-mapping ------------------------------------------------------------------------
    def susie(self, z, L=10, prior_variance=50.0, estimate_prior_variance=True, log_prior=None, dq_scale=1.0, tol=1e-4,
              max_iter=100, check_every=4, float_precision="float32"):
        """SuSiE-RSS on z-scores, one fit of `L` single effects per LD block, all blocks in lock step (`viprs_plan_susie`):
        ``z ~ N(R b, R)``, `R` as in `dot` with the diagonal.  `z`: ``(m,)``; `prior_variance`: a scalar or
        ``(n_blocks, L)``, the start of the EM update with `estimate_prior_variance`; `log_prior`: ``(m,)`` log pi_j (-inf
        excludes a SNP), None: uniform over each block.  Returns a `SusieInfo`; `alpha` and `mu` are ``(m, L)`` in
        `float_precision`.  `set_active_blocks` does not filter the call."""
        dt = np.dtype(float_precision)
        if dt not in _FLOAT_CODE:
            raise ValueError(f"float_precision: expected float32 or float64, got {float_precision}")
        starts = self.blocks()[0]
        n_blocks = len(starts) - 1
        z, v, v0, lp = susie_inputs(self.m, n_blocks, z, L, prior_variance, log_prior)
        L_ = int(L)
        alpha = np.zeros((self.m, max(L_, 0)), dtype=dt, order="F")
        mu = np.zeros((self.m, max(L_, 0)), dtype=dt, order="F")
        v_out = np.zeros((n_blocks, max(L_, 0)))
        post_var = np.zeros((n_blocks, max(L_, 0)))
        iters = np.zeros(n_blocks, dtype=np.int32)
        delta = np.zeros(n_blocks)
        status = np.zeros(n_blocks, dtype=np.int32)
        _LIB.check(_LIB.lib.viprs_plan_susie(self.handle, _FLOAT_CODE[dt], L_, _ptr(z), _ptr(lp), _ptr(v), float(v0),
                                       int(bool(estimate_prior_variance)), float(dq_scale), float(tol), int(max_iter),
                                       int(check_every), _ptr(alpha), _ptr(mu), _ptr(v_out), _ptr(post_var), _ptr(iters),
                                       _ptr(delta), _ptr(status)))
        ms = self.last_susie_ms()[0] if self.m else 0.0
        return SusieInfo(alpha, mu, v_out, post_var, iters, delta, status, starts, ms)

    def last_susie_ms(self):
        """``(ms, steps, step_kernel_ms)`` of the last `susie` on this plan: HIP-event time from its first to its last
        kernel, the step kernels it launched, and the time of one step kernel (effect L - 1 of iteration 1: every block is
        still running)."""
        ms, n, step = ctypes.c_double(0.0), ctypes.c_int(0), ctypes.c_double(0.0)
        L.check(L.lib.viprs_plan_last_susie_ms(self.handle, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(step)))
        return ms.value, n.value, step.value

    # -- extremal eigenvalues ---------------------------------------------------------------------
    def extremal_eigenvalues(self, dq_scale=1.0, rtol=None, maxiter=None, float_precision="float32"):
        """Smallest and largest eigenvalue of every LD block by one Lanczos recurrence per block, all blocks in lock step
        (`viprs_plan_extremal_eigenvalues`; what magenpy computes with ARPACK when it builds an LD store).  `R` as in `dot`
        with the diagonal; the recurrence's vectors are in `float_precision`.  Defaults: ``rtol`` 1e-4 (a tenth of the
        ``min_max_ratio`` 1e-3 the models resolve), ``maxiter`` 2048.  Returns a `SpectrumInfo`.  `set_active_blocks` does
        not filter the computation."""
        dt = np.dtype(float_precision)
        if dt not in _FLOAT_CODE:
            raise ValueError(f"float_precision: expected float32 or float64, got {float_precision}")
        rtol = 1e-4 if rtol is None else float(rtol)
        maxiter = 2048 if maxiter is None else int(maxiter)
        n_blocks = self.n_blocks
        lo, hi = np.zeros(n_blocks), np.zeros(n_blocks)
        r_lo, r_hi = np.zeros(n_blocks), np.zeros(n_blocks)
        iters = np.zeros(n_blocks, dtype=np.int32)
        status = np.zeros(n_blocks, dtype=np.int32)
        L.check(L.lib.viprs_plan_extremal_eigenvalues(self.handle, _FLOAT_CODE[dt], float(dq_scale), rtol, maxiter,
                                                      _ptr(lo), _ptr(hi), _ptr(r_lo), _ptr(r_hi), _ptr(iters),
                                                      _ptr(status)))
        ms, _, host_ms = self.last_spectrum_ms() if self.m else (0.0, 0, 0.0)
        return SpectrumInfo(lo, hi, r_lo, r_hi, iters, status, ms, host_ms)

    def last_spectrum_ms(self):
        """``(ms, iterations, host_ms)`` of the last `extremal_eigenvalues` on this plan: HIP-event time from its first to
        its last kernel (the checks of the stopping rule included), the iterations it launched, and the host's time inside
        those checks."""
        ms, n, host = ctypes.c_double(0.0), ctypes.c_int(0), ctypes.c_double(0.0)
        L.check(L.lib.viprs_plan_last_spectrum_ms(self.handle, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(host)))
        return ms.value, n.value, host.value

    # -- one-shot host-buffer E-steps (drop-ins for the Cython entry points) -------------------
    def e_step(self, std_beta, var_gamma, var_mu, eta, q, eta_diff, u_logs, sqrt_half_var_tau, mu_mult,
               dq_scale, threads=1, low_memory=None):
        T = _FLOAT_CODE[std_beta.dtype]
        low_memory = self.low_memory if low_memory is None else low_memory
        L.check(L.lib.viprs_e_step(self.handle, T, _ptr(std_beta), _ptr(var_gamma), _ptr(var_mu), _ptr(eta),
                                   _ptr(q), _ptr(eta_diff), _ptr(u_logs), _ptr(sqrt_half_var_tau),
                                   _ptr(mu_mult), float(dq_scale), int(threads), int(bool(low_memory))))

    def e_step_mixture(self, std_beta, var_gamma, var_mu, eta, q, eta_diff, log_null_pi, u_logs,
                       sqrt_half_var_tau, mu_mult, dq_scale, threads=1, low_memory=None):
        T = _FLOAT_CODE[std_beta.dtype]
        low_memory = self.low_memory if low_memory is None else low_memory
        K = var_mu.shape[1]
        L.check(L.lib.viprs_e_step_mixture(self.handle, T, int(K), _ptr(std_beta), _ptr(var_gamma), _ptr(var_mu),
                                           _ptr(eta), _ptr(q), _ptr(eta_diff), _ptr(log_null_pi), _ptr(u_logs),
                                           _ptr(sqrt_half_var_tau), _ptr(mu_mult), float(dq_scale),
                                           int(threads), int(bool(low_memory))))

    def e_step_grid(self, std_beta, var_gamma, var_mu, eta, q, eta_diff, u_logs, half_var_tau, mu_mult,
                    dq_scale, active_model_idx, threads=1, low_memory=None):
        T = _FLOAT_CODE[std_beta.dtype]
        low_memory = self.low_memory if low_memory is None else low_memory
        G = var_mu.shape[1]
        active = np.ascontiguousarray(active_model_idx, dtype=np.int32)
        L.check(L.lib.viprs_e_step_grid(self.handle, T, int(G), _ptr(std_beta), _ptr(var_gamma), _ptr(var_mu),
                                        _ptr(eta), _ptr(q), _ptr(eta_diff), _ptr(u_logs), _ptr(half_var_tau),
                                        _ptr(mu_mult), float(dq_scale), _ptr(active), int(active.shape[0]),
                                        int(threads), int(bool(low_memory))))


class DeviceState:
    """Variational state + per-SNP inputs of one plan, resident in HBM across EM iterations."""

    FIELDS = {
        "std_beta": L.FIELD_STD_BETA, "u_logs": L.FIELD_U_LOGS,
        "sqrt_half_var_tau": L.FIELD_SQRT_HALF_VAR_TAU, "half_var_tau": L.FIELD_SQRT_HALF_VAR_TAU,
        "mu_mult": L.FIELD_MU_MULT, "log_null_pi": L.FIELD_LOG_NULL_PI, "var_gamma": L.FIELD_VAR_GAMMA,
        "var_mu": L.FIELD_VAR_MU, "eta": L.FIELD_ETA, "q": L.FIELD_Q, "eta_diff": L.FIELD_ETA_DIFF,
    }

    # Placement probe (see `_probe_placement`): candidates tried / smallest plan it is worth it for
    PLACEMENT_CANDIDATES = 6
    PLACEMENT_MIN_SNPS = 200_000

    def __init__(self, plan, float_precision="float32", model="spike_slab", width=1, placement=None):
        self.plan = plan
        self.dtype = np.dtype(float_precision)
        self.model = model
        self.width = int(width)
        self._kind = {"spike_slab": L.MODEL_SPIKE_SLAB, "mixture": L.MODEL_MIXTURE, "grid": L.MODEL_GRID}[model]
        self._h = self._create()
        self.placement = None
        if not hasattr(plan, "_states"):
            plan._states = weakref.WeakSet()
        plan._states.add(self)
        mode = placement if placement is not None else os.environ.get("VIPRS_STATE_PLACEMENT", "probe")
        # (stream-bound sweeps only: fp32 state on the panel kernels -- dense blocks, mixtures of up to 8 components; a plan of
        #  windowed components or a wide mixture is chain-bound and has no panel-kernel bracket to rank candidates by)
        if (mode == "probe" and self.dtype == np.float32 and model in ("spike_slab", "mixture") and self.width <= 8
                and plan.m >= self.PLACEMENT_MIN_SNPS and plan.info(L.INFO_N_DENSE) > 0):
            own = self._h
            try:
                self._probe_placement()
            except Exception as e:              # noqa: BLE001 -- a usable state exists: the probe must never fail the constructor
                # (out of memory on the extra candidates, a team hand-off time-out when another process shares the GPU ...)
                if self._h is not own and self._h:
                    try:
                        L.lib.viprs_state_destroy(self._h)
                    except Exception:           # noqa: BLE001
                        pass
                self._h = own
                self.placement = {"error": f"{type(e).__name__}: {e}"[:200], "chosen": 0}
                try:                            # hand out what the caller was promised: a zeroed state
                    self._zero_fields()
                    self.plan.timing_reset()
                except Exception:               # noqa: BLE001
                    pass

    def _create(self):
        h = ctypes.c_void_p()
        L.check(L.lib.viprs_state_create(ctypes.byref(h), self.plan.handle, _FLOAT_CODE[self.dtype], self._kind, self.width))
        return h

    def _probe_placement(self):
        """WHERE the allocator puts a state's per-SNP arrays moves the stream-bound sweeps by up to 8 % (four levels
        2.6 % apart on cfg3: same plan, same kernels, same memory counters -- EXPERIMENTS.md round 5); the level is fixed
        for the life of the allocation.  So a large fp32 state is allocated `PLACEMENT_CANDIDATES` times, each candidate
        sweeps a synthetic input a few times (a sweep from the standard start on typical hyper-parameters: every LD
        entry is streamed), the fastest one is kept and handed out zeroed, the others are freed.  ~0.1 s once per fit;
        `VIPRS_STATE_PLACEMENT=off` (or `placement="off"`) skips it.  `self.placement` records what was measured."""
        from .utils import synthetic as syn
        m, K, T = self.plan.m, self.width, self.dtype
        rng = np.random.default_rng(12345)

        class _SS:
            n_per_snp = np.full(m, 1e5)
        beta = (0.01 * rng.standard_normal(m)).astype(T)
        if self.model == "spike_slab":
            inp = syn.make_inputs(type("S", (), {"std_beta": beta, "n_per_snp": _SS.n_per_snp})())
            fields = {"std_beta": beta, "u_logs": inp.u_logs, "sqrt_half_var_tau": inp.sqrt_half_var_tau, "mu_mult": inp.mu_mult}
            pi0 = inp.pi
        else:
            mix = syn.make_mixture_inputs(_SS, K, float_precision=T)
            pi0 = mix.pop("pi")
            fields = dict(mix, std_beta=beta)
        itemsize = np.dtype(self.plan.ld_dtype).itemsize
        dq = 1.0 if np.issubdtype(np.dtype(self.plan.ld_dtype), np.floating) else 1.0 / (2 ** (8 * itemsize - 1) - 1)
        own, handles, times = self._h, [self._h], []
        try:
            for _ in range(self.PLACEMENT_CANDIDATES - 1):
                handles.append(self._create())

            def sweeps(h, n):
                self._h = h
                self.plan.timing_reset()
                for _ in range(n):
                    self.reset(pi0)
                    self.e_step(dq, sync=False)
                self.synchronize()
                return self.plan.timing_history(which=1)
            for h in handles:
                self._h = h
                for k, a in fields.items():
                    self.upload(k, a)
            sweeps(handles[0], 40)                                   # clocks up before anything is compared
            times = [[] for _ in handles]
            for _ in range(2):                                       # two rounds: no candidate is only measured early
                for i, h in enumerate(handles):
                    times[i] += list(sweeps(h, 5))
            mins = [min(t) if t else 0.0 for t in times]
            # no decision when the timings say nothing: no panel-kernel bracket (zeros) or all candidates level (< 0.2 %)
            decided = min(mins) > 0.0 and (max(mins) - min(mins)) > 2e-3 * min(mins)
            best = int(np.argmin(mins)) if decided else 0
            self._h = handles[best]
            self._zero_fields()                                      # handed out as a fresh state: all zeros
            self.plan.timing_reset()
            self.placement = {"candidates": len(handles), "chosen": best, "decided": bool(decided),
                              "kernel_ms_min": [round(float(x), 4) for x in mins]}
        finally:
            keep = self._h if self._h in handles else own
            for h in handles:
                if h is not keep and h:
                    L.lib.viprs_state_destroy(h)
            self._h = keep

    def _zero_fields(self):
        T, m = self.dtype, self.plan.m
        zero = {k: np.zeros(self._shape(k), dtype=T) for k in
                ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult", "var_gamma", "var_mu", "eta", "q", "eta_diff")}
        if self.model == "mixture":
            zero["log_null_pi"] = np.zeros(m, dtype=T)
        for k, a in zero.items():
            self.upload(k, a)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib.viprs_state_destroy(self._h)
            self._h = ctypes.c_void_p()
            self.plan._states.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self, name):
        m = self.plan.m
        if self.model == "spike_slab" or name in ("std_beta", "log_null_pi"):
            return (m,)
        if self.model == "mixture":
            return (m,) if name in ("eta", "q", "eta_diff") else (m, self.width)
        return (m, self.width)

    def upload(self, name, array):
        shape = self._shape(name)
        order = "F" if self.model == "grid" and len(shape) == 2 else "C"
        if array.dtype != self.dtype:
            raise ValueError(f"Buffer dtype mismatch for {name}: expected {self.dtype}, got {array.dtype}")
        if tuple(array.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {array.shape}")
        a = np.asarray(array, order=order)
        if (order == "F" and not a.flags.f_contiguous) or (order == "C" and not a.flags.c_contiguous):
            raise ValueError(f"ndarray is not {'Fortran' if order == 'F' else 'C'} contiguous ({name})")
        L.check(L.lib.viprs_state_upload(self._h, self.FIELDS[name], _ptr(a)))

    def download(self, name, out=None):
        shape = self._shape(name)
        order = "F" if self.model == "grid" and len(shape) == 2 else "C"
        if out is None:
            out = np.empty(shape, dtype=self.dtype, order=order)
        else:                                   # the C side copies field_elems * itemsize bytes whatever it is handed
            if not isinstance(out, np.ndarray) or out.dtype != self.dtype:
                raise ValueError(f"Buffer dtype mismatch for {name}: expected {self.dtype}, got "
                                 f"{getattr(out, 'dtype', type(out))}")
            if tuple(out.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {out.shape}")
            if (order == "F" and not out.flags.f_contiguous) or (order == "C" and not out.flags.c_contiguous):
                raise ValueError(f"ndarray is not {'Fortran' if order == 'F' else 'C'} contiguous ({name})")
            if not out.flags.writeable:
                raise ValueError(f"{name}: output array is read-only")
        L.check(L.lib.viprs_state_download(self._h, self.FIELDS[name], _ptr(out)))
        return out

    def reset(self, pi):
        L.check(L.lib.viprs_state_reset(self._h, float(pi)))

    def set_comm(self, comm):
        """Attach an ``RcclComm`` (None detaches): `sums_begin / sums_end` (and the mixture / grid-column
        variants) then return the sums over ALL ranks -- one all-gather + rank-ordered reduction on the
        plan's stream per call (`viprs_state_set_comm`)."""
        self._comm = comm                       # keeps the communicator alive as long as the state uses it
        L.check(L.lib.viprs_state_set_comm(self._h, comm.handle if comm is not None else None))

    # -- device-resident EM iteration (spike-and-slab) ------------------------------------------
    def set_n_per_snp(self, n_per_snp):
        n = np.ascontiguousarray(n_per_snp, dtype=np.float64)
        if n.shape != (self.plan.m,):
            raise ValueError(f"n_per_snp: expected shape ({self.plan.m},), got {n.shape}")
        L.check(L.lib.viprs_state_set_n_per_snp(self._h, _ptr(n)))

    def set_snp_weights(self, weights):
        """Per-SNP weights of sum [0] (None clears): 1 / (SNPs of the chromosome) when several chromosomes
        share this plan, so that sum [0] is the reference's sum of per-chromosome means of gamma."""
        if weights is None:
            L.check(L.lib.viprs_state_set_snp_weights(self._h, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (self.plan.m,):
            raise ValueError(f"weights: expected shape ({self.plan.m},), got {w.shape}")
        L.check(L.lib.viprs_state_set_snp_weights(self._h, _ptr(w)))

    def prep(self, logit_pi, log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda):
        """VIPRS.py:400-418 on the device (asynchronous on the plan's stream).  The scalars are
        evaluated by the caller (reference dtype semantics)."""
        L.check(L.lib.viprs_state_prep(self._h, float(logit_pi), float(log_tau_beta), float(sigma_epsilon),
                                       float(tau_beta), float(one_plus_lambda)))

    def sums(self, one_plus_lambda):
        """The M-step / ELBO partial sums of this plan's SNPs (float64, deterministic order)."""
        out = (ctypes.c_double * L.N_SUMS)()
        L.check(L.lib.viprs_state_sums(self._h, float(one_plus_lambda), out))
        return np.array(out[:], dtype=np.float64)

    def sums_begin(self, one_plus_lambda):
        """Enqueue the reduction (asynchronous); `sums_end` collects it.  Lets several chromosomes reduce
        concurrently instead of one synchronisation per chromosome."""
        L.check(L.lib.viprs_state_sums_begin(self._h, float(one_plus_lambda)))

    def sums_end(self):
        out = (ctypes.c_double * L.N_SUMS)()
        L.check(L.lib.viprs_state_sums_end(self._h, out))
        return np.array(out[:], dtype=np.float64)

    # -- SNP groups: one model per chromosome in one state ---------------------------------------
    def set_groups(self, group_start):
        """Contiguous SNP ranges (whole LD blocks) with their own hyper-parameters and sums: `group_start` has
        n_groups + 1 entries from 0 to m; None removes the groups."""
        if group_start is None:
            L.check(L.lib.viprs_state_set_groups(self._h, 0, None))
            self.n_groups = 0
            return
        gs = np.ascontiguousarray(group_start, dtype=np.int64)
        L.check(L.lib.viprs_state_set_groups(self._h, int(gs.shape[0]) - 1, _ptr(gs)))
        self.n_groups = int(gs.shape[0]) - 1

    def prep_groups(self, params):
        """`prep` with per-group scalars: rows (group, logit_pi, log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda)."""
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 6)
        L.check(L.lib.viprs_state_prep_groups(self._h, int(p.shape[0]), _ptr(p)))

    def _sums_rows_begin(self, begin, *ids, one_plus_lambda):
        """Enqueues the sums of the rows (ids[0][i], ..., one_plus_lambda[i]) with the C call `begin`."""
        n = len(ids[0])
        r = np.ascontiguousarray(np.column_stack([np.asarray(x, dtype=np.float64) for x in ids] +
                                                 [np.broadcast_to(np.asarray(one_plus_lambda, dtype=np.float64), (n,))]))
        self._n_sum_cols = n
        L.check(begin(self._h, n, _ptr(r)))

    def _sums_rows_end(self, end, n_sums):
        """(rows, n_sums) sums of the last `_sums_rows_begin`, collected with the C call `end`."""
        out = np.zeros((self._n_sum_cols, n_sums), dtype=np.float64)
        L.check(end(self._h, _ptr(out)))
        return out

    def sums_groups_begin(self, groups, one_plus_lambda):
        self._sums_rows_begin(L.lib.viprs_state_sums_groups_begin, groups, one_plus_lambda=one_plus_lambda)

    def sums_groups_end(self):
        return self._sums_rows_end(L.lib.viprs_state_sums_groups_end, L.N_SUMS)

    def prep_mixture_groups(self, params):
        """`prep_mixture` with per-group parameters: rows (group, log_null_pi, sigma_epsilon, one_plus_lambda, logit_pi[K],
        log_tau_beta[K], tau_beta[K])."""
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 4 + 3 * self.width)
        L.check(L.lib.viprs_state_prep_mixture_groups(self._h, int(p.shape[0]), _ptr(p)))

    def sums_mixture_groups_begin(self, groups, one_plus_lambda):
        self._sums_rows_begin(L.lib.viprs_state_sums_mixture_groups_begin, groups, one_plus_lambda=one_plus_lambda)

    def sums_mixture_groups_end(self):
        """(n, 7 + 6 K) rows in the layout of `sums_mixture_end`."""
        return self._sums_rows_end(L.lib.viprs_state_sums_mixture_groups_end, 7 + 6 * self.width)

    # -- SNP groups of a grid state: one set of hyper-parameters per (group, column) pair ------------
    def prep_grid_groups(self, params):
        """`prep_columns` per (group, column) pair: rows (group, column, logit_pi, log_tau_beta, sigma_epsilon, tau_beta,
        one_plus_lambda); only the listed pairs' SNPs x column are rewritten."""
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 7)
        L.check(L.lib.viprs_state_prep_grid_groups(self._h, int(p.shape[0]), _ptr(p)))

    def sums_grid_groups_begin(self, groups, cols, one_plus_lambda):
        """The sums of the (groups[i], cols[i]) pairs, one launch (asynchronous); `sums_grid_groups_end` collects them."""
        self._sums_rows_begin(L.lib.viprs_state_sums_grid_groups_begin, groups, cols, one_plus_lambda=one_plus_lambda)

    def sums_grid_groups_end(self):
        """(n, 11) rows in the layout of `sums_columns_end`, [0] the plain sum of gamma over the group."""
        return self._sums_rows_end(L.lib.viprs_state_sums_grid_groups_end, L.N_SUMS)

    def set_group_columns(self, active):
        """(n_groups, width) boolean mask of the (group, column) pairs the following sweeps update (None clears it):
        column g of group c is swept only if g is in `active_model_idx` and active[c, g] is set."""
        if active is None:
            L.check(L.lib.viprs_state_set_group_columns(self._h, 0, 0, None))
            return
        a = np.ascontiguousarray(active, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError(f"active: expected an (n_groups, width) mask, got shape {a.shape}")
        L.check(L.lib.viprs_state_set_group_columns(self._h, int(a.shape[0]), int(a.shape[1]), _ptr(a)))

    def commit_groups(self, src, groups, columns):
        """Grid state as a result store: SNP group groups[i] of the spike-and-slab state `src` (same plan, same dtype, groups
        set) is copied into column columns[i] of var_gamma / var_mu / eta / q / eta_diff -- one launch on the plan's stream,
        no synchronisation."""
        pairs = np.ascontiguousarray(np.column_stack([np.asarray(groups, dtype=np.int32).ravel(),
                                                      np.asarray(columns, dtype=np.int32).ravel()]), dtype=np.int32)
        L.check(L.lib.viprs_state_commit_groups(self._h, src._h, int(pairs.shape[0]), _ptr(pairs)))

    # -- one model (column) of a grid state -----------------------------------------------------
    def prep_column(self, g, logit_pi, log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda):
        L.check(L.lib.viprs_state_prep_column(self._h, int(g), float(logit_pi), float(log_tau_beta),
                                              float(sigma_epsilon), float(tau_beta), float(one_plus_lambda)))

    def sums_column(self, g, one_plus_lambda):
        out = (ctypes.c_double * L.N_SUMS)()
        L.check(L.lib.viprs_state_sums_column(self._h, int(g), float(one_plus_lambda), out))
        return np.array(out[:], dtype=np.float64)

    # -- device-resident EM iteration of a mixture state (K <= 8) --------------------------------------
    def set_log_var_tau(self, log_var_tau):
        a = np.ascontiguousarray(log_var_tau, dtype=np.float64)
        if a.shape != (self.plan.m, self.width):
            raise ValueError(f"log_var_tau: expected shape ({self.plan.m}, {self.width}), got {a.shape}")
        L.check(L.lib.viprs_state_set_log_var_tau(self._h, _ptr(a)))

    def prep_mixture(self, logit_pi, log_tau_beta, tau_beta, log_null_pi, sigma_epsilon, one_plus_lambda):
        v = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (self.width,))) for x in
             (logit_pi, log_tau_beta, tau_beta)]
        L.check(L.lib.viprs_state_prep_mixture(self._h, _ptr(v[0]), _ptr(v[1]), _ptr(v[2]), float(log_null_pi),
                                               float(sigma_epsilon), float(one_plus_lambda)))

    def sums_mixture_begin(self, one_plus_lambda):
        L.check(L.lib.viprs_state_sums_mixture_begin(self._h, float(one_plus_lambda)))

    def sums_mixture_end(self):
        out = np.zeros(7 + 6 * self.width, dtype=np.float64)
        L.check(L.lib.viprs_state_sums_mixture_end(self._h, _ptr(out)))
        return out

    def prep_columns(self, params):
        """`prep_column` for several models in one launch: rows (column, logit_pi, log_tau_beta,
        sigma_epsilon, tau_beta, one_plus_lambda)."""
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 6)
        L.check(L.lib.viprs_state_prep_columns(self._h, int(p.shape[0]), _ptr(p)))

    def sums_columns_begin(self, cols, one_plus_lambda):
        self._sums_rows_begin(L.lib.viprs_state_sums_columns_begin, cols, one_plus_lambda=one_plus_lambda)

    def sums_columns_end(self):
        return self._sums_rows_end(L.lib.viprs_state_sums_columns_end, L.N_SUMS)

    def reset_column(self, g, pi):
        L.check(L.lib.viprs_state_reset_column(self._h, int(g), float(pi)))

    def e_step(self, dq_scale=1.0, active_model_idx=None, sync=True):
        if active_model_idx is not None:
            active = np.ascontiguousarray(active_model_idx, dtype=np.int32)
            L.check(L.lib.viprs_state_e_step(self._h, float(dq_scale), _ptr(active), int(active.shape[0]),
                                             int(bool(sync))))
        else:
            L.check(L.lib.viprs_state_e_step(self._h, float(dq_scale), None, 0, int(bool(sync))))

    # -- elastic net (lassosum): coordinate descent on the sweep of the E-step ------------------------
    def enet_sweep(self, dq_scale=1.0, active_model_idx=None, sync=True):
        """One elastic-net sweep (`viprs_state_enet_sweep`, include/viprs_hip.h; `viprs_amd.stats.enet`) of a float32
        spike-and-slab or grid state: ``mu_mult`` holds ``1 - s``, ``sqrt_half_var_tau`` / ``half_var_tau`` the penalty."""
        active, n = None, 0
        if active_model_idx is not None:
            active = np.ascontiguousarray(active_model_idx, dtype=np.int32)
            n = int(active.shape[0])
        L.check(L.lib.viprs_state_enet_sweep(self._h, float(dq_scale), None if active is None else _ptr(active), n,
                                             int(bool(sync))))

    def enet_sums(self, cols=None):
        """``(n, 6)`` float64, one row per listed column (default: every column): max |eta_diff|, sum std_beta eta,
        sum q eta, sum eta^2, sum pen |eta|, the number of eta != 0 (`viprs_state_enet_sums`)."""
        c = None if cols is None else np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32)
        n = self.width if c is None else int(c.shape[0])
        if self.model != "grid":
            n = 1 if c is None else n
        out = np.zeros((n, L.N_ENET_SUMS), dtype=np.float64)
        L.check(L.lib.viprs_state_enet_sums(self._h, n, None if c is None else _ptr(c), _ptr(out)))
        return out

    # -- LDpred2: a Gibbs draw where the E-step takes an expectation ------------------------------------
    _GIBBS = {"unif": (L.GIBBS_UNIF, np.float32), "noise": (L.GIBBS_NOISE, np.float32), "mean_sum": (L.GIBBS_MEAN_SUM, np.float64)}

    @staticmethod
    def _active(active_model_idx):
        if active_model_idx is None:
            return None, 0
        a = np.ascontiguousarray(active_model_idx, dtype=np.int32)
        return a, int(a.shape[0])

    def gibbs_draws(self, seed, draw_index, active_model_idx=None):
        """The draws of the listed columns (default: every column) of a float32 grid state (`viprs_state_gibbs_draws`,
        include/viprs_hip.h; `viprs_amd.stats.gibbs.gibbs_draws_host`): a function of (seed, draw_index, SNP, column)."""
        a, n = self._active(active_model_idx)
        L.check(L.lib.viprs_state_gibbs_draws(self._h, int(seed), int(draw_index), None if a is None else _ptr(a), n))

    def gibbs_sweep(self, dq_scale=1.0, active_model_idx=None, seed=0, draw_index=0, keep_draws=False, sync=True):
        """One LDpred2 Gibbs sweep (`viprs_state_gibbs_sweep`; `viprs_amd.stats.gibbs`) of a float32 grid state prepared by
        `prep_columns` with sigma_epsilon = 1, lambda = 0, tau_beta = m p / h2: fresh draws for the listed columns, or --
        `keep_draws` -- whatever the two buffers hold."""
        a, n = self._active(active_model_idx)
        L.check(L.lib.viprs_state_gibbs_sweep(self._h, float(dq_scale), None if a is None else _ptr(a), n, int(seed),
                                              int(draw_index), L.GIBBS_KEEP_DRAWS if keep_draws else 0, int(bool(sync))))

    def gibbs_accumulate(self, active_model_idx=None):
        """``mean_sum += float64(var_gamma) * float64(var_mu)`` for the listed columns (`viprs_state_gibbs_accumulate`)."""
        a, n = self._active(active_model_idx)
        L.check(L.lib.viprs_state_gibbs_accumulate(self._h, None if a is None else _ptr(a), n))

    def gibbs_reset_mean(self):
        L.check(L.lib.viprs_state_gibbs_reset_mean(self._h))

    def gibbs_download(self, which):
        """``"unif"`` / ``"noise"`` (float32) or ``"mean_sum"`` (float64), ``(m, G)`` column-major."""
        code, dt = self._GIBBS[which]
        out = np.zeros((self.plan.m, self.width), dtype=dt, order="F")
        L.check(L.lib.viprs_state_gibbs_download(self._h, code, _ptr(out)))
        return out

    def gibbs_upload(self, which, array):
        code, dt = self._GIBBS[which]
        a = np.asarray(array)
        if a.dtype != dt or a.shape != (self.plan.m, self.width) or not a.flags.f_contiguous:
            raise ValueError(f"{which}: a Fortran-contiguous {np.dtype(dt).name} array of shape {(self.plan.m, self.width)}")
        L.check(L.lib.viprs_state_gibbs_upload(self._h, code, _ptr(a)))

    # -- PRS-CS: the local scales psi between two Gibbs sweeps --------------------------------------------
    _CS = {"psi": L.CS_PSI, "delta": L.CS_DELTA, "ub": L.CS_UB, "z1": L.CS_Z1, "z2": L.CS_Z2, "e": L.CS_E}

    def cs_variates(self, seed, draw_index, active_model_idx=None):
        """The variates ``ub, z1, z2, e`` of the listed columns (default: every column) of a float32 grid state
        (`viprs_state_cs_variates`, include/viprs_hip.h; `viprs_amd.stats.cs.cs_variates_host`)."""
        a, n = self._active(active_model_idx)
        L.check(L.lib.viprs_state_cs_variates(self._h, int(seed), int(draw_index), None if a is None else _ptr(a), n))

    def cs_update(self, params, psi_max=1.0, seed=0, draw_index=0, keep_variates=False, prepare_only=False, sync=True):
        """New local scales ``psi`` (and ``delta``) for the chains of `params` -- rows ``(column, sigma2, phi)`` -- and the
        inputs ``mu_mult``, ``half_var_tau``, ``u_logs`` of the next `gibbs_sweep` (`viprs_state_cs_update`;
        `viprs_amd.stats.cs.cs_update_host`).  `prepare_only`: the inputs from the stored psi, nothing drawn."""
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 3)
        flags = (L.CS_KEEP_VARIATES if keep_variates else 0) | (L.CS_PREPARE_ONLY if prepare_only else 0)
        L.check(L.lib.viprs_state_cs_update(self._h, int(p.shape[0]), _ptr(p), float(psi_max), int(seed), int(draw_index), flags,
                                            int(bool(sync))))

    def cs_sums(self, cols=None):
        """``(n, 4)`` float64, one row per listed column (default: every column): sum eta^2 / psi, sum n_j eta^2 / psi,
        sum delta, sum psi (`viprs_state_cs_sums`)."""
        c = None if cols is None else np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32)
        n = self.width if c is None else int(c.shape[0])
        out = np.zeros((n, L.N_CS_SUMS), dtype=np.float64)
        L.check(L.lib.viprs_state_cs_sums(self._h, n, None if c is None else _ptr(c), _ptr(out)))
        return out

    def cs_download(self, which):
        """``"psi"``, ``"delta"``, ``"ub"``, ``"z1"``, ``"z2"`` or ``"e"``: float32 ``(m, G)`` column-major."""
        out = np.zeros((self.plan.m, self.width), dtype=np.float32, order="F")
        L.check(L.lib.viprs_state_cs_download(self._h, self._CS[which], _ptr(out)))
        return out

    def cs_upload(self, which, array):
        a = np.asarray(array)
        if a.dtype != np.float32 or a.shape != (self.plan.m, self.width) or not a.flags.f_contiguous:
            raise ValueError(f"{which}: a Fortran-contiguous float32 array of shape {(self.plan.m, self.width)}")
        L.check(L.lib.viprs_state_cs_upload(self._h, self._CS[which], _ptr(a)))

    # -- SBayesR: a mixture Gibbs draw where the mixture E-step takes an expectation -------------------------
    _BAYESR = {"unif": (L.BAYESR_UNIF, np.float32), "z": (L.BAYESR_Z, np.float32), "kstar": (L.BAYESR_KSTAR, np.int32),
               "mean_sum": (L.BAYESR_MEAN_SUM, np.float64), "pip_sum": (L.BAYESR_PIP_SUM, np.float64)}

    def bayesr_draws(self, seed, draw_index):
        """``U`` and ``z`` of every SNP of a float32 mixture state (`viprs_state_bayesr_draws`, include/viprs_hip.h;
        `viprs_amd.stats.bayesr.bayesr_draws_host`): a function of (seed, draw_index, SNP)."""
        L.check(L.lib.viprs_state_bayesr_draws(self._h, int(seed), int(draw_index)))

    def bayesr_sweep(self, dq_scale=1.0, seed=0, draw_index=0, keep_draws=False, sync=True):
        """One SBayesR sweep (`viprs_state_bayesr_sweep`; `viprs_amd.stats.bayesr`) of a float32 mixture state of K <= 4
        components prepared by `prep_mixture` with lambda = 0: fresh draws, or -- `keep_draws` -- whatever the buffers hold."""
        L.check(L.lib.viprs_state_bayesr_sweep(self._h, float(dq_scale), int(seed), int(draw_index),
                                               L.BAYESR_KEEP_DRAWS if keep_draws else 0, int(bool(sync))))

    def bayesr_sums(self):
        """``2 K + 4`` float64: the number of SNPs with k* = 0 .. K, sum eta^2 over k* = k for k = 1 .. K, sum q eta,
        sum eta^2, sum std_beta eta (`viprs_state_bayesr_sums`)."""
        out = np.zeros(2 * self.width + 4, dtype=np.float64)
        L.check(L.lib.viprs_state_bayesr_sums(self._h, _ptr(out)))
        return out

    def bayesr_accumulate(self):
        """``mean_sum += sum_k gamma_k mu_k`` and ``pip_sum += sum_k gamma_k`` (`viprs_state_bayesr_accumulate`)."""
        L.check(L.lib.viprs_state_bayesr_accumulate(self._h))

    def bayesr_reset_mean(self):
        L.check(L.lib.viprs_state_bayesr_reset_mean(self._h))

    def bayesr_download(self, which):
        """``"unif"`` / ``"z"`` (float32), ``"kstar"`` (int32), ``"mean_sum"`` / ``"pip_sum"`` (float64): ``(m,)``."""
        code, dt = self._BAYESR[which]
        out = np.zeros(self.plan.m, dtype=dt)
        L.check(L.lib.viprs_state_bayesr_download(self._h, code, _ptr(out)))
        return out

    def bayesr_upload(self, which, array):
        code, dt = self._BAYESR[which]
        a = np.asarray(array)
        if a.dtype != dt or a.shape != (self.plan.m,) or not a.flags.c_contiguous:
            raise ValueError(f"{which}: a contiguous {np.dtype(dt).name} array of shape {(self.plan.m,)}")
        L.check(L.lib.viprs_state_bayesr_upload(self._h, code, _ptr(a)))

    def dot(self, name="eta", dq_scale=1.0, include_diagonal=True):
        """``R @ eta`` with the resident posterior mean as `B` (`viprs_state_dot`): only the ``m x n_cols`` results cross to
        the host.  ``(m,)`` for spike-and-slab and mixture states, ``(m, G)`` column-major for grid states.  Any field other
        than ``"eta"`` is refused by the library (ValueError)."""
        if name not in self.FIELDS:
            raise ValueError(f"unknown field {name!r}")
        shape = self._shape("eta")
        y = np.empty(shape, dtype=self.dtype, order="F" if len(shape) == 2 else "C")
        L.check(L.lib.viprs_state_dot(self._h, self.FIELDS[name], float(dq_scale), int(bool(include_diagonal)), _ptr(y)))
        return y

    def synchronize(self):
        L.check(L.lib.viprs_state_synchronize(self._h))


class DeviceCoupling:
    """The PRS-CSx coupling of P float32 grid `DeviceState`s of one width through one local scale per SNP of the union of
    their SNP sets (`viprs_csx_*`, include/viprs_hip.h; `viprs_amd.stats.csx` is the host definition).  `row_of`: ``(P,
    m_union)`` int64, the row of every union SNP in each state's plan or -1.  The states stay the caller's; the coupling
    keeps them alive."""

    _BUF = {"psi": (L.CSX_PSI, np.float32), "delta": (L.CSX_DELTA, np.float32), "attempts": (L.CSX_ATTEMPTS, np.uint8)}

    def __init__(self, states, row_of):
        self.states = list(states)
        r = np.ascontiguousarray(row_of, dtype=np.int64)
        if r.ndim != 2 or r.shape[0] != len(self.states):
            raise ValueError("row_of: an int64 array of shape (len(states), m_union)")
        self.n_pop, self.m_union = int(r.shape[0]), int(r.shape[1])
        self.width = int(self.states[0].width) if self.states else 0
        hs = (ctypes.c_void_p * max(self.n_pop, 1))(*[s._h for s in self.states])
        self._h = ctypes.c_void_p()
        L.check(L.lib.viprs_csx_create(ctypes.byref(self._h), self.n_pop, hs, self.m_union, _ptr(r)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib.viprs_csx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, params, psi_max=1.0, seed=0, draw_index=0, keep_variates=False, prepare_only=False, sync=True):
        """One coupled update for the chains of `params` -- rows ``(column, phi, sigma2_0 .. sigma2_{P-1})``: new shared
        ``psi`` and ``delta``, scattered with ``mu_mult``, ``half_var_tau``, ``u_logs`` into every state (`viprs_csx_update`)."""
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 2 + self.n_pop)
        flags = (L.CS_KEEP_VARIATES if keep_variates else 0) | (L.CS_PREPARE_ONLY if prepare_only else 0)
        L.check(L.lib.viprs_csx_update(self._h, int(p.shape[0]), _ptr(p), float(psi_max), int(seed), int(draw_index), flags,
                                       int(bool(sync))))

    def sums(self, cols=None):
        """``(n, 2)`` float64, one row per listed column (default: every column): sum delta, sum psi over the union."""
        c = None if cols is None else np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32)
        n = self.width if c is None else int(c.shape[0])
        out = np.zeros((n, L.N_CSX_SUMS), dtype=np.float64)
        L.check(L.lib.viprs_csx_sums(self._h, n, None if c is None else _ptr(c), _ptr(out)))
        return out

    def download(self, which):
        """``"psi"``, ``"delta"`` (float32) or ``"attempts"`` (uint8): ``(m_union, G)`` column-major."""
        code, dt = self._BUF[which]
        out = np.zeros((self.m_union, self.width), dtype=dt, order="F")
        L.check(L.lib.viprs_csx_download(self._h, code, _ptr(out)))
        return out

    def upload(self, which, array):
        code, dt = self._BUF[which]
        a = np.asarray(array)
        if a.dtype != dt or a.shape != (self.m_union, self.width) or not a.flags.f_contiguous:
            raise ValueError(f"{which}: a Fortran-contiguous {np.dtype(dt).name} array of shape {(self.m_union, self.width)}")
        L.check(L.lib.viprs_csx_upload(self._h, code, _ptr(a)))

    def last(self):
        """``(ms, n_capped)`` of the last update: its event time and the draws that ended at the attempt cap."""
        ms, nc = ctypes.c_double(0.0), ctypes.c_int64(0)
        L.check(L.lib.viprs_csx_last(self._h, ctypes.byref(ms), ctypes.byref(nc)))
        return ms.value, int(nc.value)
