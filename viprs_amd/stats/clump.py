"""Greedy LD clumping on the device: the primitive of clumping + thresholding (C+T / P+T) and of LD pruning.

Walk the SNPs from the most significant down; every SNP that nobody has claimed yet becomes an INDEX SNP and claims the
SNPs in LD with it at ``r^2 >= r2`` that are still unclaimed.  The definition is stated in full in include/viprs_hip.h
(`viprs_plan_clump`) and restated by `clump_host`:

* the entries of row j are the off-diagonal entries of the symmetric matrix the arrays stand for -- a stored zero is an
  entry, the gaps of a window and the diagonal are not; in the upper form the transposed entries of the rows above j that
  reach it belong to row j;
* an entry with stored element x passes iff ``float64(x) * float64(x) >= r2 / (dq_scale * dq_scale)``;
* ``index_of[k]`` is the index SNP that claimed k (k itself for an index SNP), -1 for a SNP nobody claimed.

* ``clump_host``   plain NumPy, written from the definition: the CPU fallback and the yardstick of the tests;
* ``clump_order``  the processing order of a chi^2 vector;
* ``clump``        the clumps of one LD matrix or of every chromosome of a data loader (`LDPlan.clump`).
"""
import numpy as np

from .spectrum import _ld_matrices


def _thresholds(r2, dq_scale):
    """``(thresholds on the squared stored element, r2 was a scalar)``: two double operations, as the library's host side."""
    thr = np.atleast_1d(np.asarray(r2, dtype=np.float64))
    if thr.ndim != 1 or not 1 <= thr.shape[0] <= 32:
        raise ValueError("r2: a scalar or 1..32 thresholds")
    if not np.all(np.isfinite(thr)) or np.any(thr < 0.0):
        raise ValueError("r2 thresholds must be finite and >= 0")
    dq = float(dq_scale)
    if not np.isfinite(dq) or not dq > 0.0:
        raise ValueError("dq_scale must be finite and > 0")
    return thr / (dq * dq), np.ndim(r2) == 0


def _check_order(order, member, m):
    order = np.asarray(order)
    if order.ndim != 1 or (order.size and not np.issubdtype(order.dtype, np.integer)):
        raise ValueError("order: a 1-d array of SNP indices")
    order = order.astype(np.int64)
    if order.size and (order.min() < 0 or order.max() >= m):
        raise ValueError(f"order: SNP indices must be in [0, {m})")
    if np.unique(order).shape[0] != order.shape[0]:
        raise ValueError("order: a SNP index is repeated")
    member = np.ones(m, dtype=bool) if member is None else np.asarray(member) != 0
    if member.shape != (m,):
        raise ValueError(f"member: expected shape ({m},), got {member.shape}")
    if not np.all(member[order]):
        raise ValueError("order: every SNP of the order must be a member")
    return order, member


def clump_host(lb, ip, data, low_memory, order, r2, member=None, dq_scale=1.0):
    """``index_of`` of the matrix the arrays stand for (the layout of `LDPlan`): int32 ``(m,)`` for a scalar `r2`, ``(m, G)``
    for a sequence, every column clumped on its own.  `order`: distinct SNP indices, most significant first; `member`:
    ``(m,)`` booleans, the SNPs that may belong to a clump (None: all)."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    thr, scalar = _thresholds(r2, dq_scale)
    order, member = _check_order(order, member, m)
    x = np.asarray(data).astype(np.float64)
    p = x * x
    first = None
    if low_memory:
        # the lowest row whose stored entries reach column j: the rows above j that hold a transposed entry of row j
        reach = np.arange(m) + np.diff(ip)
        first = np.searchsorted(np.maximum.accumulate(reach), np.arange(m), side="left")
    out = np.full((m, thr.shape[0]), -1, dtype=np.int32)
    for g, t in enumerate(thr):
        avail = member.copy()
        index_of = out[:, g]
        for j in order:
            j = int(j)
            if not avail[j]:
                continue
            index_of[j] = j
            avail[j] = False
            s, e = int(ip[j]), int(ip[j + 1])
            cols = int(lb[j]) + np.arange(e - s)
            ok = p[s:e] >= t
            if not low_memory:
                ok &= cols != j                              # symmetric form: the stored diagonal entry is no entry
            k = cols[ok]
            if low_memory and first[j] < j:
                i = np.arange(int(first[j]), j)
                i = i[reach[i] >= j]
                k = np.concatenate([i[p[ip[i] + (j - i - 1)] >= t], k])
            k = k[avail[k]]
            index_of[k] = j
            avail[k] = False
    return out[:, 0] if scalar else out


def clump_order(chisq, min_chisq=0.0):
    """The processing order of a clumping: the SNPs with ``chisq >= min_chisq`` by descending chi^2, ties by ascending index
    (a stable sort); NaN is excluded."""
    chisq = np.asarray(chisq, dtype=np.float64)
    keep = np.flatnonzero(chisq >= float(min_chisq))        # (NaN compares false)
    return keep[np.argsort(-chisq[keep], kind="stable")].astype(np.int32)


def chisq_cutoff(p):
    """The chi^2 (1 degree of freedom) a p-value threshold stands for; p >= 1 keeps every SNP."""
    if float(p) >= 1.0:
        return 0.0
    from scipy.stats import chi2
    return float(chi2.isf(float(p), 1))


def clump(ld_mat_or_gdl, chisq=None, r2=0.1, p1=1.0, p2=1.0, order=None, member=None, low_memory=True,
          dequantize_on_the_fly=False, device=0, float_precision="float32", clump_fn=None):
    """The clumps of one LD matrix object, of a ``{chromosome: LD matrix}`` dict or of every chromosome of a data loader:
    ``{chromosome: index_of}``, int32 ``(m_c,)`` for a scalar `r2` or ``(m_c, G)`` for a sequence (see `clump_host`).

    `chisq`: ``(m_c,)`` chi^2 statistics or a ``{chromosome: array}`` dict; None: the loader's own summary statistics.
    Index SNPs have ``p <= p1``, the SNPs they may claim ``p <= p2`` (PLINK's ``--clump-p1 / --clump-p2``); the p-values
    become chi^2 cut-offs by ``scipy.stats.chi2.isf(p, 1)``.  `order` (an array or a ``{chromosome: array}`` dict) replaces
    the order by chi^2, and `member` the members by `p2`: with ``order=np.arange(m_c)``, the natural order, the operation
    is LD PRUNING -- the SNPs with ``index_of[k] == k`` are a set in which no stored pair reaches `r2`, scanned first to last.

    The LD is loaded as `ld_scores` loads it (`load_chromosome_ld`; a matrix that holds only the upper-triangular store is
    clumped in that form with ``low_memory=False`` too).  On HIP device `device` (`LDPlan.clump`); without a device, or with
    `clump_fn` (a callable with `clump_host`'s signature), on the host."""
    from .. import _lib
    from ..model._ld_loading import dequantize_scale, load_chromosome_ld, open_plan
    from .ldsc import chisq_statistic
    on_host = clump_fn is not None or _lib.device_count() < 1
    clump_fn = clump_fn or clump_host
    pick = lambda v, c: v[c] if isinstance(v, dict) else v
    out = {}
    for c, ld_mat in _ld_matrices(ld_mat_or_gdl).items():
        ld = load_chromosome_ld(ld_mat, low_memory, dequantize_on_the_fly, float_precision).as_stored()
        m = ld.left_bound.shape[0]
        o, mem, x2 = pick(order, c), pick(member, c), pick(chisq, c)
        if x2 is None and (o is None or mem is None) and hasattr(ld_mat_or_gdl, "sumstats_table"):
            x2 = chisq_statistic(ld_mat_or_gdl.sumstats_table[c])
        if o is None:
            if x2 is None:
                raise ValueError(f"chromosome {c}: clump needs `chisq` (or a loader with summary statistics) or an `order`")
            o = clump_order(x2, chisq_cutoff(p1))
        if mem is None and x2 is not None and float(p2) < 1.0:
            mem = np.asarray(x2, dtype=np.float64) >= chisq_cutoff(p2)
            mem[np.asarray(o, dtype=np.int64)] = True          # (an index SNP is a member of its own clump)
        dq = dequantize_scale(ld_mat, ld.dequantize)
        if on_host:
            out[c] = clump_fn(ld.left_bound, ld.indptr, ld.data, ld.form == "upper", o, r2, mem, dq)
            continue
        plan = open_plan(ld, device)
        try:
            out[c] = plan.clump(o, r2, member=mem, dq_scale=dq)
        finally:
            plan.close()
    return out
