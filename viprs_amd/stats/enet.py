"""The elastic-net (lassosum) sweep on the host: the definition `viprs_state_enet_sweep` is pinned to, and the CPU fallback.

lassosum (Mak et al. 2017) minimises ``b'((1 - s) R + s I) b - 2 b'beta_hat + 2 sum_j pen_j |b_j|`` by cyclic coordinate
descent over each LD block with a running ``q = (R - I) b``.  One sweep, per SNP j in index order, every operation
separately rounded in float32 (include/viprs_hip.h states it with the device call):

    t = c_j q_j;  u = beta_hat_j - t;  a = |u| - pen_j;  b = a > 0 ? copysign(a, u) : +0;  d = b - eta_j
    var_mu[j] = u;  var_gamma[j] = (b != 0);  eta_diff[j] = d;  eta[j] += d
    q[k] = fma(R[j, k], dq_scale d, q[k]) over the row's window in index order   (symmetric form: then q[j] -= d)

and, upper form, after the last SNP ``q[j] += dq_scale dot(row(j), eta_diff)`` with the dot a serial fma chain from 0.

The float32 fused multiply-add is formed exactly in NumPy: the product of two float32 values is exact in float64, the sum
is rounded TO ODD in float64 (the error term of the addition says whether it was exact and on which side the true value
lies) and a value rounded to odd in 53 bits rounds to the nearest float32 as the exact value does (Boldo & Melquiond 2008:
53 >= 2 * 24 + 2).  A plain float64 emulation rounds twice and is off by one ulp now and then;
tests/test_enet_reference.py compares this one `==` with libm's `fmaf`.
"""
import numpy as np

N_ENET_SUMS = 6
_F32, _F64 = np.float32, np.float64


def fma32(a, b, c):
    """``fl32(a * b + c)`` with ONE rounding, elementwise, for float32 arrays (or scalars) of finite values; a non-finite
    operand gives what the float64 expression gives (inf / nan as `fmaf` does)."""
    p = np.asarray(a, dtype=_F32).astype(_F64) * np.asarray(b, dtype=_F32).astype(_F64)     # exact: 48 bits
    c = np.asarray(c, dtype=_F32).astype(_F64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                     # TwoSum: p + c = s + err exactly
        bits = np.array(s, dtype=_F64, ndmin=1).view(np.int64)
        inexact_even = np.isfinite(s) & (err != 0.0) & ((bits & 1) == 0)
        # the neighbour of s on the side of the true value: its last mantissa bit is odd
        step = np.where((np.atleast_1d(err) > 0.0) == (np.atleast_1d(s) > 0.0), 1, -1)
        odd = np.where(np.atleast_1d(inexact_even), bits + step, bits).view(_F64).reshape(np.shape(s))
        return odd.astype(_F32)


def _as_columns(a, m, name):
    a = np.asarray(a)
    if a.dtype != _F32 or a.shape[0] != m or a.ndim not in (1, 2):
        raise ValueError(f"{name}: a float32 array of shape (m,) or (m, G)")
    return a.reshape(m, -1)


def _sweep_column(lb, ip, x, low_memory, beta, c, pen, eta, q, dq):
    m = lb.shape[0]
    ed, mu, gam = np.zeros(m, dtype=_F32), np.zeros(m, dtype=_F32), np.zeros(m, dtype=_F32)
    zero = _F32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            t = c[j] * q[j]
            u = beta[j] - t
            a = np.abs(u) - pen[j]
            b = np.copysign(a, u) if a > zero else zero
            d = b - eta[j]
            mu[j], gam[j], ed[j] = u, (1.0 if b != zero else 0.0), d
            s, e = ip[j], ip[j + 1]
            if e > s:
                k = lb[j]
                q[k:k + e - s] = fma32(x[s:e], dq * d, q[k:k + e - s])
            if not low_memory:
                q[j] = q[j] - d
            eta[j] = eta[j] + d
        if low_memory:
            # update_q_factor: every row's dot is a serial chain from 0 in index order; the chains advance side by side
            length = (ip[1:] - ip[:-1]).astype(np.int64)
            acc = np.zeros(m, dtype=_F32)
            rows = np.flatnonzero(length > 0)
            i = 0
            while rows.shape[0]:
                acc[rows] = fma32(x[ip[rows] + i], ed[lb[rows] + i], acc[rows])
                i += 1
                rows = rows[length[rows] > i]
            q += dq * acc
    return ed, mu, gam


def enet_sweep_host(lb, ip, data, low_memory, std_beta, mult, penalty, eta, q, dq_scale=1.0):
    """One elastic-net sweep (module docstring) over LD in the layout of `LDPlan`; `mult`, `penalty`, `eta`, `q` are float32
    arrays ``(m,)`` or ``(m, G)`` (one column per model: the columns are independent).  `eta` and `q` are updated IN PLACE;
    returns ``(eta_diff, var_mu, var_gamma)`` in their shape."""
    lb = np.asarray(lb, dtype=np.int64)
    ip = np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    x = np.asarray(data).astype(_F32)                       # (T)ld[i]: exact for int8 / int16 / fp32 LD
    beta = np.asarray(std_beta)
    if beta.dtype != _F32 or beta.shape != (m,):
        raise ValueError("std_beta: a float32 array of shape (m,)")
    if not (isinstance(eta, np.ndarray) and isinstance(q, np.ndarray) and eta.shape == q.shape):
        raise ValueError("eta, q: float32 arrays of one shape, updated in place")
    shape = eta.shape
    C, Pn, E, Q = (_as_columns(a, m, n) for a, n in ((mult, "mult"), (penalty, "penalty"), (eta, "eta"), (q, "q")))
    if not (C.shape == Pn.shape == E.shape):
        raise ValueError("mult, penalty, eta and q must have one shape")
    if not (np.shares_memory(E, eta) and np.shares_memory(Q, q)):
        raise ValueError("eta, q: contiguous per column (C order for (m,), Fortran order for (m, G))")
    dq = _F32(dq_scale)
    outs = [np.zeros(E.shape, dtype=_F32, order="F") for _ in range(3)]
    for g in range(E.shape[1]):
        ej, qj = np.array(E[:, g]), np.array(Q[:, g])
        res = _sweep_column(lb, ip, x, bool(low_memory), beta, C[:, g], Pn[:, g], ej, qj, dq)
        E[:, g], Q[:, g] = ej, qj
        for o, r in zip(outs, res):
            o[:, g] = r
    return tuple(o.reshape(shape) if len(shape) == 1 else o for o in outs)


# ---- the sums ---------------------------------------------------------------------------------------------------------------
def _ordered(terms, cap, is_max):
    """One sum (or fmax) in THE ORDER of include/viprs_hip.h: nb = min(ceil(len / 256), cap) workgroups of 256 threads,
    thread t of workgroup b takes terms b * 256 + t, + nb * 256, ... serially; a binary tree over the 256 accumulators; lane l
    of 64 adds partials l, l + 64, ... serially; an xor butterfly over the lanes."""
    n = terms.shape[0]
    if n == 0:
        return 0.0
    op = np.fmax if is_max else np.add
    nb = min(-(-n // 256), cap)
    passes = -(-n // (nb * 256))
    t = np.zeros(passes * nb * 256, dtype=_F64)
    t[:n] = terms
    t = t.reshape(passes, nb, 256)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((nb, 256), dtype=_F64)
        for k in range(passes):
            acc = op(acc, t[k])
        s = 128
        while s > 0:
            acc[:, :s] = op(acc[:, :s], acc[:, s:2 * s])
            s //= 2
        part = np.zeros(-(-nb // 64) * 64, dtype=_F64)
        part[:nb] = acc[:, 0]
        part = part.reshape(-1, 64)
        a = np.zeros(64, dtype=_F64)
        for k in range(part.shape[0]):
            a = op(a, part[k])
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            a = op(a, a[lane ^ off])
    return float(a[0])


def enet_sums_host(std_beta, penalty, eta, q, eta_diff, cols=None, grid=None):
    """`viprs_state_enet_sums` on the host: ``(n, 6)`` float64 -- max |eta_diff|, sum std_beta eta, sum q eta, sum eta^2,
    sum pen |eta|, the number of eta != 0 -- per listed column, every term formed in float64 from the float32 values and
    summed in the order of the device reduction.  `grid`: the arrays are those of a grid state (256 workgroups at most per
    row instead of 1024); default: they are two-dimensional."""
    eta = np.asarray(eta)
    m = eta.shape[0]
    grid = (eta.ndim == 2) if grid is None else bool(grid)
    cap = 256 if grid else 1024
    G = 1 if eta.ndim == 1 else eta.shape[1]
    E, Q, D, Pn = (np.asarray(a, dtype=_F32).reshape(m, G).astype(_F64) for a in (eta, q, eta_diff, penalty))
    b = np.asarray(std_beta, dtype=_F32).astype(_F64)
    cols = range(E.shape[1]) if cols is None else [int(c) for c in np.atleast_1d(cols)]
    out = np.zeros((len(cols), N_ENET_SUMS), dtype=_F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, g in enumerate(cols):
            e = E[:, g]
            out[i] = (_ordered(np.abs(D[:, g]), cap, True), _ordered(b * e, cap, False), _ordered(Q[:, g] * e, cap, False),
                      _ordered(e * e, cap, False), _ordered(Pn[:, g] * np.abs(e), cap, False),
                      _ordered((e != 0.0).astype(_F64), cap, False))
    return out


def lambda_path(lo=0.001, hi=0.1, n=20):
    """`n` penalties from `hi` down to `lo`, log-spaced (lassosum's default path)."""
    if not (0.0 < lo <= hi) or n < 1:
        raise ValueError("lambda_path: 0 < lo <= hi and n >= 1")
    return np.exp(np.linspace(np.log(hi), np.log(lo), int(n)))


def enet_objective(sums, s):
    """``b'((1 - s) R + s I) b - 2 b'beta_hat + 2 sum pen |b|`` from rows of `enet_sums` (with ``q = (R - I) b``:
    ``b'Rb = sum q eta + sum eta^2``)."""
    sums = np.asarray(sums, dtype=_F64)
    s = np.asarray(s, dtype=_F64)
    return (1.0 - s) * (sums[..., 2] + sums[..., 3]) + s * sums[..., 3] - 2.0 * sums[..., 1] + 2.0 * sums[..., 4]
