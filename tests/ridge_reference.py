"""Host model of the ridge solve (include/viprs_hip.h, `viprs_plan_solve_ridge`): the specification of its recurrences.

    (R + diag(shift)) x = b,  R = unit diagonal + dq_scale * stored off-diagonal entries,

solved independently for every LD block by MINRES (Paige & Saunders 1975; the recurrences are those of
scipy.sparse.linalg.minres with the shift ADDED).  Per block:

    r1 = y = b - A x0, beta1 = sqrt(y.y), bnorm = sqrt(b.b)  (= beta1 without x0)
    every iteration:  v = y / beta;  y = A v;  itn >= 2: y -= (beta / oldb) r1;  alfa = v.y;  y -= (alfa / beta) r2;
                      r1 <- r2 <- y;  oldb <- beta;  beta = sqrt(y.y);
                      oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;
                      dbar = -cs beta;  gamma = max(sqrt(gbar^2 + beta^2), eps);  cs = gbar / gamma;  sn = beta / gamma;
                      phi = cs phibar;  phibar = sn phibar;
                      w = (v - oldeps w1 - delta w2) / gamma;  x += phi w
    stop when phibar <= rtol * bnorm or beta == 0

The stopping rule is relative to ||b||: with a start vector the residual that counts is still ||b - A x|| / ||b||, so a
converged x0 comes back at once (scipy measures against ||b - A x0|| and would iterate on rounding noise).

Vectors are in the state precision T, every vector operation is one rounded operation in T with its scalar coefficient
rounded to T first; scalars and dot products are float64.  A v is fl(fl(dq_scale) S) + v + fl(shift) v with S the
off-diagonal sum.

The two sums the header gives an ORDER for are seams (`minres_block(..., off=, dot=)`, `solve(..., off_product=, dot=)`):
    off(v)     S, the off-diagonal sum of a block, in T.  Default: float64 matrix product, rounded to T once -- a model of
               the recurrences, not of the device's bits
    dot(a, b)  a float64 value.  Default: `np.dot` of the float64 copies
With the replays of tests/order_replay.py in both seams (the product's own order in T, the 256-thread order of the dot
products) the model IS the device's arithmetic, operation by operation: the GPU tests compare it with `==`.

status: 0 converged, 1 stopped at maxiter, 2 zero right-hand side (x = 0, no iteration).
"""
import numpy as np

from viprs_amd.plan import RidgeInfo, plan_blocks

from .ld_dot_reference import block_matrix

_EPS = np.finfo(np.float64).eps


def blocks_of(lb, ip, low_memory):
    starts, _ = plan_blocks(np.ascontiguousarray(lb, dtype=np.int32), np.ascontiguousarray(ip), bool(low_memory))
    return [(int(s), int(e)) for s, e in zip(starts[:-1], starts[1:])]


def shift_vector(shift, m, dtype):
    """The shift the solver applies: per SNP, rounded to the state precision; as float64."""
    sh = np.asarray(shift, dtype=np.float64)
    sh = np.full(m, float(sh)) if sh.ndim == 0 else sh
    return sh.astype(dtype).astype(np.float64)


def block_systems(lb, ip, data, low_memory, shift, dq_scale, dtype):
    """[(start, end, A)]: the dense float64 matrix I + fl(dq_scale) R_off + diag(fl(shift)) of every LD block, rebuilt from the
    stored arrays through the windowed-row reconstruction of ld_dot_reference (dense and windowed blocks, both forms)."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    sh = shift_vector(shift, lb.shape[0], dtype)
    dq = float(np.dtype(dtype).type(dq_scale))
    out = []
    for s, e in blocks_of(lb, ip, low_memory):
        R, _ = block_matrix(lb, ip, np.asarray(data, dtype=np.float64), low_memory, s, e)
        out.append((s, e, np.eye(e - s) + dq * R + np.diag(sh[s:e])))
    return out


def dense_solve(systems, b):
    """x* of every block by np.linalg.solve in float64."""
    x = np.zeros(np.asarray(b).shape[0], dtype=np.float64)
    b64 = np.asarray(b, dtype=np.float64)
    for s, e, A in systems:
        x[s:e] = np.linalg.solve(A, b64[s:e])
    return x


def true_residuals(systems, b, x):
    """||b - A x|| / ||b|| per block, float64 (0 for a zero right-hand side)."""
    b64, x64 = np.asarray(b, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = np.zeros(len(systems))
    for k, (s, e, A) in enumerate(systems):
        nb = np.linalg.norm(b64[s:e])
        out[k] = np.linalg.norm(b64[s:e] - A @ x64[s:e]) / nb if nb > 0 else 0.0
    return out


def condition_numbers(systems):
    out = np.zeros(len(systems))
    for k, (_, _, A) in enumerate(systems):
        ev = np.abs(np.linalg.eigvalsh(A))
        out[k] = ev.max() / ev.min()
    return out


def _default_dot(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


def minres_block(R_off, b, sh, dq, rtol, maxiter, x0=None, off=None, dot=None):
    """One block.  R_off: stored off-diagonal entries (float64, not dequantised; unused with `off`); b, sh, x0 in T; dq a T
    scalar.  `off`, `dot`: the seams of the module docstring."""
    T = b.dtype.type
    if off is None:
        off = lambda v: (R_off @ v.astype(np.float64)).astype(b.dtype)
    _dot = _default_dot if dot is None else dot

    def matvec(v):
        y = dq * off(v)
        y = y + v
        return y + sh * v

    n = b.shape[0]
    bnorm = np.sqrt(_dot(b, b))
    if bnorm == 0.0:
        return np.zeros(n, dtype=b.dtype), 0, 0.0, RidgeInfo.ZERO_RHS
    if x0 is None:
        x = np.zeros(n, dtype=b.dtype)
        y = b.copy()
    else:
        x = x0.astype(b.dtype, copy=True)
        y = b - matvec(x)
    r1 = y.copy()
    r2 = y
    beta1 = np.sqrt(_dot(y, y))
    if beta1 <= rtol * bnorm:
        return x, 0, beta1 / bnorm, RidgeInfo.CONVERGED
    oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, -1.0, 0.0
    w = np.zeros(n, dtype=b.dtype)
    w2 = np.zeros(n, dtype=b.dtype)
    status = RidgeInfo.MAXITER
    itn = 0
    while itn < maxiter:
        itn += 1
        v = y / T(beta)
        y = matvec(v)
        if itn >= 2:
            y = y - T(beta / oldb) * r1
        alfa = _dot(v, y)
        y = y - T(alfa / beta) * r2
        r1, r2 = r2, y
        oldb = beta
        beta = np.sqrt(_dot(y, y))
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = max(np.sqrt(gbar * gbar + beta * beta), _EPS)
        cs = gbar / gamma
        sn = beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        w1, w2 = w2, w
        w = ((v - T(oldeps) * w1) - T(delta) * w2) / T(gamma)
        x = x + T(phi) * w
        if phibar <= rtol * bnorm or beta == 0.0:
            status = RidgeInfo.CONVERGED
            break
    return x, itn, phibar / bnorm, status


def solve(lb, ip, data, low_memory, b, shift, dq_scale=1.0, rtol=None, maxiter=None, x0=None, off_product=None, dot=None):
    """The host model over every block: `(x, RidgeInfo)` -- the signature of `LDPredInf(solve_fn=...)`.  `off_product(s, e)`
    gives the `off` of block [s, e) (None: the float64 matrix product), `dot` is handed to every block."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    b = np.asarray(b)
    dtype = b.dtype
    assert dtype in (np.float32, np.float64)
    m = lb.shape[0]
    if rtol is None:
        rtol = 1e-5 if dtype == np.float32 else 1e-10
    blocks = blocks_of(lb, ip, low_memory)
    if maxiter is None:
        maxiter = 5 * max((e - s for s, e in blocks), default=1)
    sh = shift_vector(shift, m, dtype).astype(dtype)
    dq = dtype.type(dq_scale)
    x = np.zeros(m, dtype=dtype)
    iters, relres, status = [], [], []
    data64 = np.asarray(data, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for s, e in blocks:
            R = block_matrix(lb, ip, data64, low_memory, s, e)[0] if off_product is None else None
            xb, it, rr, st = minres_block(R, b[s:e], sh[s:e], dq, float(rtol), int(maxiter),
                                          None if x0 is None else np.asarray(x0)[s:e],
                                          None if off_product is None else off_product(s, e), dot)
            x[s:e] = xb
            iters.append(it)
            relres.append(rr)
            status.append(st)
    return x, RidgeInfo(iters, relres, status)


def banded_ar1(m, rho, window, low_memory, dtype=np.float32):
    """One windowed component: the AR(1) matrix rho^|i-j| truncated to |i - j| <= window (not positive definite any more),
    in the symmetric form (row j: columns j - window .. j + window, diagonal included) or the upper one (j + 1 .. j + window)."""
    j = np.arange(m)
    lo = j + 1 if low_memory else np.maximum(j - window, 0)
    hi = np.minimum(j + window + 1, m)
    length = np.maximum(hi - lo, 0)
    ip = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    lb = np.where(length > 0, lo, np.minimum(lo, m - 1)).astype(np.int32)
    data = np.concatenate([np.power(rho, np.abs(np.arange(lo[r], hi[r]) - r)) for r in range(m)]).astype(dtype)
    return lb, ip, data
