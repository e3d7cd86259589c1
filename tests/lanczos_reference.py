"""Host model of the extremal-eigenvalue computation (include/viprs_hip.h, `viprs_plan_extremal_eigenvalues`): the
specification of its recurrence, start vector, check schedule and stopping rule.

    A = I + fl(dq_scale) * stored off-diagonal entries,  per LD block

Lanczos without reorthogonalisation, per block, iteration k = 1, 2, ... (beta_1 = 0, v_prev = 0):

    w = A v - fl_T(beta_k) v_prev;  alpha_k = v.w;  w -= fl_T(alpha_k) v;  beta_{k+1} = ||w||;
    v_prev <- v;  v <- fl_T(w / beta_{k+1})

Start vector: a function of the index i inside the block only,

    h = splitmix64 finaliser of (i + 1) * 0x9E3779B97F4A7C15 (mod 2^64),
    u_i = (h >> 40) * 2^-24 - 0.5 + 2^-25   (an odd multiple of 2^-25: exact in float32, never zero),
    v = fl_T(u / ||u||).

At k = 1, 2, 4, 8, ... and at maxiter the extreme Ritz pairs (theta, s) of the tridiagonal T_k are taken; with s_k the last
component of a unit eigenvector, beta_{k+1} |s_k| is the residual norm ||A y - theta y|| of the Ritz vector, hence an upper
bound of the distance from theta to the nearest eigenvalue of A (to O(eps ||A||) in finite precision).  A block stops when
both bounds are <= rtol * max(|theta_min|, |theta_max|), or when beta_{k+1} == 0.  k reaching the block's size is NOT a
reason to stop: in finite precision the Ritz values at k = size are not the eigenvalues.

Vectors are in the state precision T, every vector operation is one rounded operation in T with its scalar coefficient
rounded to T first; scalars and dot products are float64.  A v is fl(fl(dq_scale) S) + v with S the off-diagonal sum.

What the header gives an ORDER or a routine for is a seam (`lanczos_block(..., off=, dot=, ritz=)`,
`extremal_eigenvalues(..., off_product=, dot=, ritz=)`):
    off(v)              S, the off-diagonal sum of a block, in T.  Default: float64 matrix product, rounded to T once
    dot(a, b)           a float64 value (the norm of the start vector included).  Default: `np.dot` of the float64 copies
    ritz(alpha, beta)   the extreme Ritz pairs of T_k.  Default: `np.linalg.eigh` (`ritz_extremes` below); the C library has
                        its own implicit-QL routine (`viprs_tridiagonal_extremes`)
With the defaults this is a model of the recurrence, not of the device's bits.  With the replays of tests/order_replay.py in
the seams (the product's own order in T, the 256-thread order of the dot products, the library's QL routine) it IS the
device's arithmetic, operation by operation: the GPU tests compare all six outputs with `==`.

status: 0 converged, 1 stopped at maxiter (the current Ritz values and bounds are still returned).
"""
import numpy as np

from viprs_amd.plan import SpectrumInfo

from .ld_dot_reference import block_matrix
from .ridge_reference import block_systems, blocks_of

def start_vector(n):
    """u of a block of n SNPs, float64 (every entry is exact in float32)."""
    h = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    h = h ^ (h >> np.uint64(31))
    return (h >> np.uint64(40)).astype(np.float64) * 2.0 ** -24 - 0.5 + 2.0 ** -25


def check_points(maxiter):
    """k = 1, 2, 4, ... below maxiter, then maxiter."""
    ks, k = [], 1
    while k < maxiter:
        ks.append(k)
        k *= 2
    return ks + [int(maxiter)]


def ritz_extremes(alpha, beta):
    """(theta_min, theta_max, resid_min, resid_max) of T_k: diagonal alpha[:k], off-diagonal beta[:k - 1], with beta[k - 1]
    = beta_{k+1} the coefficient of the residual bounds."""
    k = len(alpha)
    T = np.diag(np.asarray(alpha, dtype=np.float64))
    if k > 1:
        off = np.asarray(beta[:k - 1], dtype=np.float64)
        T += np.diag(off, 1) + np.diag(off, -1)
    theta, S = np.linalg.eigh(T)
    return theta[0], theta[-1], beta[k - 1] * abs(S[-1, 0]), beta[k - 1] * abs(S[-1, -1])


def _default_dot(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


def lanczos_block(R_off, dq, rtol, maxiter, dtype, off=None, dot=None, ritz=None, n=None):
    """One block.  R_off: stored off-diagonal entries (float64, not dequantised; unused with `off`, which needs the size
    `n`); dq a T scalar.  `off`, `dot`, `ritz`: the seams of the module docstring.
    Returns (theta_min, theta_max, resid_min, resid_max, iterations, status)."""
    dtype = np.dtype(dtype)
    T = dtype.type
    n = R_off.shape[0] if n is None else int(n)
    if off is None:
        off = lambda v: (R_off @ v.astype(np.float64)).astype(dtype)
    _dot = _default_dot if dot is None else dot
    ritz = ritz_extremes if ritz is None else ritz
    u = start_vector(n)
    v = (u / np.sqrt(_dot(u, u))).astype(dtype)
    v_prev = np.zeros(n, dtype=dtype)
    alpha, beta = [], []
    b = 0.0
    checks = set(check_points(maxiter))
    out = None
    for k in range(1, int(maxiter) + 1):
        w = (dq * off(v)) + v
        w = w - T(b) * v_prev
        a = _dot(v, w)
        w = w - T(a) * v
        b = np.sqrt(_dot(w, w))
        alpha.append(a)
        beta.append(b)
        if b == 0.0 or k in checks:
            lo, hi, r_lo, r_hi = out = ritz(alpha, beta)
            scale = max(abs(lo), abs(hi))
            if b == 0.0 or (r_lo <= rtol * scale and r_hi <= rtol * scale):
                return lo, hi, r_lo, r_hi, k, SpectrumInfo.CONVERGED
        v_prev, v = v, (w.astype(np.float64) / b).astype(dtype)
    return out + (int(maxiter), SpectrumInfo.MAXITER)


def extremal_eigenvalues(lb, ip, data, low_memory, dq_scale=1.0, rtol=None, maxiter=None, float_precision="float32",
                         off_product=None, dot=None, ritz=None):
    """The host model over every block: a `SpectrumInfo` like `LDPlan.extremal_eigenvalues` returns.  `off_product(s, e)`
    gives the `off` of block [s, e) (None: the float64 matrix product); `dot` and `ritz` are handed to every block."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    dtype = np.dtype(float_precision)
    assert dtype in (np.float32, np.float64)
    rtol = 1e-4 if rtol is None else float(rtol)
    maxiter = 2048 if maxiter is None else int(maxiter)
    dq = dtype.type(dq_scale)
    data64 = np.asarray(data, dtype=np.float64)
    rows = []
    for s, e in blocks_of(lb, ip, low_memory):
        R = block_matrix(lb, ip, data64, low_memory, s, e)[0] if off_product is None else None
        rows.append(lanczos_block(R, dq, rtol, maxiter, dtype, None if off_product is None else off_product(s, e), dot,
                                  ritz, e - s))
    cols = list(zip(*rows)) if rows else [[]] * 6
    return SpectrumInfo(*cols)


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------
def run_blocks(args, dq_scale, T, rtol, factor=5):
    """The host model with maxiter = factor x size for every block of its own, and the dense spectra."""
    lb, ip, data, low_memory = args
    lb, ip, data64 = np.asarray(lb), np.asarray(ip, dtype=np.int64), np.asarray(data, dtype=np.float64)
    dq = np.dtype(T).type(dq_scale)
    rows, eigs = [], []
    for (s, e), (_, _, A) in zip(blocks_of(lb, ip, low_memory), block_systems(*args, 0.0, dq_scale, T)):
        R, _ = block_matrix(lb, ip, data64, low_memory, s, e)
        rows.append(lanczos_block(R, dq, rtol, factor * (e - s), T))
        eigs.append(np.linalg.eigvalsh(A))
    return SpectrumInfo(*zip(*rows)), eigs


def check_against_dense(info, eigs, rtol):
    """status 0, both error bounds and both residual bounds; returns the worst error / (rtol scale)."""
    worst = 0.0
    assert np.all(info.status == 0), info.status
    for k, ev in enumerate(eigs):
        scale = max(abs(ev[0]), abs(ev[-1]))
        e_lo, e_hi = abs(info.lambda_min[k] - ev[0]), abs(info.lambda_max[k] - ev[-1])
        worst = max(worst, e_lo / (rtol * scale), e_hi / (rtol * scale))
        assert e_lo <= rtol * scale and e_hi <= rtol * scale, (k, e_lo / (rtol * scale), e_hi / (rtol * scale))
        ritz_scale = max(abs(info.lambda_min[k]), abs(info.lambda_max[k]))
        assert info.resid_min[k] <= rtol * ritz_scale and info.resid_max[k] <= rtol * ritz_scale, k
    return worst
