"""Host replay of THE ORDER of every sum the LD product, the LD scores and the two solvers form on the device, as
include/viprs_hip.h states it -- what the `==` tests of the four calls compare with.

    replay_dot / replay_scores   the product's order: entry e of a row's window to accumulator e % V of lane (e / V) % 64,
                                 one FMA per entry in the state precision T, a binary tree over V, the xor butterfly over
                                 the lanes (oracle/ld_order_replay.c through ctypes: libm `fmaf` / `fma` -- Python 3.10 has
                                 no `math.fma`, and a float32 FMA emulated in float64 rounds twice).  They return the sums
                                 BEFORE the epilogue: S, resp. (S2, S0); the epilogues stay in ld_dot_reference.finish /
                                 ld_score_reference.finish
    ordered_dot                  the solvers' dot product: 16-byte chunks dealt to 256 threads, one float64 accumulator per
                                 thread, the butterfly over each wavefront, the four wavefronts in order (NumPy)
    BlockProduct                 the off-diagonal product of one LD block in the product's order: the `off_product=` seam of
                                 ridge_reference.solve / lanczos_reference.extremal_eigenvalues
    ritz_extremes                the Ritz extremes by the library's own host routine (`viprs_tridiagonal_extremes`, pinned
                                 against `eigh` by tests/test_lanczos_reference.py): the `ritz=` seam of the Lanczos model
    replayed_solve / replayed_spectrum   the two host models driven by all of the above
"""
import ctypes
import functools
import os
import subprocess

import numpy as np

_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
_PATH = os.path.join(_ORACLE, "libldreplay.so")
_SUFFIX = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
N_THREADS = 256                # the solvers' workgroup
_vp = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def _lib():
    if not os.path.exists(_PATH):
        subprocess.run(["make", "-C", _ORACLE, "libldreplay.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(_PATH)
    for sfx in _SUFFIX.values():
        f = getattr(lib, f"ld_replay_dot_{sfx}")
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]
        f = getattr(lib, f"ld_replay_scores_{sfx}")
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]
    return lib


def _p(a):
    return a.ctypes.data_as(_vp)


def _windows(lb, ip, data, dtype):
    """The index arrays as the C replay takes them, the LD elements converted to T (one rounding for int32 / int64 / fp64
    LD in a float32 state: the conversion the header names) and V = 16 / sizeof(stored LD element)."""
    data = np.asarray(data)
    lb = np.ascontiguousarray(lb, dtype=np.int32)
    ip = np.ascontiguousarray(ip, dtype=np.int64)
    assert ip.shape[0] == lb.shape[0] + 1 and int(ip[-1]) == data.shape[0]
    return lb, ip, np.ascontiguousarray(data.astype(dtype)), 16 // data.dtype.itemsize


def replay_dot(lb, ip, data, low_memory, B, dtype=None):
    """S of `viprs_plan_dot` (the sum before dq_scale), in THE ORDER: `B` is (m,) or (m, G); the result has its shape, in
    T."""
    B = np.asarray(B)
    dtype = np.dtype(B.dtype if dtype is None else dtype)
    lb, ip, x, V = _windows(lb, ip, data, dtype)
    m = lb.shape[0]
    b = np.asfortranarray(B.astype(dtype))
    assert b.shape[0] == m and b.ndim in (1, 2)
    S = np.zeros(b.shape, dtype=dtype, order="F")
    n_cols = 1 if b.ndim == 1 else b.shape[1]
    rc = getattr(_lib(), f"ld_replay_dot_{_SUFFIX[dtype]}")(m, _p(lb), _p(ip), _p(x), V, int(bool(low_memory)), n_cols,
                                                             _p(b), _p(S))
    assert rc == 0, "ld_replay_dot: bad arguments"
    return S


def replay_scores(lb, ip, data, low_memory, A, dtype):
    """(S2, S0) of `viprs_plan_ld_scores` in THE ORDER; `A` None: one column of ones, results of shape (m,)."""
    dtype = np.dtype(dtype)
    lb, ip, x, V = _windows(lb, ip, data, dtype)
    m = lb.shape[0]
    if A is None:
        a, shape, n_cols = None, (m,), 1
    else:
        a = np.asfortranarray(np.asarray(A).astype(dtype))
        assert a.shape[0] == m and a.ndim in (1, 2)
        shape, n_cols = a.shape, (1 if a.ndim == 1 else a.shape[1])
    S2 = np.zeros(shape, dtype=dtype, order="F")
    S0 = np.zeros(shape, dtype=dtype, order="F")
    rc = getattr(_lib(), f"ld_replay_scores_{_SUFFIX[dtype]}")(m, _p(lb), _p(ip), _p(x), V, int(bool(low_memory)), n_cols,
                                                                None if a is None else _p(a), _p(S2), _p(S0))
    assert rc == 0, "ld_replay_scores: bad arguments"
    return S2, S0


# ---- the solvers' dot product ---------------------------------------------------------------------------------------------
def thread_partials(a, b, V=None):
    """The 256 per-thread accumulators of a dot product: element e belongs to chunk e // V (V = 16 / sizeof(T): the elements
    of 16 bytes), chunk c to thread c % 256; a thread adds fl(a_e b_e) to ONE float64 accumulator in ascending e -- the
    multiply and the add are two separately rounded float64 operations.  (A thread without an element at some step adds an
    exact +0.)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.ndim == 1 and a.shape == b.shape
    V = 16 // a.dtype.itemsize if V is None else int(V)
    n = a.shape[0]
    span = N_THREADS * V
    passes = max(1, -(-n // span))
    prod = np.zeros(passes * span, dtype=np.float64)
    prod[:n] = a.astype(np.float64) * b.astype(np.float64)
    prod = prod.reshape(passes, N_THREADS, V)
    acc = np.zeros(N_THREADS, dtype=np.float64)
    for p in range(passes):
        for i in range(V):
            acc = acc + prod[p, :, i]
    return acc


def reduce_threads(acc):
    """6 xor-butterfly levels inside each wavefront of 64 lanes, then the 4 wavefront sums in wavefront order."""
    t = np.asarray(acc, dtype=np.float64).reshape(N_THREADS // 64, 64)
    lane = np.arange(64)
    w = 1
    while w < 64:
        t = t + t[:, lane ^ w]
        w *= 2
    s = t[0, 0]
    for k in range(1, t.shape[0]):
        s = s + t[k, 0]
    return float(s)


def ordered_dot(a, b, V=None):
    """a . b in the order of the solvers (ridge.h): a float64 value, a function of the vectors and of V alone."""
    return reduce_threads(thread_partials(a, b, V))


# ---- the seams of the two host models -------------------------------------------------------------------------------------
def block_arrays(lb, ip, data, s, e):
    """Rows s .. e - 1 of the arrays as a panel of their own (one LD block: its windows do not leave it)."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    o0, o1 = int(ip[s]), int(ip[e])
    sub_lb = np.clip(lb[s:e].astype(np.int64) - s, 0, max(e - s - 1, 0)).astype(np.int32)
    return sub_lb, ip[s:e + 1] - o0, np.asarray(data)[o0:o1]


class BlockProduct:
    """`off_product=` of the host models: `BlockProduct(...)(s, e)` is the function v -> S of block [s, e): the sum over the
    stored off-diagonal entries (not dequantised), in the state precision of `v`, in the product's own order."""

    def __init__(self, lb, ip, data, low_memory):
        self.args = (np.asarray(lb), np.asarray(ip, dtype=np.int64), np.asarray(data))
        self.low_memory = bool(low_memory)

    def __call__(self, s, e):
        lb, ip, data = block_arrays(*self.args, s, e)
        return lambda v: replay_dot(lb, ip, data, self.low_memory, v)


def dot_for(dtype):
    """`dot=` of the host models for the state precision `dtype`: a chunk holds 16 / sizeof(T) elements in every dot product
    of a solve, whatever the operands are (header: the start vector of the Lanczos recurrence is summed in float64 values,
    16 / sizeof(T) of them to a chunk all the same)."""
    return functools.partial(ordered_dot, V=16 // np.dtype(dtype).itemsize)


def ritz_extremes(alpha, beta):
    """(theta_min, theta_max, resid_min, resid_max) of T_k by the library's host routine; beta[k - 1] = beta_{k+1}."""
    from viprs_amd import _lib as L
    k = len(alpha)
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    b = np.ascontiguousarray(beta[:k - 1], dtype=np.float64)
    out = np.zeros(4)
    rc = L.lib.viprs_tridiagonal_extremes(k, _p(a), _p(b) if k > 1 else None, _p(out))
    assert rc == L.OK
    res = float(beta[k - 1])
    return float(out[0]), float(out[1]), res * float(out[2]), res * float(out[3])


def replayed_solve(lb, ip, data, low_memory, b, shift, dq_scale=1.0, rtol=None, maxiter=None, x0=None):
    from . import ridge_reference as RR
    return RR.solve(lb, ip, data, low_memory, b, shift, dq_scale, rtol, maxiter, x0,
                    off_product=BlockProduct(lb, ip, data, low_memory), dot=dot_for(np.asarray(b).dtype))


def replayed_spectrum(lb, ip, data, low_memory, dq_scale=1.0, rtol=None, maxiter=None, float_precision="float32"):
    from . import lanczos_reference as LR
    return LR.extremal_eigenvalues(lb, ip, data, low_memory, dq_scale, rtol, maxiter, float_precision,
                                   off_product=BlockProduct(lb, ip, data, low_memory), dot=dot_for(float_precision),
                                   ritz=ritz_extremes)
