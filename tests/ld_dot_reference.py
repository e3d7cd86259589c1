"""Host reference of the LD product (include/viprs_hip.h, `viprs_plan_dot`), written from its definition:

    S[j, g] = sum over the off-diagonal entries (j, i) of row j of the symmetric matrix the arrays stand for of r_ji B[i, g]

Symmetric form: row j stores columns left_bound[j] .. left_bound[j] + len_j - 1, the diagonal entry among them is skipped.
Upper form (low_memory): row j stores columns j + 1 .. j + len_j; the transposed entries (i, j) of the rows i < j that reach
j count too.

`reference(...)` returns
    exact      the product: Python-integer arithmetic (mode "int": every r_ji and B value is an integer and the sums stay
               below 2**53, so a float64 matrix product IS the integer product -- checked) or `math.fsum` over the float64
               terms (mode "fsum": products of two float32 values are exact in float64)
    abs_terms  sum |r_ji B[i, g]| per row and column (mode "abs": only this, L and W are computed)
    L          stored off-diagonal entries per row
    W          width of the row's window (first to last column that holds an entry or the diagonal): L + 1 when the window
               has no gaps
`depth(W, itemsize)` is the header's D: additions on the longest path of a row.
"""
import math

import numpy as np

from viprs_amd.plan import plan_blocks


def depth(W, ld_itemsize):
    """D = ceil(W / (64 V)) + log2(V) + 6 with V = 16 / sizeof(LD element) (the contract in include/viprs_hip.h)."""
    V = 16 // int(ld_itemsize)
    W = np.asarray(W, dtype=np.int64)
    return (W + 64 * V - 1) // (64 * V) + int(math.log2(V)) + 6


def block_matrix(lb, ip, data, low_memory, s, e):
    """(R, stored): the off-diagonal part of rows s..e-1 as a dense float64 square and the mask of stored entries."""
    b = e - s
    R = np.zeros((b, b), dtype=np.float64)
    M = np.zeros((b, b), dtype=bool)
    for j in range(s, e):
        n = int(ip[j + 1] - ip[j])
        if n == 0:
            continue
        c0 = int(lb[j]) - s
        assert 0 <= c0 and c0 + n <= b, "a row window leaves its block"
        R[j - s, c0:c0 + n] = data[ip[j]:ip[j + 1]]
        M[j - s, c0:c0 + n] = True
    if low_memory:
        assert not np.tril(M).any(), "upper form: entries on or below the diagonal"
        R = R + R.T
        M = M | M.T
    else:
        d = np.arange(b)
        R[d, d] = 0.0
        M[d, d] = False
    return R, M


def reference(lb, ip, data, low_memory, B, mode="fsum"):
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    B2 = np.asarray(B, dtype=np.float64).reshape(m, -1)
    G = B2.shape[1]
    exact = np.zeros((m, G), dtype=np.float64)
    abs_terms = np.zeros((m, G), dtype=np.float64)
    L = np.zeros(m, dtype=np.int64)
    W = np.zeros(m, dtype=np.int64)
    starts, _ = plan_blocks(np.ascontiguousarray(lb, dtype=np.int32), np.ascontiguousarray(ip), low_memory)
    for s, e in zip(starts[:-1], starts[1:]):
        s, e = int(s), int(e)
        R, M = block_matrix(lb, ip, data, low_memory, s, e)
        Bb = B2[s:e]
        abs_terms[s:e] = np.abs(R) @ np.abs(Bb)
        L[s:e] = M.sum(axis=1)
        Md = M.copy()
        d = np.arange(e - s)
        Md[d, d] = True
        first = Md.argmax(axis=1)
        last = (e - s) - 1 - Md[:, ::-1].argmax(axis=1)
        W[s:e] = last - first + 1
        if mode == "int":
            assert np.array_equal(R, np.rint(R)) and np.array_equal(Bb, np.rint(Bb)), "mode 'int' needs integer values"
            assert abs_terms[s:e].max(initial=0.0) < 2.0 ** 53
            exact[s:e] = R @ Bb
        elif mode == "fsum":
            for r in range(e - s):
                idx = np.nonzero(M[r])[0]
                if idx.size == 0:
                    continue
                terms = R[r, idx][:, None] * Bb[idx]
                for g in range(G):
                    exact[s + r, g] = math.fsum(terms[:, g])
    shape = np.asarray(B).shape
    return {"exact": exact.reshape(shape), "abs_terms": abs_terms.reshape(shape), "L": L, "W": W}


def finish(S, B, dq_scale, include_diagonal, dtype):
    """The header's last two operations in the state precision: fl(fl(dq_scale) * S) (+ B)."""
    T = np.dtype(dtype).type
    y = T(dq_scale) * np.asarray(S).astype(dtype)
    if include_diagonal:
        y = y + np.asarray(B, dtype=dtype)
    return y.astype(dtype)


def dot_fn(arrays):
    """`dot_fn=` for viprs_amd.eval.pseudo_metrics: `ld` objects are (left_bound, indptr, data, low_memory, dq_scale) tuples;
    R has a unit diagonal and off-diagonal entries dq_scale * stored, evaluated in float64."""
    def fn(ld, B):
        lb, ip, data, low_memory, dq = ld
        ref = reference(lb, ip, np.asarray(data, dtype=np.float64), low_memory, B, mode="fsum")
        return dq * ref["exact"] + np.asarray(B, dtype=np.float64)
    return fn if arrays is None else fn(arrays[0], arrays[1])
