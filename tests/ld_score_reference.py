"""Host reference of the LD scores (include/viprs_hip.h, `viprs_plan_ld_scores`), from the product's reference
(tests/ld_dot_reference.py): over the off-diagonal entries (j, i) of row j

    S2[j, g] = sum x_ji^2 A[i, g]      the product reference applied to the SQUARED stored entries
    S0[j, g] = sum A[i, g]             the product reference applied to ones in place of the entries

`sums(...)` returns both exactly (mode "int": integer entries and weights; mode "fsum": `math.fsum` over the float64 terms),
`P = sum x^2 |A|`, `Q = sum |A|` and the product's `L`, `W`.  `finish(...)` is the header's epilogue in NumPy scalars of the
state precision T; `bound(...)` the rounding bound that follows from the header's definition.
"""
import numpy as np

from tests import ld_dot_reference as R


def sums(lb, ip, stored, low_memory, A=None, mode="int"):
    """`stored`: the stored elements as float64 (mode "int": integers)."""
    m = np.asarray(lb).shape[0]
    stored = np.asarray(stored, dtype=np.float64)
    A2 = np.ones(m) if A is None else np.asarray(A, dtype=np.float64)
    sq = stored * stored                     # exact in float64: integers below 2^26, or float32 values (24-bit significands)
    r2 = R.reference(lb, ip, sq, low_memory, A2, mode=mode)
    r0 = R.reference(lb, ip, np.ones_like(stored), low_memory, A2, mode=mode)
    return {"S2": r2["exact"], "S0": r0["exact"], "P": r2["abs_terms"], "Q": r0["abs_terms"], "L": r2["L"], "W": r2["W"],
            "A": A2}


def finish(S2, S0, A, corr, dq_scale, dtype):
    """d = fl(dq_scale); d2 = fl(d d); U = fl(d2 S2); score = fl(U + A) or fl(fl(U + fl(c fl(U - S0))) + A), c = fl(corr[j]):
    every operation separately rounded in the state precision.  `S2`, `S0`: the sums as the device holds them (values of
    `dtype`).  `A`: the weights (None: ones)."""
    T = np.dtype(dtype).type
    S2 = np.asarray(S2).astype(dtype)
    S0 = np.asarray(S0).astype(dtype)
    a = np.ones(S2.shape, dtype=dtype) if A is None else np.asarray(A).astype(dtype)
    d = T(dq_scale)
    d2 = T(d * d)
    U = (d2 * S2).astype(dtype)
    if corr is None:
        return (U + a).astype(dtype)
    c = np.asarray(corr).astype(dtype)
    if S2.ndim == 2:
        c = c[:, None]
    t = (U - S0).astype(dtype)
    t = (c * t).astype(dtype)
    y = (U + t).astype(dtype)
    return (y + a).astype(dtype)


def exact_score(ref, corr, dq_scale, dtype):
    """The score the header defines, evaluated in float64 from the exact sums: d and c are the values ROUNDED to the state
    precision (that rounding is part of the definition)."""
    T = np.dtype(dtype).type
    d = float(T(dq_scale))
    U = d * d * ref["S2"]
    if corr is None:
        return U + ref["A"]
    c = np.asarray(corr).astype(dtype).astype(np.float64)
    if U.ndim == 2:
        c = c[:, None]
    return U + c * (U - ref["S0"]) + ref["A"]


def bound(ref, corr, dq_scale, dtype, ld_itemsize):
    """|device score - exact_score| <= this.  In units of eps_T (= 2 u: first-order terms counted at twice the unit roundoff,
    which covers the higher-order ones), with D = D(L) of the product, M0 = d^2 P + |a_j|:

      S2     eps (D + 1) P            (header: D additions on the longest path, + 1 for p = fl(x x))
      S0     eps D Q                  (header)
      U      two more roundings (d2, the product): |U - d^2 S2_exact| <= eps (D + 3) d^2 P
      no correction:    one rounded add                                   -> eps (D + 4) M0
      correction:       t1 = fl(U - S0), t2 = fl(c t1), t3 = fl(U + t2), t4 = fl(t3 + a): with
                        M = (1 + |c|) d^2 P + |c| Q + |a_j|
                        (1 + |c|) eps (D + 3) d^2 P + |c| eps D Q + 2 u |c| (d^2 P + Q) + 2 u M   -> eps (D + 5) M
      the reference itself: `fsum` of float64 products, each rounded once, <= 2^-53 of the same magnitudes -> + 1
    """
    T = np.dtype(dtype).type
    eps = float(np.finfo(dtype).eps)
    d = float(T(dq_scale))
    D = R.depth(ref["W"], ld_itemsize).astype(np.float64)
    P, Q, a = d * d * ref["P"], ref["Q"], np.abs(ref["A"])
    if P.ndim == 2:
        D = D[:, None]
    if corr is None:
        return eps * (D + 5) * (P + a)
    c = np.abs(np.asarray(corr).astype(dtype).astype(np.float64))
    if P.ndim == 2:
        c = c[:, None]
    return eps * (D + 6) * ((1 + c) * P + c * Q + a)
