"""Host replay of `viprs_plan_susie` (include/viprs_hip.h): the step of the header, operation for operation -- what the `==`
tests of tests/test_gpu_susie.py compare the device with.

    per-SNP operations   NumPy float64 elementwise operations, one ufunc call per IEEE operation of the header (nothing can be
                         contracted across calls); roundings to the state precision T by `astype`
    exp                  `math.exp`: the host libm's (NumPy's vectorised `exp` is not glibc's)
    S, Q                 `order_replay.ordered_dot` against a vector of ones (the product with 1 is exact): the 256-thread
                         order of the solvers with chunks of 16 / sizeof(T) elements
    the product          `order_replay.BlockProduct` (the product's own order in T) and `ld_dot_reference.finish`
    log_prior = None     `-math.log(float(size))`
"""
import math

import numpy as np

from viprs_amd.plan import SusieInfo, susie_inputs

from . import ld_dot_reference as LDR
from . import order_replay as OR
from .ridge_reference import blocks_of


def _exp(x):
    return np.array([math.exp(v) for v in x], dtype=np.float64)


def replay_block(off, z, lp, L, V0, estimate, dq_scale, tol, max_iter, T):
    """One block: (alpha, mu, V, post_var, iterations, delta, status)."""
    n = z.shape[0]
    T = np.dtype(T)
    chunk = 16 // T.itemsize
    ones = np.ones(n)
    alpha = np.zeros((n, L), dtype=T)
    mu = np.zeros((n, L), dtype=T)
    Rb = np.zeros((n, L), dtype=T)
    V = np.array(V0, dtype=np.float64)
    post_var = np.zeros(L)
    Y = None
    for it in range(1, max_iter + 1):
        delta = 0.0
        for l in range(L):
            if Y is not None:
                Rb[:, (l - 1) % L] = Y
            acc = np.zeros(n)
            for k in range(L):
                if k != l:
                    acc = acc + Rb[:, k].astype(np.float64)
            r = z - acc
            s = V[l] / (1.0 + V[l])
            w = (0.5 * (r * r)) * s + lp
            mu[:, l] = (s * r).astype(T)
            e = _exp(w - np.max(w))
            md = mu[:, l].astype(np.float64)
            S = OR.ordered_dot(e, ones, chunk)
            Q = OR.ordered_dot(e * (s + md * md), ones, chunk)
            a_new = (e / S).astype(T)
            d = float(np.max(np.abs(a_new.astype(np.float64) - alpha[:, l].astype(np.float64))))
            bbar = (a_new.astype(np.float64) * md).astype(T)
            alpha[:, l] = a_new
            post_var[l] = s
            if estimate:
                V[l] = Q / S
            delta = d if l == 0 else max(delta, d)
            Y = LDR.finish(off(bbar), bbar, dq_scale, True, T)
        if delta < tol:
            return alpha, mu, V, post_var, it, delta, SusieInfo.CONVERGED
    return alpha, mu, V, post_var, max_iter, delta, SusieInfo.MAXITER


def susie_replay(lb, ip, data, low_memory, z, L=10, prior_variance=50.0, estimate_prior_variance=True, log_prior=None,
                 dq_scale=1.0, tol=1e-4, max_iter=100, float_precision="float32"):
    """The signature of `viprs_amd.stats.susie.susie_host`; a `SusieInfo` whose every field is the device's, bit for bit."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    blocks = blocks_of(lb, ip, low_memory)
    nb = len(blocks)
    L = int(L)
    T = np.dtype(float_precision)
    z, v, v0, lp = susie_inputs(m, nb, z, L, prior_variance, log_prior)
    V0 = np.full((nb, L), v0) if v is None else v
    product = OR.BlockProduct(lb, ip, data, low_memory)
    alpha = np.zeros((m, L), dtype=T, order="F")
    mu = np.zeros((m, L), dtype=T, order="F")
    V = np.zeros((nb, L))
    post_var = np.zeros((nb, L))
    iters, delta, status = np.zeros(nb, np.int32), np.zeros(nb), np.zeros(nb, np.int32)
    for k, (s, e) in enumerate(blocks):
        lpb = np.full(e - s, -math.log(float(e - s))) if lp is None else lp[s:e]
        with np.errstate(over="ignore", invalid="ignore"):
            out = replay_block(product(s, e), z[s:e], lpb, L, V0[k], bool(estimate_prior_variance), dq_scale, float(tol),
                               int(max_iter), T)
        alpha[s:e], mu[s:e], V[k], post_var[k], iters[k], delta[k], status[k] = out
    starts = np.array([b[0] for b in blocks] + [m], dtype=np.int64)
    return SusieInfo(alpha, mu, V, post_var, iters, delta, status, starts)
