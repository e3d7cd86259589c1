"""Host reference of the device prep and of the M-step / ELBO sums (plain NumPy, no package imports).

Written from the statements the device code cites -- the reference's `VIPRS.e_step` prep (VIPRS.py:400-418), `compute_zeta`
(:896), the M-step (:426-471) and the ELBO (:497-581), `VIPRSMix.py:169-260` -- and from the sums layouts of
include/viprs_hip.h.  It is NOT a transcription of the kernels: every sum is the exactly rounded sum (`math.fsum`) of its
per-SNP float64 terms, so it does not depend on any summation order, and it comes with `fsum(|terms|)`, the scale the rounding
error of a floating-point summation of those terms is bounded by.

C_* below: the number of rounded float64 operations in ONE term of each sum (counted beside the term), a `log` counted
with `LOG_ULPS` roundings.  tests/test_em_reference.py pins this module to the host path of the package.
"""
import math

import numpy as np

f64 = np.float64
EPS64 = float(np.finfo(np.float64).eps)          # 2^-52: one ulp of 1.0; a rounded operation errs by at most EPS64 / 2 relative
RES = 1e-15                                       # np.finfo(float64).resolution: the clip margin of the ELBO (VIPRS.py:509)

# How far one `log` of the implementation under test may sit from this module's `np.log`, in units of EPS64 |log x|.
# The ROCm installation carries no accuracy table for its device library's float64 `log`, so this is the measured figure,
# doubled: on an MI355X (ROCm 7.2) the device's log differs from `np.log` by at most 1.00 ulp over the 140 000 inputs of
# `test_device_log_accuracy` (tests/test_gpu_prep_sums.py; EXPERIMENTS.md 6.11), in 1 519 of them.
LOG_ULPS = 2.0 * 1.0

N_SUMS = 11


def mixture_n_sums(K):
    return 7 + 6 * K


# ---- prep -------------------------------------------------------------------------------------------------------------------
def prep(n, logit_pi, log_tau_beta, sigma_eps, tau_beta, one_plus_lambda, dtype, grid=False):
    """Spike-and-slab (and one column / (group, column) pair of a grid state, `grid=True`): float64, cast at the end.
    Returns var_tau (float64) and the three E-step inputs in `dtype`; `shvt` is sqrt(var_tau / 2), or var_tau / 2 for a grid."""
    n = np.asarray(n, dtype=f64)
    vt = n * f64(one_plus_lambda) / f64(sigma_eps) + f64(tau_beta)
    half = 0.5 * vt
    return {"var_tau": vt,
            "mu_mult": (n / (vt * f64(sigma_eps))).astype(dtype),
            "u_logs": (f64(logit_pi) + 0.5 * (f64(log_tau_beta) - np.log(vt))).astype(dtype),
            "shvt": (half if grid else np.sqrt(half)).astype(dtype)}


def prep_mixture(n, logit_pi, log_tau_beta, tau_beta, log_null_pi, sigma_eps, one_plus_lambda, dtype):
    """(m, K) arrays, C order: component k of SNP j takes n_j and (logit_pi, log_tau_beta, tau_beta)[k]."""
    n = np.asarray(n, dtype=f64).reshape(-1, 1)                             # (m,) or the mixture model's (m, 1)
    lp, lt, tau = (np.asarray(x, dtype=f64)[None, :] for x in (logit_pi, log_tau_beta, tau_beta))
    vt = n * f64(one_plus_lambda) / f64(sigma_eps) + tau
    return {"var_tau": vt,
            "mu_mult": (n / (vt * f64(sigma_eps))).astype(dtype),
            "u_logs": (lp + 0.5 * (lt - np.log(vt))).astype(dtype),
            "shvt": np.sqrt(0.5 * vt).astype(dtype),
            "log_null_pi": np.full(n.shape[0], log_null_pi, dtype=f64).astype(dtype)}


def u_logs_bound(logit_pi, log_tau_beta, var_tau):
    """Bound on |u_logs(device) - u_logs(here)| for a float64 state, elementwise.  With u = EPS64 / 2 and
    A = max(|logit_pi|, |log_tau_beta|, |log var_tau|), both sides evaluate  r = fl(logit_pi + 0.5 * fl(log_tau_beta - L)):
      * the two L differ by at most LOG_ULPS * EPS64 * |log var_tau|; halved: LOG_ULPS * u * A
      * the subtraction is rounded once on each side, u |log_tau_beta - L| <= 2 u A each, halved (exactly): 2 u A together
      * the addition is rounded once on each side, u |r| <= u (A + A) each: 4 u A together
    so |difference| <= (LOG_ULPS + 6) * u * A (first order; the products of two roundings are below 2^-100 A)."""
    A = np.maximum(np.maximum(np.abs(np.asarray(logit_pi, dtype=f64)), np.abs(np.asarray(log_tau_beta, dtype=f64))),
                   np.abs(np.log(var_tau)))
    return (LOG_ULPS + 6.0) * 0.5 * EPS64 * A


# ---- sums -------------------------------------------------------------------------------------------------------------------
def _fsum(terms):
    """(fsum(terms), fsum(|terms|)); the sums of no terms are 0.  A NaN term makes both NaN."""
    t = np.asarray(terms, dtype=f64).ravel()
    if np.isnan(t).any():
        return math.nan, math.nan
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())


def _clip(x):
    return np.clip(x, RES, 1.0 - RES)


def _max_abs(ed):
    return float(np.max(np.abs(np.asarray(ed, dtype=f64)))) if np.size(ed) else 0.0


# rounded operations per term (float64; inputs, casts from the state dtype and clipping are exact)
C_ZETA = 4                                        # mu * mu, 1 / var_tau, +, gamma *
C_SPIKE_SLAB = (1,                                # [0] gamma * weight (0 without weights)
                C_ZETA,                           # [1] zeta
                C_ZETA + 2,                       # [2] one_plus_lambda * zeta, + (q * eta formed in the state dtype: part of the term)
                1,                                # [3] std_beta * eta
                1,                                # [4] eta * eta
                LOG_ULPS + 1,                     # [5] log, gamma_c *
                LOG_ULPS + 2,                     # [6] 1 - gamma, log, *
                0,                                # [7] gamma_c
                1,                                # [8] 1 - gamma
                LOG_ULPS + 1)                     # [9] log var_tau, gamma_c *


def sums_terms(gamma, mu, eta, q, std_beta, var_tau, one_plus_lambda, weight=None):
    """The ten per-SNP term arrays of the spike-and-slab / grid sums [0..9] (viprs_hip.h), float64."""
    g, m_, e = (np.asarray(x).astype(f64) for x in (gamma, mu, eta))
    vt = np.asarray(var_tau, dtype=f64)
    zeta = g * (m_ * m_ + 1.0 / vt)                                          # VIPRS.py:896
    qe = np.multiply(q, eta).astype(f64)                                     # in the state dtype, as the reference's np.multiply
    gc, ng = _clip(g), _clip(1.0 - g)
    return [g if weight is None else g * np.asarray(weight, dtype=f64),      # update_pi: sum of per-chromosome means
            zeta,
            f64(one_plus_lambda) * zeta + qe,                                # :455
            np.asarray(std_beta).astype(f64) * e,
            e * e,
            gc * np.log(gc), ng * np.log(ng), gc, ng,                        # entropy / prior terms of the ELBO
            gc * np.log(vt)]


def sums(gamma, mu, eta, q, eta_diff, std_beta, var_tau, one_plus_lambda, weight=None):
    """(exact, scale): 11 exactly rounded sums ([10] = max |eta_diff|) and fsum(|terms|) of each (0 for [10])."""
    pairs = [_fsum(t) for t in sums_terms(gamma, mu, eta, q, std_beta, var_tau, one_plus_lambda, weight)]
    exact = np.array([p[0] for p in pairs] + [_max_abs(eta_diff)])
    return exact, np.array([p[1] for p in pairs] + [0.0])


def sums_ops(weighted=True):
    """Rounded operations per term of sums [0..9]."""
    c = np.array(C_SPIKE_SLAB, dtype=f64)
    if not weighted:
        c[0] = 0
    return c


def mixture_sums_terms(gamma, mu, eta, q, std_beta, var_tau, log_var_tau0, one_plus_lambda):
    """Term arrays in the layout s[0..5] | kv[6][K] of `viprs_state_sums_mixture_end` (VIPRSMix._partial_sums):
    a list of 6 + 6 K arrays of length m.  `log_var_tau0` is what `set_log_var_tau` was given (the reference's ELBO keeps
    the log of the INITIAL var_tau), not log(var_tau)."""
    g, m_ = np.asarray(gamma).astype(f64), np.asarray(mu).astype(f64)
    e = np.asarray(eta).astype(f64)
    vt, lv0 = np.asarray(var_tau, dtype=f64), np.asarray(log_var_tau0, dtype=f64)
    K = g.shape[1]
    second = m_ * m_ + 1.0 / vt                                              # E[beta^2 | component k]
    z = g * second
    zeta, gsum = np.zeros(g.shape[0]), np.zeros(g.shape[0])
    for k in range(K):                                                       # over the components, in order
        zeta = zeta + z[:, k]
        gsum = gsum + g[:, k]
    qe = np.multiply(q, eta).astype(f64)
    ng = _clip(1.0 - gsum)
    gc = _clip(g)
    s = [zeta, f64(one_plus_lambda) * zeta + qe, np.asarray(std_beta).astype(f64) * e, e * e, ng * np.log(ng), ng]
    kv = [g, z, gc * np.log(gc), gc, gc * lv0, gc * second]
    return s + [row[:, k] for row in kv for k in range(K)]


def mixture_sums_ops(K):
    """Rounded operations per term, same layout (6 + 6 K)."""
    s = [C_ZETA + (K - 1), C_ZETA + (K - 1) + 2, 1, 1, (K - 1) + 1 + LOG_ULPS + 1, (K - 1) + 1]
    kv = [0, C_ZETA, LOG_ULPS + 1, 0, 1, C_ZETA]
    return np.array(s + [c for c in kv for _ in range(K)], dtype=f64)


def mixture_sums(gamma, mu, eta, q, eta_diff, std_beta, var_tau, log_var_tau0, one_plus_lambda):
    """(exact, scale) of the 7 + 6 K mixture sums; the last is max |eta_diff|."""
    pairs = [_fsum(t) for t in mixture_sums_terms(gamma, mu, eta, q, std_beta, var_tau, log_var_tau0, one_plus_lambda)]
    exact = np.array([p[0] for p in pairs] + [_max_abs(eta_diff)])
    return exact, np.array([p[1] for p in pairs] + [0.0])


# ---- the reduction's contract (include/viprs_hip.h) ------------------------------------------------------------------------
SUMS_BLOCK = 256
CAP = {"spike_slab": 1024, "mixture": 1024, "grid": 256}


def reduction_depth(length, kind):
    """D: additions on the longest path of a row's reduction.  A row of `length` SNPs takes
    nb = min(ceil(length / 256), cap) workgroups of 256 threads; thread t of workgroup b adds elements
    b * 256 + t, + nb * 256, ... serially (ceil(length / (nb * 256)) additions), the workgroup combines its 256 accumulators
    in a tree (8 levels in LDS; mixture rows: 6 shuffle levels, then 3 additions over the 4 waves), and the final pass adds the
    nb partials 64 lanes wide (ceil(nb / 64) serial additions per lane, then 6 shuffle levels)."""
    if length <= 0:
        return 0
    nb = min(-(-length // SUMS_BLOCK), CAP[kind])
    serial = -(-length // (nb * SUMS_BLOCK))
    tree = 9 if kind == "mixture" else 8
    return serial + tree + -(-nb // 64) + 6


def sums_bound(scale, ops, length, kind):
    """|device - exact| <= EPS64 * (D + C) * fsum(|terms|): the textbook worst case of a floating-point summation with D
    additions on its longest path over terms that carry C rounded operations each."""
    return EPS64 * (reduction_depth(length, kind) + np.asarray(ops, dtype=f64)) * np.asarray(scale, dtype=f64)
