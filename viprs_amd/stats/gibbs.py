"""The LDpred2 Gibbs sweep on the host: the definition `viprs_state_gibbs_sweep` / `viprs_state_gibbs_draws` are pinned to, and
the CPU fallback.

LDpred2 (Prive, Arbel and Vilhjalmsson 2020) draws every effect from its conditional posterior under a point-normal prior,
SNP after SNP over each LD block with a running ``q = (R - I) beta``.  With ``sigma_epsilon = 1``, ``lambda = 0`` and
``tau_beta = m p / h2`` its update is the grid-column E-step (`prep_columns` writes ``mu_mult``, ``half_var_tau`` and
``u_logs``) with a draw where the E-step stores ``gamma mu``.  One sweep, per SNP j in index order, every operation
separately rounded in float32 (include/viprs_hip.h states it with the device call):

    mu = mu_mult_j (beta_hat_j - q_j);  gamma = sigmoid(u_logs_j + (half_var_tau_j mu) mu)
    b = gamma > U_j ? mu + noise_j : +0;  d = b - eta_j
    var_mu[j] = mu;  var_gamma[j] = gamma;  eta_diff[j] = d;  eta[j] = b
    q[k] = fma(R[j, k], dq_scale d, q[k]) over the row's window in index order   (symmetric form: then q[j] -= d)

and, upper form, after the last SNP ``q[j] += dq_scale dot(row(j), eta_diff)`` with the dot a serial fma chain from 0.  The
sigmoid is the reference's (e_step.hpp:245-261: ``e = expf(-|x|)``, the add and the divide in double, rounded once) with the
C library's `expf`, called through ctypes: NumPy's float32 `exp` is another function.

The draws: one Philox4x32-10 block per (SNP j, column g) with key = the two halves of the seed and counter = (j, g, the two
halves of draw_index); ``U = (2 (x0 >> 9) + 1) 2^-24`` and ``u1``, ``u2`` likewise from ``x1``, ``x2``; ``z = sqrt(-2 log u1)
cos(2 pi u2)`` -- here in float64 and rounded to float32, on the device in float32 with its `logf` and `cospif(2 u2)`, so `U`
is the device's bit for bit and `z` is not -- and ``noise = z * (1 / sqrt(2 half_var_tau))``.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

from .enet import fma32

_F32, _F64, _U32, _U64 = np.float32, np.float64, np.uint32, np.uint64
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK = _U64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011), integer-exact: `counter` an array ``(..., 4)`` and `key` an array ``(..., 2)``
    (or ``(2,)``) of 32-bit words; returns the ``(..., 4)`` uint32 output blocks."""
    c = np.asarray(counter).astype(_U64) & _MASK
    k = np.broadcast_to(np.asarray(key).astype(_U64) & _MASK, c.shape[:-1] + (2,))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0 = _U64(PHILOX_M0) * c0                       # 32 x 32 bits: exact in 64
        p1 = _U64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> _U64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> _U64(32)) ^ c3 ^ k1, p0 & _MASK
        k0 = (k0 + _U64(PHILOX_W0)) & _MASK
        k1 = (k1 + _U64(PHILOX_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(_U32)


def _open_unit(x):
    """``(2 (x >> 9) + 1) 2^-24`` as float32: exact, strictly inside (0, 1)."""
    return ((2 * (x.astype(np.int64) >> 9) + 1).astype(_F64) * 2.0 ** -24).astype(_F32)


def gibbs_words_host(seed, draw_index, m, cols):
    """The Philox output blocks of SNPs ``0 .. m - 1`` for the listed columns: uint32 ``(m, len(cols), 4)``."""
    seed, draw_index = int(seed) & (2 ** 64 - 1), int(draw_index) & (2 ** 64 - 1)
    cols = np.atleast_1d(np.asarray(cols, dtype=np.int64))
    ctr = np.empty((int(m), cols.shape[0], 4), dtype=_U64)
    ctr[..., 0] = np.arange(int(m), dtype=_U64)[:, None] & _MASK
    ctr[..., 1] = cols[None, :].astype(_U64)
    ctr[..., 2] = draw_index & 0xFFFFFFFF
    ctr[..., 3] = draw_index >> 32
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=_U64))


def gibbs_normals_host(seed, draw_index, m, cols):
    """``(U, z)``, float32 ``(m, len(cols))``: the uniforms (the device's bit for bit) and the Box-Muller normals formed in
    float64 and rounded to float32."""
    w = gibbs_words_host(seed, draw_index, m, cols)
    u1 = _open_unit(w[..., 1]).astype(_F64)
    u2 = _open_unit(w[..., 2]).astype(_F64)
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return _open_unit(w[..., 0]), z.astype(_F32)


def gibbs_draws_host(seed, draw_index, half_var_tau, cols=None):
    """`viprs_state_gibbs_draws` on the host: ``(U, noise)``, float32 arrays of `half_var_tau`'s shape ``(m, G)`` in Fortran
    order, the listed columns (default: all) filled and the others zero."""
    hvt = np.asarray(half_var_tau)
    if hvt.dtype != _F32 or hvt.ndim != 2:
        raise ValueError("half_var_tau: a float32 array of shape (m, G)")
    m, G = hvt.shape
    cols = np.arange(G) if cols is None else np.atleast_1d(np.asarray(cols, dtype=np.int64))
    unif, noise = (np.zeros((m, G), dtype=_F32, order="F") for _ in range(2))
    if cols.shape[0] == 0 or m == 0:
        return unif, noise
    u, z = gibbs_normals_host(seed, draw_index, m, cols)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = _F32(1.0) / np.sqrt(_F32(2.0) * hvt[:, cols])
        unif[:, cols] = u
        noise[:, cols] = z * sd
    return unif, noise


@functools.lru_cache(maxsize=None)
def _expf():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.expf.restype = ctypes.c_float
    lib.expf.argtypes = [ctypes.c_float]
    return lib.expf


def sigmoid32(x):
    """The reference's float32 sigmoid (e_step.hpp:245-261) of one float32 value: `expf` of the C library, the add and the
    divide in double, one rounding to float32."""
    x = float(x)
    if x < 0:
        e = float(_expf()(x))
        return _F32(e / (1.0 + e))
    if x != x:
        return _F32(np.nan)
    e = float(_expf()(-x))
    return _F32(1.0 / (1.0 + e))


def _sweep_columns(lb, ip, x, low_memory, beta, mm, hvt, ulog, unif, noise, eta, q, dq):
    """All columns side by side (they are independent): every array ``(m, G)``, one walk over the SNPs."""
    m, G = eta.shape
    ed, mu_out, gam = (np.zeros((m, G), dtype=_F32) for _ in range(3))
    zero = _F32(0.0)
    xc = x[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            mu = mm[j] * (beta[j] - q[j])
            u = ulog[j] + hvt[j] * mu * mu
            gamma = np.array([sigmoid32(v) for v in u], dtype=_F32)
            b = np.where(gamma > unif[j], mu + noise[j], zero)
            d = b - eta[j]
            mu_out[j], gam[j], ed[j] = mu, gamma, d
            s, e = ip[j], ip[j + 1]
            if e > s:
                k = lb[j]
                q[k:k + e - s] = fma32(xc[s:e], (dq * d)[None, :], q[k:k + e - s])
            if not low_memory:
                q[j] = q[j] - d
            eta[j] = b
        if low_memory:
            # update_q_factor: every row's dot is a serial chain from 0 in index order; the chains advance side by side
            length = (ip[1:] - ip[:-1]).astype(np.int64)
            acc = np.zeros((m, G), dtype=_F32)
            rows = np.flatnonzero(length > 0)
            i = 0
            while rows.shape[0]:
                acc[rows] = fma32(xc[ip[rows] + i], ed[lb[rows] + i], acc[rows])
                i += 1
                rows = rows[length[rows] > i]
            q += dq * acc
    return ed, mu_out, gam


def gibbs_sweep_host(lb, ip, data, low_memory, std_beta, mu_mult, half_var_tau, u_logs, unif, noise, eta, q, dq_scale=1.0):
    """One Gibbs sweep (module docstring) over LD in the layout of `LDPlan` with the given draws; `mu_mult`, `half_var_tau`,
    `u_logs`, `unif`, `noise`, `eta`, `q` are float32 arrays ``(m,)`` or ``(m, G)`` (one column per chain: the columns are
    independent).  `eta` and `q` are updated IN PLACE; returns ``(eta_diff, var_mu, var_gamma)`` in their shape."""
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
    cols = []
    for a, name in ((mu_mult, "mu_mult"), (half_var_tau, "half_var_tau"), (u_logs, "u_logs"), (unif, "unif"), (noise, "noise"),
                    (eta, "eta"), (q, "q")):
        a = np.asarray(a)
        if a.dtype != _F32 or a.shape != shape or a.ndim not in (1, 2) or a.shape[0] != m:
            raise ValueError(f"{name}: a float32 array of the shape of eta, (m,) or (m, G)")
        cols.append(a.reshape(m, -1))
    MM, H, UL, UN, NO, E, Q = cols
    if not (np.shares_memory(E, eta) and np.shares_memory(Q, q)):
        raise ValueError("eta, q: contiguous per column (C order for (m,), Fortran order for (m, G))")
    rows = lambda a: np.ascontiguousarray(a)                # (m, G) with a SNP's columns side by side
    ej, qj = rows(E).copy(), rows(Q).copy()
    res = _sweep_columns(lb, ip, x, bool(low_memory), beta, rows(MM), rows(H), rows(UL), rows(UN), rows(NO), ej, qj,
                         _F32(dq_scale))
    E[...], Q[...] = ej, qj
    return tuple(np.asfortranarray(r).reshape(shape) if len(shape) == 1 else np.asfortranarray(r) for r in res)


def gibbs_prep_host(n_per_snp, m_total, p, h2):
    """What `prep_columns` writes for LDpred2's ``(p, h2)`` (sigma_epsilon = 1, lambda = 0, tau_beta = m p / h2), float32:
    ``(mu_mult, half_var_tau, u_logs)`` = ``(C2, 1 / (2 C4), logit(p) - 0.5 log(1 + C1))``."""
    n = np.asarray(n_per_snp, dtype=_F64)
    tau = float(m_total) * float(p) / float(h2)
    vt = n + tau
    logit = np.log(p) - np.log1p(-p) if p < 1.0 else np.inf
    return (n / vt).astype(_F32), (0.5 * vt).astype(_F32), (logit + 0.5 * (np.log(tau) - np.log(vt))).astype(_F32)


def gibbs_prep_rows(cols, m_total, p, h2):
    """The rows of `DeviceState.prep_columns` for chains `cols` with proportions `p` and heritabilities `h2`: (column,
    logit_pi, log_tau_beta, sigma_epsilon = 1, tau_beta = m p / h2, one_plus_lambda = 1)."""
    p, h2 = np.asarray(p, dtype=_F64), np.asarray(h2, dtype=_F64)
    tau = float(m_total) * p / h2
    with np.errstate(divide="ignore"):
        logit = np.where(p < 1.0, np.log(p) - np.log1p(-np.minimum(p, 1.0 - 1e-16)), np.inf)
    return np.stack([np.asarray(cols, dtype=_F64), logit, np.log(tau), np.ones_like(tau), tau, np.ones_like(tau)], axis=1)


def gibbs_route(ld_dtype, dense, ragged, band_ok=True):
    """The route of a Gibbs sweep (`viprs_gibbs_route`): a dict over `viprs_amd._lib.ROUTE_FIELDS`; needs no GPU."""
    from .. import _lib
    return _lib.gibbs_route(ld_dtype, dense, ragged, band_ok)
