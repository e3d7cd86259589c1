"""PRS-CSx on the host: the definition `viprs_csx_update` / `viprs_csx_sums` are pinned to (include/viprs_hip.h states the
operation order with the calls), and the CPU fallback of `viprs_amd.model.PRSCSx`.

PRS-CSx (Ruan et al. 2022) couples one PRS-CS chain per population through ONE local scale per SNP: with ``K`` populations
carrying a SNP, ``psi ~ GIG(1 - K / 2, 2 delta, B)``, ``B = sum_k n_k beta_k^2 / sigma2_k``.  ``K = 1`` is the closed form of
`viprs_amd.stats.cs`; ``K >= 2`` is Devroye's (2014) rejection sampler for the log-concave density of ``log X`` (the algorithm
of PRS-CS's ``gigrnd``), at most `MAX_ATTEMPTS` attempts, each from one Philox block: the integer stream and the open-unit
uniforms are the device's bit for bit, ``exp``, ``log``, ``cosh``, ``sinh`` are NumPy's float64 functions where the device has
its own -- a local scale agrees with the device to one float32 ulp, an attempt count exactly unless an accept decision is
closer than the difference of the two libraries (about 1e-15).
"""
import numpy as np

from .cs import CS_TAG, PSI_MIN, U_LOGS, cs_variates_host
from .enet import _ordered
from .gibbs import _open_unit, philox4x32_10

_F32, _F64, _U64 = np.float32, np.float64, np.uint64
MAX_POP = 8
MAX_ATTEMPTS = 32
N_CSX_SUMS = 2
COSH1, EXP1, EXPM1 = 1.5430806348152437, 2.718281828459045, 0.36787944117144233    # cosh(1), exp(1), exp(-1) in float64


def _psi(x, alpha, lam):
    return -alpha * (np.cosh(x) - 1.0) - lam * (np.exp(x) - x - 1.0)


def _dpsi(x, alpha, lam):
    return -alpha * np.sinh(x) - lam * (np.exp(x) - 1.0)


def csx_attempt_uniforms(seed, draw_index, u, g, attempt):
    """``(U, V, W)``, float32, of attempt `attempt` for the union SNPs `u` (array) of column `g`: the open-unit uniforms of
    the first three words of the Philox block with counter ``(u, g + 2^31 + (attempt + 1) 2^16, draw_index)``."""
    seed, draw_index = int(seed) & (2 ** 64 - 1), int(draw_index) & (2 ** 64 - 1)
    u = np.asarray(u, dtype=np.int64)
    ctr = np.empty(u.shape + (4,), dtype=_U64)
    ctr[..., 0] = u.astype(_U64) & _U64(0xFFFFFFFF)
    ctr[..., 1] = int(g) + CS_TAG + ((int(attempt) + 1) << 16)
    ctr[..., 2] = draw_index & 0xFFFFFFFF
    ctr[..., 3] = draw_index >> 32
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=_U64))
    return tuple(_open_unit(w[..., k]) for k in range(3))


def gig_host(p, a, b, uniforms):
    """Draws of GIG(p, a, b) -- density proportional to ``x^(p - 1) exp(-(a x + b / x) / 2)`` -- for ``p <= 0`` a multiple of
    1/2, ``a > 0``, ``b > 0`` (arrays of one shape, or scalars) by the sampler of include/viprs_hip.h, float64, the device's
    operation order.  `uniforms`: an array ``(attempts, 3)`` + the shape of the draws -- ``U, V, W`` of attempt ``k`` at
    ``[k]`` --, or a callable ``(attempt, index) -> (U, V, W)`` for the flat indices `index` of the draws still rejected.
    Returns ``(x, attempts, capped)``: the draws, the attempts each took (at most `MAX_ATTEMPTS`; a draw still rejected
    at the last one keeps that proposal) and whether it ended at the cap."""
    p, a, b = np.broadcast_arrays(*(np.asarray(v, dtype=_F64) for v in (p, a, b)))
    shape = p.shape
    p, a, b = p.ravel(), a.ravel(), b.ravel()
    if callable(uniforms):
        draw = uniforms
    else:
        un = np.asarray(uniforms).reshape(np.shape(uniforms)[0], 3, -1)
        draw = lambda k, idx: tuple(un[k, c, idx] for c in range(3))
        if un.shape[0] < 1:
            raise ValueError("uniforms: at least one attempt")
    n_att = MAX_ATTEMPTS if callable(uniforms) else min(MAX_ATTEMPTS, un.shape[0])
    with np.errstate(all="ignore"):
        lam = -p                                                    # |p|
        omega = np.sqrt(a * b)
        alpha = np.sqrt(omega * omega + lam * lam) - lam
        x1 = alpha * (COSH1 - 1.0) + lam * (EXP1 - 1.0 - 1.0)       # -psi(1)
        t = np.where(x1 > 2.0, np.sqrt(2.0 / (alpha + lam)), np.where(x1 < 0.5, np.log(4.0 / (alpha + 2.0 * lam)), 1.0))
        x2 = alpha * (COSH1 - 1.0) + lam * EXPM1                    # -psi(-1)
        ia = 1.0 / alpha
        s_log = np.log(1.0 + ia + np.sqrt(ia * ia + 2.0 * ia))
        s_log = np.where(lam > 0.0, np.fmin(1.0 / lam, s_log), s_log)
        s = np.where(x2 > 2.0, np.sqrt(4.0 / (alpha * COSH1 + lam)), np.where(x2 < 0.5, s_log, 1.0))
        eta, zeta = -_psi(t, alpha, lam), -_dpsi(t, alpha, lam)
        theta, xi = -_psi(-s, alpha, lam), _dpsi(-s, alpha, lam)
        pe, re = 1.0 / xi, 1.0 / zeta
        td, sd = t - re * eta, s - pe * theta
        q = td + sd
        norm = pe + q + re
        cut1, cut2 = q / norm, (q + re) / norm
        x = np.zeros(p.shape[0], dtype=_F64)
        attempts = np.zeros(p.shape[0], dtype=np.uint8)
        live = np.arange(p.shape[0])
        for k in range(n_att):
            if live.shape[0] == 0:
                break
            U, V, W = (np.asarray(v, dtype=_F64) for v in draw(k, live))
            i = live
            lv = np.log(V)
            xk = np.where(U < cut1[i], -sd[i] + q[i] * V, np.where(U < cut2[i], td[i] - re[i] * lv, -sd[i] + pe[i] * lv))
            gx = np.where(xk > td[i], np.exp(-eta[i] - zeta[i] * (xk - t[i])),
                          np.where(xk < -sd[i], np.exp(-theta[i] + xi[i] * (xk + s[i])), 1.0))
            ok = W * gx <= np.exp(_psi(xk, alpha[i], lam[i]))
            x[i] = xk
            attempts[i] = k + 1
            live = live[~ok]
        capped = np.zeros(p.shape[0], dtype=bool)
        capped[live] = True
        lo = lam / omega
        out = np.exp(x) * (lo + np.sqrt(1.0 + lo * lo))
        out = np.where(p < 0.0, 1.0 / out, out)
        out = out / np.sqrt(a / b)
    return out.reshape(shape), attempts.reshape(shape), capped.reshape(shape)


def csx_update_host(row_of, n_per_snp, eta, psi, delta, members, params, psi_max=1.0, variates=None, seed=0, draw_index=0,
                    prepare_only=False):
    """`viprs_csx_update` on the host, IN PLACE.  `row_of`: ``(P, m_union)`` int64; `n_per_snp`, `eta`: per population the
    ``(m_k,)`` sample sizes and the float32 ``(m_k, G)`` effects; `psi`, `delta`: the shared float32 ``(m_union, G)`` arrays;
    `members`: per population the float32 ``(m_k, G)`` arrays ``(psi_k, delta_k, mu_mult, half_var_tau, u_logs)`` the update
    scatters into; `params`: rows ``(column, phi, sigma2_0 .. sigma2_{P-1})``; `variates`: ``(ub, z1, z2, e)`` as float32
    ``(m_union, G)`` arrays (None: `viprs_amd.stats.cs.cs_variates_host` of `seed`, `draw_index`; not read with
    `prepare_only`).  The attempts of the sampler are always generated here from (`seed`, `draw_index`).  Returns
    ``(attempts, n_capped)``: the uint8 ``(m_union, G)`` attempt counts (0 where nothing was drawn or listed) and the number
    of draws that ended at the cap."""
    row_of = np.asarray(row_of, dtype=np.int64)
    P, mu = row_of.shape
    if not 1 <= P <= MAX_POP:
        raise ValueError("1..8 populations")
    params = np.asarray(params, dtype=_F64).reshape(-1, 2 + P)
    psi_max = float(psi_max)
    if not (PSI_MIN < psi_max < np.inf):
        raise ValueError("psi_max must lie in (2^-40, inf)")
    cols = params[:, 0].astype(np.int64)
    G = psi.shape[1]
    if np.any(cols != params[:, 0]) or np.any((cols < 0) | (cols >= G)) or np.unique(cols).shape[0] != cols.shape[0]:
        raise ValueError("params: distinct columns of the states")
    if not np.all(np.isfinite(params[:, 1:]) & (params[:, 1:] > 0)):
        raise ValueError("params: phi and sigma2 must be positive and finite")
    if psi.dtype != _F32 or delta.dtype != _F32 or psi.shape != (mu, G) or delta.shape != (mu, G):
        raise ValueError("psi, delta: float32 arrays of shape (m_union, G)")
    carried = row_of >= 0
    K = carried.sum(axis=0)
    if np.any(K == 0):
        raise ValueError("row_of: a union row is carried by no population")
    first = np.argmax(carried, axis=0)
    n = [np.asarray(v, dtype=_F64) for v in n_per_snp]
    attempts = np.zeros((mu, G), dtype=np.uint8, order="F")
    n_capped = 0
    if variates is None and not prepare_only:
        got = cs_variates_host(seed, draw_index, mu, cols)
        variates = [np.zeros((mu, G), dtype=_F32, order="F") for _ in range(4)]
        for dst, src in zip(variates, got):
            dst[:, cols] = src
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for row, g in zip(params, cols):
            phi, sigma2 = row[1], row[2:]
            if not prepare_only:
                ub, z1, z2, e = (np.asarray(v)[:, g].astype(_F64) for v in variates)
                g15 = 0.5 * z2 * z2 + e
                d = g15 / (psi[:, g].astype(_F64) + phi)
                lam = 2.0 * d
                B = np.zeros(mu, dtype=_F64)
                eta1, n1, s1 = np.zeros(mu), np.zeros(mu), np.ones(mu)
                for k in range(P):
                    u = np.flatnonzero(carried[k])
                    r = row_of[k, u]
                    ek = np.asarray(eta[k])[r, g].astype(_F64)
                    B[u] = B[u] + n[k][r] * ek * ek / sigma2[k]
                    f = u[first[u] == k]
                    eta1[f], n1[f], s1[f] = np.asarray(eta[k])[row_of[k, f], g].astype(_F64), n[k][row_of[k, f]], sigma2[k]
                s = np.abs(eta1) * np.sqrt(n1 / (lam * s1))
                y = z1 * z1
                A = s + (y + np.sqrt(y * (4.0 * lam * s + y))) / (2.0 * lam)
                new = np.where(ub * (A + s) <= A, A, s * s / A)
                many = np.flatnonzero(K >= 2)
                zero = many[B[many] == 0.0]
                new[zero] = PSI_MIN
                go = many[~(B[many] == 0.0)]
                if go.shape[0]:
                    x, att, cap = gig_host(1.0 - 0.5 * K[go], lam[go], B[go],
                                           lambda a, idx: csx_attempt_uniforms(seed, draw_index, go[idx], g, a))
                    new[go] = x
                    attempts[go, g] = att
                    n_capped += int(cap.sum())
                new = np.where(new < PSI_MIN, PSI_MIN, new)
                new = np.where(new > psi_max, psi_max, new)
                psi[:, g] = new.astype(_F32)
                delta[:, g] = d.astype(_F32)
            p = psi[:, g].astype(_F64)
            mm = (p / (1.0 + p)).astype(_F32)
            hv = 1.0 + 1.0 / p
            for k in range(P):
                u = np.flatnonzero(carried[k])
                r = row_of[k, u]
                psi_k, delta_k, mu_mult, hvt, u_logs = members[k]
                psi_k[r, g] = psi[u, g]
                delta_k[r, g] = delta[u, g]
                mu_mult[r, g] = mm[u]
                hvt[r, g] = (n[k][r] * hv[u] / (2.0 * sigma2[k])).astype(_F32)
                u_logs[r, g] = U_LOGS
    return attempts, n_capped


def csx_sums_host(psi, delta, cols=None):
    """`viprs_csx_sums` on the host: ``(n, 2)`` float64 -- sum delta, sum psi over the union -- per listed column of the shared
    float32 ``(m_union, G)`` arrays, summed in the order of the device reduction (rows of a grid state)."""
    P, D = (np.asarray(a, dtype=_F32).astype(_F64) for a in (psi, delta))
    cols = range(P.shape[1]) if cols is None else [int(c) for c in np.atleast_1d(cols)]
    out = np.zeros((len(cols), N_CSX_SUMS), dtype=_F64)
    for i, g in enumerate(cols):
        out[i] = (_ordered(D[:, g], 256, False), _ordered(P[:, g], 256, False))
    return out


def gig_moments(p, a, b, n_grid=200001, span=60.0):
    """``(E X, Var X, E 1/X, Var 1/X)`` of GIG(p, a, b) by the trapezoid rule on a log grid of `n_grid` points over
    ``exp(+-span)`` around the mode scale ``sqrt(b / a)`` (the integrand in ``y = log x`` is ``exp(p y - (a e^y + b e^-y) /
    2)``, log-concave and smooth: the rule converges geometrically)."""
    y = np.linspace(-span, span, int(n_grid)) + 0.5 * np.log(b / a)
    with np.errstate(over="ignore", under="ignore"):
        logf = p * y - 0.5 * (a * np.exp(y) + b * np.exp(-y))
        w = np.exp(logf - np.max(logf))
        mom = lambda k: float(np.sum(w * np.exp(np.clip(k * y, -700, 700))) / np.sum(w))
        m1, m2, i1, i2 = mom(1.0), mom(2.0), mom(-1.0), mom(-2.0)
    return m1, m2 - m1 * m1, i1, i2 - i1 * i1
