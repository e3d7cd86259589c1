"""PRS-CS on the host: the definition `viprs_state_cs_variates` / `_update` / `_sums` are pinned to, and the CPU fallback.

PRS-CS (Ge et al. 2019) shrinks every effect by a scale of its own: ``beta_j ~ N(0, sigma2 / n psi_j)``, ``psi_j ~ Gamma(a,
delta_j)``, ``delta_j ~ Gamma(b, phi)``.  Given psi the conditional of one effect is Gaussian -- what the LDpred2 Gibbs sweep
draws from ``mu_mult = psi / (1 + psi)``, ``half_var_tau = n_j (1 + 1 / psi) / (2 sigma2)`` and ``u_logs = 32`` (inclusion
probability exactly 1 in float32) --; given the effects, ``delta_j ~ Gamma(a + b) / (psi_j + phi)`` and ``psi_j ~ GIG(a - 1/2,
2 delta_j, n_j beta_j^2 / sigma2)``.  For the defaults ``a = 1, b = 1/2`` both have closed forms with a fixed number of
variates: ``Gamma(3/2) = z^2 / 2 + Exp(1)``, and the reciprocal of a GIG(1/2) variable is inverse-Gaussian, which Michael,
Schucany and Haas (1976) draw from one normal and one uniform (`gig_half_from_variates`).  Every step is then IEEE float64
arithmetic on given float32 variates: `cs_update_host` fed the device's variates equals the device bit for bit
(include/viprs_hip.h states the operation order with the call).

The variates: one Philox4x32-10 block per (SNP j, column g) with the key of the Gibbs draws and counter ``(j, g + 2^31, the
two halves of draw_index)``; ``ub``, ``u1``, ``u2``, ``u3`` the open-unit uniforms of the four words, ``z1, z2 = sqrt(-2 log
u1) (cos, sin)(2 pi u2)``, ``e = -log u3`` -- here in float64 and rounded to float32, on the device in float32 with its
`logf`, `cospif`, `sinpif`: ``ub`` is the device's bit for bit, the other three are not.
"""
import numpy as np

from .enet import _ordered
from .gibbs import _open_unit, philox4x32_10

_F32, _F64, _U64 = np.float32, np.float64, np.uint64
PSI_MIN = 2.0 ** -40
CS_TAG = 2 ** 31                    # added to the column in the Philox counter: the Gibbs draws use the plain column
U_LOGS = _F32(32.0)                 # sigmoid32(x) == 1 for x >= 32
N_CS_SUMS = 4
VARIATES = ("ub", "z1", "z2", "e")


def cs_words_host(seed, draw_index, m, cols):
    """The Philox output blocks of SNPs ``0 .. m - 1`` for the listed columns: uint32 ``(m, len(cols), 4)``."""
    seed, draw_index = int(seed) & (2 ** 64 - 1), int(draw_index) & (2 ** 64 - 1)
    cols = np.atleast_1d(np.asarray(cols, dtype=np.int64))
    ctr = np.empty((int(m), cols.shape[0], 4), dtype=_U64)
    ctr[..., 0] = np.arange(int(m), dtype=_U64)[:, None] & _U64(0xFFFFFFFF)
    ctr[..., 1] = (cols[None, :] + CS_TAG).astype(_U64)
    ctr[..., 2] = draw_index & 0xFFFFFFFF
    ctr[..., 3] = draw_index >> 32
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=_U64))


def cs_uniforms_host(seed, draw_index, m, cols):
    """``(ub, u1, u2, u3)``, float32 ``(m, len(cols))``: exact, the device's bit for bit."""
    w = cs_words_host(seed, draw_index, m, cols)
    return tuple(_open_unit(w[..., k]) for k in range(4))


def cs_variates_host(seed, draw_index, m, cols):
    """``(ub, z1, z2, e)``, float32 ``(m, len(cols))``: `viprs_state_cs_variates` with the transcendental functions in float64
    and one rounding to float32."""
    ub, u1, u2, u3 = cs_uniforms_host(seed, draw_index, m, cols)
    r = np.sqrt(-2.0 * np.log(u1.astype(_F64)))
    ang = 2.0 * np.pi * u2.astype(_F64)
    return ub, (r * np.cos(ang)).astype(_F32), (r * np.sin(ang)).astype(_F32), (-np.log(u3.astype(_F64))).astype(_F32)


def gig_half_from_variates(a, b, z, u):
    """A draw of GIG(p = 1/2, a, b) -- density proportional to ``x^(-1/2) exp(-(a x + b / x) / 2)``, ``a > 0``, ``b >= 0`` --
    from a standard normal `z` and a uniform `u`: with ``s = sqrt(b / a)`` and ``y = z^2`` the larger root of the
    Michael-Schucany-Haas quadratic is ``A = s + (y + sqrt(y (4 a s + y))) / (2 a)`` (a sum of non-negative terms: no
    cancellation, and ``b = 0`` gives the Gamma(1/2, rate a / 2) draw ``z^2 / a``), the smaller one ``s^2 / A``; the draw is
    ``A`` with probability ``A / (A + s)``.  float64, elementwise; mean ``sqrt(b / a) + 1 / a``.  (In the PRS-CS update ``a``
    is ``lam = 2 delta`` and ``b`` is ``n_j eta^2 / sigma2``.)"""
    a, b, z, u = (np.asarray(v, dtype=_F64) for v in (a, b, z, u))
    s = np.sqrt(b / a)
    y = z * z
    A = s + (y + np.sqrt(y * (4.0 * a * s + y))) / (2.0 * a)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(u * (A + s) <= A, A, s * s / A)


def cs_update_host(n_per_snp, eta, psi, delta, mu_mult, half_var_tau, u_logs, params, psi_max=1.0, variates=None,
                   prepare_only=False):
    """`viprs_state_cs_update` on the host, IN PLACE on the float32 ``(m, G)`` arrays `psi`, `delta`, `mu_mult`,
    `half_var_tau`, `u_logs` for the columns of `params` (rows ``(column, sigma2, phi)``); `variates`: ``(ub, z1, z2, e)`` as
    float32 ``(m, G)`` arrays (not read with `prepare_only`).  float64, the kernel's operation order."""
    n = np.asarray(n_per_snp, dtype=_F64)
    params = np.asarray(params, dtype=_F64).reshape(-1, 3)
    psi_max = float(psi_max)
    if not (PSI_MIN < psi_max < np.inf):
        raise ValueError("psi_max must lie in (2^-40, inf)")
    cols = params[:, 0].astype(np.int64)
    if np.any(cols != params[:, 0]) or np.any((cols < 0) | (cols >= psi.shape[1])) or np.unique(cols).shape[0] != cols.shape[0]:
        raise ValueError("params: distinct columns of the state")
    if not np.all(np.isfinite(params[:, 1:]) & (params[:, 1:] > 0)):
        raise ValueError("params: sigma2 and phi must be positive and finite")
    for arr in (psi, delta, mu_mult, half_var_tau, u_logs):
        if arr.dtype != _F32 or arr.shape != psi.shape:
            raise ValueError("psi, delta, mu_mult, half_var_tau, u_logs: float32 arrays of one shape (m, G)")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for g, sigma2, phi in zip(cols, params[:, 1], params[:, 2]):
            if not prepare_only:
                ub, z1, z2, e = (np.asarray(v)[:, g].astype(_F64) for v in variates)
                g15 = 0.5 * z2 * z2 + e
                d = g15 / (psi[:, g].astype(_F64) + phi)
                lam = 2.0 * d
                s = np.abs(np.asarray(eta)[:, g].astype(_F64)) * np.sqrt(n / (lam * sigma2))
                y = z1 * z1
                A = s + (y + np.sqrt(y * (4.0 * lam * s + y))) / (2.0 * lam)
                new = np.where(ub * (A + s) <= A, A, s * s / A)
                new = np.where(new < PSI_MIN, PSI_MIN, new)
                new = np.where(new > psi_max, psi_max, new)
                psi[:, g] = new.astype(_F32)
                delta[:, g] = d.astype(_F32)
            p = psi[:, g].astype(_F64)
            mu_mult[:, g] = (p / (1.0 + p)).astype(_F32)
            half_var_tau[:, g] = (n * (1.0 + 1.0 / p) / (2.0 * sigma2)).astype(_F32)
            u_logs[:, g] = U_LOGS


def cs_sums_host(n_per_snp, eta, psi, delta, cols=None):
    """`viprs_state_cs_sums` on the host: ``(n, 4)`` float64 -- sum eta^2 / psi, sum n_j eta^2 / psi, sum delta, sum psi -- per
    listed column of the float32 ``(m, G)`` arrays, summed in the order of the device reduction (rows of a grid state)."""
    n = np.asarray(n_per_snp, dtype=_F64)
    E, P, D = (np.asarray(a, dtype=_F32).astype(_F64) for a in (eta, psi, delta))
    cols = range(E.shape[1]) if cols is None else [int(c) for c in np.atleast_1d(cols)]
    out = np.zeros((len(cols), N_CS_SUMS), dtype=_F64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i, g in enumerate(cols):
            t = E[:, g] * E[:, g] / P[:, g]
            out[i] = (_ordered(t, 256, False), _ordered(n * t, 256, False), _ordered(D[:, g], 256, False),
                      _ordered(P[:, g], 256, False))
    return out


def cs_sigma2_draw(rng, nbar, m, sum_beta_eta, quad, weighted_quad):
    """PRS-CS's residual variance: ``1 / Gamma((nbar + m) / 2, scale 1 / err)`` with ``err = max(nbar / 2 (1 - 2 sum
    beta_hat eta + quad), weighted_quad / 2)``, ``quad = eta'R eta + sum eta^2 / psi`` and ``weighted_quad = sum n_j eta^2 /
    psi``.  One draw of `rng`."""
    err = max(0.5 * nbar * (1.0 - 2.0 * sum_beta_eta + quad), 0.5 * weighted_quad)
    return 1.0 / rng.gamma(0.5 * (nbar + m), 1.0 / err)


def cs_phi_draw(rng, m, b, phi, sum_delta):
    """PRS-CS's global scale under the half-Cauchy prior on its root: ``w ~ Gamma(1, scale 1 / (1 + phi))``, then ``phi ~
    Gamma(m b + 1/2, scale 1 / (sum delta + w))``.  Two draws of `rng`."""
    w = rng.gamma(1.0, 1.0 / (1.0 + phi))
    return rng.gamma(m * b + 0.5, 1.0 / (sum_delta + w))
