"""The SBayesR Gibbs sweep on the host: the definition `viprs_state_bayesr_sweep` / `viprs_state_bayesr_draws` /
`viprs_state_bayesr_sums` are pinned to, the CPU fallback, and the hyper-parameter draws of `viprs_amd.model.SBayesR`.

SBayesR (Lloyd-Jones et al. 2019) draws every effect from its conditional posterior under a finite mixture of normals with a
point mass at zero -- component k = 1..K with prior variance ``gamma_k sigma2_beta`` and weight ``pi_k``, the null with weight
``pi_0`` -- SNP after SNP over each LD block with a running ``q = (R - I) beta``.  With ``lambda = 0``, ``tau_beta[k] = 1 /
(gamma_k sigma2_beta)``, ``sigma_epsilon = sigma2_e``, ``logit_pi[k] = log pi_k`` and ``log_null_pi = log pi_0`` its update is
the mixture E-step (`prep_mixture` writes ``mu_mult``, ``sqrt_half_var_tau``, ``u_logs`` and ``log_null_pi``;
`bayesr_prep_host` is the same on the host) with a draw where the E-step stores ``sum_k gamma_k mu_k``.  One sweep, per SNP j
in index order, every operation separately rounded in float32, fma only where written (include/viprs_hip.h states it with
the device call):

    r = beta_hat_j - q_j
    mu_k = mu_mult_jk r;  t_k = sqrt_half_var_tau_jk mu_k;  u_k = fma(t_k, t_k, u_logs_jk)                   k = 1..K
    mx = max(log_null_pi_j, u_1, .., u_K)
    e_k = expf(u_k - mx);  ssum = ((0 + e_1) + .. + e_K) + expf(log_null_pi_j - mx)                      the null term last
    gamma_k = e_k / ssum
    sd_k = float32(1 / sqrt 2) / sqrt_half_var_tau_jk;  n_k = z_j sd_k
    c_1 = gamma_1;  c_k = c_{k-1} + gamma_k
    k* = the smallest k in 1..K with U_j < c_k, 0 if there is none
    b = k* ? mu_{k*} + n_{k*} : +0;  d = b - eta_j
    var_mu[j, k] = mu_k;  var_gamma[j, k] = gamma_k;  eta_diff[j] = d;  eta[j] = b;  kstar[j] = k*
    q[i] = fma(R[j, i], dq_scale d, q[i]) over the row's window in index order         (symmetric form: then q[j] -= d)

and, upper form, after the last SNP ``q[j] += dq_scale dot(row(j), eta_diff)`` with the dot a serial fma chain from 0.  `expf`
is the C library's, called through ctypes (NumPy's float32 `exp` is another function).

The draws: one Philox4x32-10 block per SNP j with key = the two halves of the seed and counter = (j, 2^30, the two halves of
draw_index) -- the tag 2^30 in the second word keeps the stream apart from the LDpred2 draws (a column there) and the PRS-CS
variates (bit 31 there) --; ``U = (2 (x0 >> 9) + 1) 2^-24`` and ``u1``, ``u2`` likewise from ``x1``, ``x2``;
``z = sqrt(-2 log u1) cos(2 pi u2)``, here in float64 and rounded to float32, on the device in float32 with its `logf` and
`cospif`: `U` is the device's bit for bit, `z` is not.

The hyper-parameter draws (`draw_pi`, `draw_sigma2_beta`, `draw_sigma2_e`) are GCTB's conditionals on the standardised scale;
``sigma2_e`` is floored at `SIGMA2_E_MIN` = 1e-6.
"""
import numpy as np

from .enet import _ordered, fma32
from .gibbs import _expf, _open_unit, philox4x32_10

_F32, _F64, _U64 = np.float32, np.float64, np.uint64
STREAM_TAG = 1 << 30
INV_SQRT2_F32 = _F32(float.fromhex("0x1.6a09e6p-1"))
MAX_K = 4
DEFAULT_GAMMA = (0.01, 0.1, 1.0)
DEFAULT_PI = (0.95, 0.02, 0.02, 0.01)            # the null first
NU = 4.0
SIGMA2_E_MIN = 1e-6


def bayesr_words_host(seed, draw_index, m):
    """The Philox output blocks of SNPs ``0 .. m - 1``: uint32 ``(m, 4)``."""
    seed, draw_index = int(seed) & (2 ** 64 - 1), int(draw_index) & (2 ** 64 - 1)
    ctr = np.empty((int(m), 4), dtype=_U64)
    ctr[:, 0] = np.arange(int(m), dtype=_U64) & _U64(0xFFFFFFFF)
    ctr[:, 1] = STREAM_TAG
    ctr[:, 2] = draw_index & 0xFFFFFFFF
    ctr[:, 3] = draw_index >> 32
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=_U64))


def bayesr_draws_host(seed, draw_index, m):
    """`viprs_state_bayesr_draws` on the host: ``(U, z)``, float32 ``(m,)``; the normals are formed in float64 and rounded."""
    w = bayesr_words_host(seed, draw_index, m)
    u1 = _open_unit(w[:, 1]).astype(_F64)
    u2 = _open_unit(w[:, 2]).astype(_F64)
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return _open_unit(w[:, 0]), z.astype(_F32)


def bayesr_prep_host(n_per_snp, pi, gamma, sigma2_beta, sigma2_e):
    """What `prep_mixture` writes for SBayesR's parameters (`pi`: K + 1 weights, the null first; lambda = 0), float32:
    ``(mu_mult, sqrt_half_var_tau, u_logs)`` of shape ``(m, K)`` and ``log_null_pi`` of shape ``(m,)``."""
    n = np.asarray(n_per_snp, dtype=_F64)[:, None]
    pi = np.asarray(pi, dtype=_F64)
    tau = 1.0 / (np.asarray(gamma, dtype=_F64) * float(sigma2_beta))[None, :]
    vt = n / float(sigma2_e) + tau
    with np.errstate(divide="ignore"):
        ulog = np.log(pi[1:])[None, :] + 0.5 * (np.log(tau) - np.log(vt))
        lnp = np.full(n.shape[0], np.log(pi[0]))
    return ((n / (vt * float(sigma2_e))).astype(_F32), np.sqrt(0.5 * vt).astype(_F32), ulog.astype(_F32), lnp.astype(_F32))


def bayesr_prep_args(pi, gamma, sigma2_beta, sigma2_e):
    """The arguments of `DeviceState.prep_mixture` for the same: (logit_pi, log_tau_beta, tau_beta, log_null_pi, sigma_epsilon,
    one_plus_lambda)."""
    pi = np.asarray(pi, dtype=_F64)
    tau = 1.0 / (np.asarray(gamma, dtype=_F64) * float(sigma2_beta))
    with np.errstate(divide="ignore"):
        return np.log(pi[1:]), np.log(tau), tau, float(np.log(pi[0])), float(sigma2_e), 1.0


def _exp32(x):
    return _F32(_expf()(float(x)))


def bayesr_snp_host(beta, q, mm, sv, ulog, lnp, unif, z, eta_old):
    """The update of one SNP (module docstring) from float32 scalars and ``(K,)`` float32 arrays: ``(mu, gamma, kstar, b, d)``."""
    K = mm.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = _F32(beta) - _F32(q)
        mu = (mm * r).astype(_F32)
        t = (sv * mu).astype(_F32)
        u = fma32(t, t, ulog)
        mx = _F32(lnp)
        for k in range(K):
            mx = np.fmax(mx, u[k])                      # (fmaxf: a NaN operand loses)
        e = np.array([_exp32(u[k] - mx) for k in range(K)], dtype=_F32)
        ssum = _F32(0.0)
        for k in range(K):
            ssum = _F32(ssum + e[k])
        ssum = _F32(ssum + _exp32(_F32(lnp) - mx))
        gam = (e / ssum).astype(_F32)
        sd = (INV_SQRT2_F32 / sv).astype(_F32)
        nz = (_F32(z) * sd).astype(_F32)
        c, kstar, b = _F32(0.0), 0, _F32(0.0)
        for k in range(K):
            c = gam[k] if k == 0 else _F32(c + gam[k])
            if kstar == 0 and _F32(unif) < c:
                kstar, b = k + 1, _F32(mu[k] + nz[k])
        d = _F32(b - _F32(eta_old))
    return mu, gam, kstar, b, d


def bayesr_sweep_host(lb, ip, data, low_memory, std_beta, mu_mult, sqrt_half_var_tau, u_logs, log_null_pi, unif, z, eta, q,
                      dq_scale=1.0):
    """One SBayesR sweep (module docstring) over LD in the layout of `LDPlan` with the given draws: `mu_mult`,
    `sqrt_half_var_tau`, `u_logs` float32 ``(m, K)``, the rest float32 ``(m,)``.  `eta` and `q` are updated IN PLACE; returns
    ``(eta_diff, var_mu, var_gamma, kstar)``."""
    lb = np.asarray(lb, dtype=np.int64)
    ip = np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    x = np.asarray(data).astype(_F32)
    mm, sv, ul = (np.asarray(a) for a in (mu_mult, sqrt_half_var_tau, u_logs))
    K = mm.shape[1] if mm.ndim == 2 else -1
    if not 1 <= K <= MAX_K:
        raise ValueError(f"mu_mult: a float32 array of shape (m, K) with 1 <= K <= {MAX_K}")
    for a, name, shape in ((mm, "mu_mult", (m, K)), (sv, "sqrt_half_var_tau", (m, K)), (ul, "u_logs", (m, K)),
                           (std_beta, "std_beta", (m,)), (log_null_pi, "log_null_pi", (m,)), (unif, "unif", (m,)), (z, "z", (m,)),
                           (eta, "eta", (m,)), (q, "q", (m,))):
        a = np.asarray(a)
        if a.dtype != _F32 or a.shape != shape:
            raise ValueError(f"{name}: a float32 array of shape {shape}")
    dq = _F32(dq_scale)
    ed = np.zeros(m, dtype=_F32)
    mu_out, gam_out = np.zeros((m, K), dtype=_F32), np.zeros((m, K), dtype=_F32)
    kstar = np.zeros(m, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            mu, gam, ks, b, d = bayesr_snp_host(std_beta[j], q[j], mm[j], sv[j], ul[j], log_null_pi[j], unif[j], z[j], eta[j])
            mu_out[j], gam_out[j], kstar[j], ed[j] = mu, gam, ks, d
            s, e = ip[j], ip[j + 1]
            if e > s:
                k = lb[j]
                q[k:k + e - s] = fma32(x[s:e], _F32(dq * d), q[k:k + e - s])
            if not low_memory:
                q[j] = q[j] - d
            eta[j] = b
        if low_memory:
            length = (ip[1:] - ip[:-1]).astype(np.int64)
            acc = np.zeros(m, dtype=_F32)
            rows = np.flatnonzero(length > 0)
            i = 0
            while rows.shape[0]:
                acc[rows] = fma32(x[ip[rows] + i], ed[lb[rows] + i], acc[rows])
                i += 1
                rows = rows[length[rows] > i]
            q += dq * acc
    return ed, mu_out, gam_out, kstar


def bayesr_sums_host(kstar, eta, q, std_beta, K):
    """`viprs_state_bayesr_sums` on the host, ``2 K + 4`` float64: the number of SNPs with k* = 0 .. K, sum eta^2 over
    k* = k for k = 1 .. K, sum q eta, sum eta^2, sum std_beta eta -- every term formed in float64 from the float32 values and
    summed in the order of the device reduction (1024 workgroups at most)."""
    ks = np.asarray(kstar)
    e = np.asarray(eta, dtype=_F32).astype(_F64)
    qq = np.asarray(q, dtype=_F32).astype(_F64)
    b = np.asarray(std_beta, dtype=_F32).astype(_F64)
    out = [_ordered((ks == k).astype(_F64), 1024, False) for k in range(K + 1)]
    out += [_ordered(np.where(ks == k, e * e, 0.0), 1024, False) for k in range(1, K + 1)]
    out += [_ordered(qq * e, 1024, False), _ordered(e * e, 1024, False), _ordered(b * e, 1024, False)]
    return np.array(out, dtype=_F64)


def bayesr_accumulate_host(var_gamma, var_mu, mean_sum, pip_sum):
    """`viprs_state_bayesr_accumulate` on the host: the two ``(m,)`` float64 accumulators updated in place."""
    g = np.asarray(var_gamma, dtype=_F32).astype(_F64)
    mu = np.asarray(var_mu, dtype=_F32).astype(_F64)
    s, p = np.zeros(g.shape[0]), np.zeros(g.shape[0])
    for k in range(g.shape[1]):
        s = s + g[:, k] * mu[:, k]
        p = p + g[:, k]
    mean_sum += s
    pip_sum += p


# ---- the hyper-parameter draws of the sampler (host, float64) -------------------------------------------------------------------
def initial_sigma2_beta(h2, m, pi, gamma):
    """``h2 / (m sum_k pi_k gamma_k)``: the common variance under which the prior's expected ``sum beta^2`` is `h2`."""
    pi, gamma = np.asarray(pi, dtype=_F64), np.asarray(gamma, dtype=_F64)
    return float(h2) / (float(m) * float(pi[1:] @ gamma))


def draw_pi(rng, counts):
    """``pi ~ Dirichlet(counts + 1)``, kept strictly inside the simplex."""
    p = np.maximum(rng.dirichlet(np.asarray(counts, dtype=_F64) + 1.0), 1e-300)
    return p / p.sum()


def draw_sigma2_beta(rng, ssq, gamma, m_nonzero, s2):
    """``(sum_k ssq_k / gamma_k + nu s2) / chi2(nu + m_nonzero)`` with nu = 4."""
    return float((np.asarray(ssq, dtype=_F64) / np.asarray(gamma, dtype=_F64)).sum() + NU * s2) / rng.chisquare(NU + m_nonzero)


def draw_sigma2_e(rng, nbar, sum_beta_eta, sum_eta2, sum_q_eta, s2_e):
    """``(nbar (1 - 2 sum beta_hat eta + sum eta^2 + sum q eta) + nu s2_e) / chi2(nbar + nu)``, floored at `SIGMA2_E_MIN`."""
    sse = nbar * (1.0 - 2.0 * sum_beta_eta + sum_eta2 + sum_q_eta)
    return max(float(sse + NU * s2_e) / rng.chisquare(nbar + NU), SIGMA2_E_MIN)
