"""SuSiE fine-mapping on summary statistics (Wang et al. 2020; Zou et al. 2022): what goes with `LDPlan.susie`.

    susie_host       the fit in plain NumPy float64 from the arrays of an `LDPlan` (the CPU fallback; the definition of
                     include/viprs_hip.h, `viprs_plan_susie`, with NumPy's sums and exp: the same model, not the device's bits)
    susie_elbo       the evidence lower bound of a fit, per LD block
    pips             posterior inclusion probabilities
    credible_sets    credible sets with the purity filter

Model, per LD block: ``z ~ N(R b, R)``, ``b = sum_l b_l``, every ``b_l`` a single effect (one non-zero SNP chosen with prior
``pi``, its value ``N(0, V_l)``); `R` has a unit diagonal and off-diagonal entries ``dq_scale * stored``.
"""
import numpy as np

from ..plan import SusieInfo, plan_blocks, susie_inputs

_V_FLOOR = 1e-9                # an effect whose prior variance is at most this has been switched off


def block_starts(lb, ip, low_memory):
    return plan_blocks(np.ascontiguousarray(lb, dtype=np.int32), np.ascontiguousarray(ip), bool(low_memory))[0]


def block_matrix(lb, ip, data, low_memory, s, e, dq_scale=1.0):
    """Dense float64 `R` of the LD block of SNPs s .. e - 1 (unit diagonal; an entry outside a window is 0)."""
    b = e - s
    R = np.zeros((b, b))
    x = np.asarray(data)
    for j in range(s, e):
        n = int(ip[j + 1] - ip[j])
        if n:
            c0 = int(lb[j]) - s
            R[j - s, c0:c0 + n] = x[int(ip[j]):int(ip[j + 1])]
    if low_memory:
        R = np.triu(R, 1)
        R = R + R.T
    R = float(dq_scale) * R
    R[np.arange(b), np.arange(b)] = 1.0
    return R


def _log_prior(log_prior, starts, m):
    if log_prior is not None:
        return log_prior
    lp = np.zeros(m)
    for s, e in zip(starts[:-1], starts[1:]):
        lp[s:e] = -np.log(float(e - s))
    return lp


def _check_values(z, v, v0, lp, starts, L, tol, max_iter, dq_scale):
    """The refusals of the library (include/viprs_hip.h), as ValueError."""
    if not 1 <= L <= 32:
        raise ValueError("L must be in 1..32")
    if not tol > 0.0:
        raise ValueError("tol must be positive")
    if max_iter < 1:
        raise ValueError("max_iter must be at least 1")
    if not (np.isfinite(dq_scale) and dq_scale > 0.0):
        raise ValueError("dq_scale must be finite and positive")
    pv = np.array([v0]) if v is None else v
    if not np.all(np.isfinite(pv)) or np.any(pv < 0.0):
        raise ValueError("prior variance must be finite and >= 0")
    if not np.all(np.isfinite(z)):
        raise ValueError("z must be finite")
    if np.any(np.isnan(lp)) or np.any(lp == np.inf):
        raise ValueError("log_prior must be finite or -inf")
    for s, e in zip(starts[:-1], starts[1:]):
        if not np.any(np.isfinite(lp[s:e])):
            raise ValueError("log_prior is -inf for every SNP of an LD block")


def susie_host(lb, ip, data, low_memory, z, L=10, prior_variance=50.0, estimate_prior_variance=True, log_prior=None,
               dq_scale=1.0, tol=1e-4, max_iter=100, float_precision="float64", callback=None):
    """`LDPlan.susie` on the host: the same arguments behind the arrays of the plan, the same `SusieInfo`.  The arithmetic is
    float64 throughout; `alpha` and `mu` are returned in `float_precision`.  `callback(block, iteration, state)` is called
    after every iteration of every block with ``state = dict(alpha, mu, prior_variance, post_var)`` of that block (views)."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    starts = block_starts(lb, ip, low_memory)
    nb = len(starts) - 1
    L = int(L)
    z, v, v0, lp = susie_inputs(m, nb, z, L, prior_variance, log_prior)
    lp = _log_prior(lp, starts, m)
    _check_values(z, v, v0, lp, starts, L, float(tol), int(max_iter), float(dq_scale))
    V = np.full((nb, L), v0) if v is None else v.copy()
    alpha = np.zeros((m, L), order="F")
    mu = np.zeros((m, L), order="F")
    post_var = np.zeros((nb, L))
    iters = np.zeros(nb, dtype=np.int32)
    delta = np.zeros(nb)
    status = np.zeros(nb, dtype=np.int32)
    for k in range(nb):
        s, e = int(starts[k]), int(starts[k + 1])
        R = block_matrix(lb, ip, data, low_memory, s, e, dq_scale)
        zb, lpb = z[s:e], lp[s:e]
        a, mb = alpha[s:e], mu[s:e]
        Rb = np.zeros((e - s, L))
        st = SusieInfo.MAXITER
        for it in range(1, int(max_iter) + 1):
            d_it = 0.0
            for l in range(L):
                r = zb - Rb[:, np.arange(L) != l].sum(axis=1)
                sl = V[k, l] / (1.0 + V[k, l])
                w = 0.5 * r * r * sl + lpb
                ew = np.exp(w - w.max())
                S = ew.sum()
                mb[:, l] = sl * r
                a_new = ew / S
                d_it = max(d_it, float(np.max(np.abs(a_new - a[:, l]))))
                a[:, l] = a_new
                post_var[k, l] = sl
                if estimate_prior_variance:
                    V[k, l] = float(np.sum(ew * (sl + mb[:, l] ** 2)) / S)
                Rb[:, l] = R @ (a_new * mb[:, l])
            iters[k], delta[k] = it, d_it
            if callback is not None:
                callback(k, it, dict(alpha=a, mu=mb, prior_variance=V[k], post_var=post_var[k]))
            if d_it < tol:
                st = SusieInfo.CONVERGED
                break
        status[k] = st
    dt = np.dtype(float_precision)
    return SusieInfo(np.asfortranarray(alpha.astype(dt)), np.asfortranarray(mu.astype(dt)), V, post_var, iters, delta,
                     status, starts)


def _xlogy(a, b):
    """a log(b) with 0 log 0 = 0."""
    out = np.zeros_like(a)
    nz = a > 0
    out[nz] = a[nz] * np.log(b[nz])
    return out


def elbo_block(R, z, log_pi, alpha, mu, prior_variance, post_var):
    """The bound of one block: ``-0.5 (E[b'Rb] - 2 bbar'z) - sum_l KL_l`` (up to the constant of the likelihood), with
    ``E[b'Rb] = bbar'R bbar + sum_l (sum_j alpha_lj (mu_lj^2 + s_l) - bbar_l'R bbar_l)`` and
    ``KL_l = sum_j alpha_lj (log(alpha_lj / pi_j) + 0.5 (log(V_l / s_l) + (s_l + mu_lj^2) / V_l - 1))``; effects with
    ``V_l = 0`` are omitted (their posterior is their prior and their effect is 0)."""
    alpha, mu = np.asarray(alpha, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    on = np.asarray(prior_variance) > 0.0
    B = (alpha * mu)[:, on]
    bbar = B.sum(axis=1)
    RB = R @ B
    second = 0.0
    kl = 0.0
    for i, l in enumerate(np.nonzero(on)[0]):
        V, s = float(prior_variance[l]), float(post_var[l])
        a, m2 = alpha[:, l], mu[:, l] ** 2
        second += float(np.sum(a * (m2 + s)) - B[:, i] @ RB[:, i])
        with np.errstate(invalid="ignore"):               # (0 * -inf of an excluded SNP: `where` takes the 0)
            kl += float(np.sum(_xlogy(a, a) - np.where(a > 0, a * log_pi, 0.0)))
        kl += float(np.sum(a * 0.5 * (np.log(V / s) + (s + m2) / V - 1.0)))
    ebrb = float(bbar @ (R @ bbar)) + second
    return -0.5 * (ebrb - 2.0 * float(bbar @ z)) - kl


def susie_elbo(lb, ip, data, low_memory, z, info, log_prior=None, dq_scale=1.0):
    """The evidence lower bound of every LD block of a fit (`elbo_block`), float64, ``(n_blocks,)``."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    z = np.asarray(z, dtype=np.float64)
    starts = info.block_start
    lp = _log_prior(None if log_prior is None else np.asarray(log_prior, dtype=np.float64), starts, lb.shape[0])
    out = np.zeros(len(starts) - 1)
    for k in range(len(starts) - 1):
        s, e = int(starts[k]), int(starts[k + 1])
        R = block_matrix(lb, ip, data, low_memory, s, e, dq_scale)
        out[k] = elbo_block(R, z[s:e], lp[s:e], info.alpha[s:e], info.mu[s:e], info.prior_variance[k], info.post_var[k])
    return out


def pips(info):
    """``1 - prod_{l: V_l > 1e-9} (1 - alpha_lj)``, float64 ``(m,)``."""
    alpha = np.asarray(info.alpha, dtype=np.float64)
    out = np.zeros(alpha.shape[0])
    starts = info.block_start
    for k in range(len(starts) - 1):
        s, e = int(starts[k]), int(starts[k + 1])
        on = info.prior_variance[k] > _V_FLOOR
        out[s:e] = 1.0 - np.prod(1.0 - alpha[s:e][:, on], axis=1)
    return out


def ld_entries(lb, ip, data, low_memory, idx, dq_scale=1.0):
    """The square of `R` over the SNPs `idx` (global indices) read from the arrays: unit diagonal, an entry outside a
    window counts as 0."""
    lb, ip = np.asarray(lb), np.asarray(ip, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    n = idx.shape[0]
    a, b = np.meshgrid(idx, idx, indexing="ij")
    if low_memory:
        row, col = np.minimum(a, b), np.maximum(a, b)
        off = col - row - 1
    else:
        row, col = a, b
        off = col - lb[row].astype(np.int64)
    length = ip[row + 1] - ip[row]
    ok = (off >= 0) & (off < length) & (row != col)
    out = np.zeros((n, n))
    x = np.asarray(data)
    out[ok] = float(dq_scale) * x[(ip[row] + off)[ok]].astype(np.float64)
    out[np.arange(n), np.arange(n)] = 1.0
    return out


def credible_sets(info, lb, ip, data, low_memory, dq_scale=1.0, coverage=0.95, min_abs_corr=0.5, n_purity=100, seed=0):
    """The credible sets of a fit.  Per block and effect with ``V_l > 1e-9``: the shortest prefix of the SNPs, sorted by
    descending `alpha` (ties to the lower index), whose `alpha` sums to at least `coverage`; its purity is the smallest
    ``|r|`` over its pairs, read from the arrays (a set larger than `n_purity` is subsampled with `seed`).  Sets below
    `min_abs_corr` are dropped, so are repeats of a set.  Returns a list of dicts: `block`, `effect`, `snps` (indices over
    all SNPs, in the order of the prefix), `coverage` (the sum reached) and `purity`."""
    alpha = np.asarray(info.alpha, dtype=np.float64)
    starts = info.block_start
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    for k in range(len(starts) - 1):
        s, e = int(starts[k]), int(starts[k + 1])
        for l in range(alpha.shape[1]):
            if not info.prior_variance[k, l] > _V_FLOOR:
                continue
            a = alpha[s:e, l]
            order = np.argsort(-a, kind="stable")
            csum = np.cumsum(a[order])
            n = min(int(np.searchsorted(csum, coverage, side="left")) + 1, e - s)
            snps = order[:n] + s
            key = tuple(sorted(snps.tolist()))
            if key in seen:
                continue
            sub = snps if n <= n_purity else np.sort(rng.choice(snps, size=n_purity, replace=False))
            purity = float(np.min(np.abs(ld_entries(lb, ip, data, low_memory, sub, dq_scale))))
            if purity < min_abs_corr:
                continue
            seen.add(key)
            out.append(dict(block=k, effect=l, snps=snps, coverage=float(csum[n - 1]), purity=purity))
    return out
