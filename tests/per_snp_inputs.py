"""Per-SNP inputs of the sweeps that DIFFER from SNP to SNP -- what tests/test_per_snp_inputs.py (CPU) and
tests/test_gpu_per_snp_inputs.py feed the kernels -- and `first_difference`, which names the SNP where two results part.

Every other generator of the suite (`synthetic.make_inputs`, `make_mixture_inputs`, `make_grid_inputs`, `_mixture_inputs` /
`_grid_inputs` of tests/test_oracle_vs_ref.py, `_inputs` of tests/test_band.py, `gibbs_replay.chain_inputs` as the tests call
it) derives `u_logs`, `sqrt_half_var_tau` / `half_var_tau`, `mu_mult` and `log_null_pi` from `n_per_snp = np.full(m, n)`: one
value per column, repeated along the SNPs.  A kernel that read one of them at the wrong SNP would stay `==` the oracle.
Here the sample size n_j and the prior pi_j are drawn per SNP (real GWAS sample sizes differ from SNP to SNP):

    n_j = 1e5 * 10^U(-1, 0.3)      pi_j = 10^U(-3, -1)      w_j = 10^U(-0.5, 0.5) (mixture / grid: pis_jk = pis_k w_j)

All draws of one `Draws(m, seed)` come from one `np.random.default_rng(seed)` in a fixed order (n, pi, w, then what a model
asks for), are formed in float64 and rounded to the state type last."""
import numpy as np

from viprs_amd.utils import synthetic as syn

# The seed of the draws.  Chosen on the CPU (tests/test_per_snp_inputs.py: test_conditions_on_the_inputs states what it has
# to give on the plan [2370, 1601, 130, 64, 1], longrange LD, seed 53): the first seed counted up from 1 at which no float32
# value of mu_mult, u_logs or sqrt_half_var_tau repeats inside a 64-row panel (seeds 1 .. 9 each repeat a mu_mult, which lies
# in 0.98 .. 0.999 where float32 has few values) and the blocks of 64 and of 130 SNPs each hold a skipped and an unskipped
# SNP in both float32 sweeps (EXPERIMENTS.md 6.31).
SEED = 10
SIGMA_EPS = 0.8
H2 = 0.2
PI = 0.01


class Draws:
    """n_j, pi_j, w_j of `m` SNPs, and the generator they came from (for what a model draws after them)."""

    def __init__(self, m, seed=SEED):
        self.m = int(m)
        self.rng = np.random.default_rng(seed)
        self.n = 1e5 * 10.0 ** self.rng.uniform(-1.0, 0.3, self.m)
        self.pi = 10.0 ** self.rng.uniform(-3.0, -1.0, self.m)
        self.w = 10.0 ** self.rng.uniform(-0.5, 0.5, self.m)


def spike_slab(std_beta, T=np.float32, seed=SEED):
    """`EStepInputs` (what `helpers.run_oracle` / `run_hip` take) for the spike-and-slab model: sigma_eps = 0.8,
    tau = m 0.01 / 0.2, var_tau_j = n_j / sigma_eps + tau; the state of `make_inputs` with var_gamma = pi_j."""
    T = np.dtype(T)
    m = std_beta.shape[0]
    d = Draws(m, seed)
    tau = m * PI / H2
    var_tau = d.n / SIGMA_EPS + tau
    mu_mult = d.n / (var_tau * SIGMA_EPS)
    u_logs = np.log(d.pi) - np.log1p(-d.pi) + 0.5 * (np.log(tau) - np.log(var_tau))
    z = lambda: np.zeros(m, dtype=T)
    return syn.EStepInputs(std_beta=std_beta.astype(T), var_gamma=d.pi.astype(T), var_mu=z(), eta=z(), q=z(), eta_diff=z(),
                           u_logs=u_logs.astype(T), sqrt_half_var_tau=np.sqrt(0.5 * var_tau).astype(T),
                           mu_mult=mu_mult.astype(T), pi=d.pi, sigma_epsilon=SIGMA_EPS, tau_beta=tau)


def mixture(m, K=4, T=np.float32, seed=SEED):
    """(inputs, state) as `_mixture_inputs` of tests/test_oracle_vs_ref.py returns them (C-order (m, K), the keys `_run_mix`
    reads), its per-component d_k, pis_k and tau_k, with n_j per SNP and pis_jk = pis_k w_j: sum_k pis_jk <= 0.01 10^0.5 <
    0.04.  var_gamma starts at pis_jk, var_mu at 0.01 N(0, 1)."""
    T = np.dtype(T)
    dr = Draws(m, seed)
    d = 2.0 ** np.linspace(-min(K - 1, 7), 0, K)
    pis = PI * np.array([0.4, 0.3, 0.2, 0.1])[:K] if K == 4 else np.full(K, PI / K)
    tau = d * (m * pis.sum() / H2)
    pjk = pis[None, :] * dr.w[:, None]
    assert float(pjk.sum(axis=1).max()) < 0.04
    n = dr.n[:, None]
    var_tau = n / SIGMA_EPS + tau[None, :]
    c = lambda a: np.ascontiguousarray(a.astype(T))
    inputs = dict(log_null_pi=np.log(1.0 - pjk.sum(axis=1)).astype(T),
                  u_logs=c(np.log(pjk) - np.log1p(-pjk) + 0.5 * (np.log(tau)[None, :] - np.log(var_tau))),
                  shvt=c(np.sqrt(0.5 * var_tau)), mu_mult=c(n / (var_tau * SIGMA_EPS)))
    st = dict(var_gamma=c(pjk), var_mu=c(0.01 * dr.rng.standard_normal((m, K))), eta=np.zeros(m, T), q=np.zeros(m, T),
              eta_diff=np.zeros(m, T))
    return inputs, st


def grid(m, G=8, T=np.float32, seed=SEED):
    """(inputs, state) as `_grid_inputs` of tests/test_oracle_vs_ref.py returns them (Fortran (m, G), the keys `_run_grid`
    reads), its per-model pis_g, sigma_g and tau_g, with n_j per SNP and pis_jg = pis_g w_j (<= 0.1 10^0.5 < 1).  var_gamma
    starts at pis_jg, everything else at 0."""
    T = np.dtype(T)
    dr = Draws(m, seed)
    pis = np.logspace(-3, -1, G)
    sig = np.linspace(0.7, 0.95, G)
    tau = pis * m / (1 - sig)
    pjg = pis[None, :] * dr.w[:, None]
    n = dr.n[:, None]
    var_tau = n / sig[None, :] + tau[None, :]
    f = lambda a: np.asfortranarray(a.astype(T))
    inputs = dict(u_logs=f(np.log(pjg) - np.log1p(-pjg) + 0.5 * (np.log(tau)[None, :] - np.log(var_tau))),
                  hvt=f(0.5 * var_tau), mu_mult=f(n / (var_tau * sig[None, :])))
    z = lambda: f(np.zeros((m, G)))
    return inputs, dict(var_gamma=f(pjg), var_mu=z(), eta=z(), q=z(), eta_diff=z())


def enet(m, pairs, seed=SEED):
    """(mult, pen) of the elastic-net sweep for the columns `pairs = ((s, lambda), ...)`, float32, Fortran (m, G) ((m,) for
    one column): mult[j, g] = (1 - s_g) U(0.5, 1), pen[j, g] = lambda_g 10^U(-0.5, 0.5)."""
    dr = Draws(m, seed)
    G = len(pairs)
    s = np.array([p[0] for p in pairs], dtype=np.float64)
    lam = np.array([p[1] for p in pairs], dtype=np.float64)
    mult = (1.0 - s)[None, :] * dr.rng.uniform(0.5, 1.0, (m, G))
    pen = lam[None, :] * 10.0 ** dr.rng.uniform(-0.5, 0.5, (m, G))
    shape = (m,) if G == 1 else (m, G)
    f = lambda a: np.asfortranarray(a.astype(np.float32).reshape(shape))
    return f(mult), f(pen)


def gibbs(m, pairs, seed=SEED):
    """`gibbs_replay.chain_inputs` with the n_j above: dict(mu_mult, half_var_tau, u_logs), float32 Fortran (m, G)."""
    from tests import gibbs_replay as GR
    return dict(zip(("mu_mult", "half_var_tau", "u_logs"), GR.chain_inputs(Draws(m, seed).n, pairs)))


def swap_neighbours(a, block_start):
    """A copy of `a` (rows = SNPs) with the neighbours j <-> j ^ 1 exchanged inside every block (j counted from the block's
    first SNP; the last SNP of a block of odd size stays)."""
    out = a.copy(order="K")
    for s, e in zip(block_start[:-1], block_start[1:]):
        s, e = int(s), int(e)
        l = np.arange(e - s)
        p = l ^ 1
        p[p >= e - s] = l[p >= e - s]
        out[s:e] = a[s + p]
    return out


def blocks_changed(a, b, block_start):
    """Per block: does any row of `a` differ from `b`?"""
    rows = (a != b).reshape(a.shape[0], -1).any(axis=1)
    return np.array([rows[int(s):int(e)].any() for s, e in zip(block_start[:-1], block_start[1:])])


def first_difference(got, ref, ld, fields=None):
    """None when `got` and `ref` (dicts of arrays whose rows are the SNPs) agree `==`; otherwise a sentence naming the FIRST
    SNP at which any array differs: the array, the global index (and the column of a 2-D array), the LD block and its size,
    the 64-row panel inside the block and the row inside the panel -- which role of a kernel read or wrote it."""
    fields = list(ref.keys() if fields is None else fields)
    best = None
    counts = {}
    for k in fields:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if g.shape != r.shape or g.dtype != r.dtype:
            return f"{k}: shape / dtype {g.shape} {g.dtype} against {r.shape} {r.dtype}"
        ne = (g != r).reshape(g.shape[0], -1)
        if not ne.any():
            continue
        counts[k] = int(ne.sum())
        j = int(np.argmax(ne.any(axis=1)))
        if best is None or j < best[0]:
            best = (j, k, int(np.argmax(ne[j])), ne.shape[1], g.reshape(ne.shape)[j], r.reshape(ne.shape)[j])
    if best is None:
        return None
    j, k, col, width, g, r = best
    bs = np.asarray(ld.block_start)
    bi = int(np.searchsorted(bs, j, side="right") - 1)
    s, b = int(bs[bi]), int(bs[bi + 1] - bs[bi])
    where = f"{k}[{j}" + (f", {col}]" if width > 1 else "]")
    return (f"first difference at {where}: got {g[col]!r}, expected {r[col]!r}; SNP {j} = row {j - s} of block {bi} "
            f"({b} SNPs, starts at {s}), panel {(j - s) // 64} of {(b + 63) // 64}, row {(j - s) % 64} of the panel; "
            f"entries that differ per array: {counts}")


def assert_equal(got, ref, ld, fields):
    """`==` on every array of `fields`, as `helpers.assert_state_equal`; a failure says where the results part."""
    for k in fields:
        assert np.array_equal(got[k], ref[k]), first_difference(got, ref, ld, fields)
