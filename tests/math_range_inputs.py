"""Inputs that make the ARGUMENT of the device's exp / sigmoid / softmax an input of the sweep -- what
tests/test_math_range_inputs.py (CPU) and tests/test_gpu_math_range.py feed the kernels -- and the long-double references.

Every other float32 test draws its arguments from fit-like data: the sigmoid argument u^2 + ulog lies in about -12 .. +1000,
where the result is 1.0 for x > 17 whatever exp returns and nothing below -16 is ever fed.  Here sqrt_half_var_tau = 0
(spike-and-slab, mixture) or half_var_tau = 0 (grid columns, Gibbs): the argument is fma(0 mu, 0 mu, ulog) = u_logs[j]
exactly, whatever q is, and the list of arguments is chosen:

    float32  c = ln2 / 32: for every k = 0 .. -4802 of glibc's expf reduction k = round(x 32 / ln2) the float32 nearest the
             boundary (k - 1/2) c, its two neighbours and one seeded point inside the interval; the mirror images -x of all
             x > -18; the specials (zeros, denormals, FLT_MIN, ln FLT_MIN, ln 2^-149, glibc's underflow threshold, the clamp
             at -104, -1e3, +-FLT_MAX, +-inf, 88.7, 104), each with its float32 neighbours.  No NaN.
    float64  the same on the 137.6 k intervals of ln2 / 128 over [-745.2, 0]: one interior point per k, the boundary for every
             8th k (its two neighbours for every 64th), |x| < 2^-54, the binade edges at 512, 708.4, 745.13, 1024 and +-inf.

The LD stays the real long-range LD, so q evolves: the serial chain's own gamma reaches the output only through d and q.
Small results are made visible by mu_mult[j] = 2^e_j, e_j = min(cap, floor(-log2 gamma_ref)) (`scales`): every d_j has the
magnitude of std_beta, so the spike-and-slab skip branch (|gamma mu - eta| < eps) passes them and no term swamps another
in q.  In pass p, SNP j takes A[perm[(j + p m) mod N]]."""
import numpy as np

from tests.per_snp_inputs import assert_equal, first_difference  # noqa: F401  (re-used by the tests)
from viprs_amd.utils import synthetic as syn

SEED = 7
VAR_GAMMA0 = 0.01                     # the starting var_gamma of every bundle
LN2 = 0.6931471805599453
C32 = LN2 / 32                        # width of one k-interval of glibc's expf
C64 = LN2 / 128                       # ... of glibc's exp
K32_LAST = -4802                      # -104 32 / ln2 = -4801.3: the clamp lies inside k = -4801
TINY32 = 2.0 ** -149
TINY64 = 2.0 ** -1074
CAP = {np.dtype(np.float32): 126, np.dtype(np.float64): 1000}


def have_long_double():
    """Is np.longdouble an extended format (x87's 64-bit mantissa or better)?"""
    return np.finfo(np.longdouble).eps < 1e-18


def _with_neighbours(values, T):
    v = np.asarray(values, dtype=T)
    with np.errstate(over="ignore"):
        out = np.concatenate([v, np.nextafter(v, T(-np.inf)), np.nextafter(v, T(np.inf))])
    return out[~np.isnan(out)]


def _distinct(a):
    """`a` without repeated bit patterns (+0 and -0 both stay), first occurrences in order."""
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    _, first = np.unique(bits, return_index=True)
    return a[np.sort(first)]


def arguments32():
    """The float32 list (module docstring), about 22.6 k distinct values, deterministic."""
    T = np.float32
    rng = np.random.default_rng(SEED)
    k = np.arange(0, K32_LAST - 1, -1, dtype=np.float64)
    edge = ((k - 0.5) * C32).astype(T)
    inside = ((k - 0.5 + rng.uniform(0.05, 0.95, k.size)) * C32).astype(T)
    body = np.concatenate([edge, np.nextafter(edge, T(-np.inf)), np.nextafter(edge, T(np.inf)), inside])
    mirror = -body[body > -18]
    fi = np.finfo(T)
    special = [0.0, -0.0, TINY32, -TINY32, fi.tiny, -fi.tiny, 1e-30, -1e-30, np.log(float(fi.tiny)), np.log(TINY32),
               float.fromhex("-0x1.9fe368p6"), -104.0, -1e3, -fi.max, -np.inf, 88.7, 104.0, fi.max, np.inf]
    return _distinct(np.concatenate([body, mirror, _with_neighbours(special, T)]).astype(T))


def arguments64():
    """The float64 list (module docstring), about 168 k distinct values."""
    T = np.float64
    rng = np.random.default_rng(SEED + 1)
    k = np.arange(0, -int(745.2 / C64) - 2, -1, dtype=np.float64)
    inside = (k - 0.5 + rng.uniform(0.05, 0.95, k.size)) * C64
    edge = (k[::8] - 0.5) * C64
    body = np.concatenate([inside, edge, np.nextafter(edge[::8], -np.inf), np.nextafter(edge[::8], np.inf)])
    mirror = -body[body > -40]
    fi = np.finfo(T)
    small = [0.0, -0.0, TINY64, -TINY64, fi.tiny, -fi.tiny, 1e-300, -1e-300, 2.0 ** -54, -2.0 ** -54, 2.0 ** -60, -2.0 ** -60]
    edges = [-512.0, -708.4, -745.13, -1024.0, -745.2, -1e6, -fi.max, -np.inf, 512.0, 708.4, 745.13, 1024.0, fi.max, np.inf]
    return _distinct(np.concatenate([body, mirror, _with_neighbours(small + edges, T)]))


def arguments(T):
    return arguments32() if np.dtype(T) == np.float32 else arguments64()


def lane_table_arguments():
    """32 float32 arguments, one per entry of the 32-entry table of expf: x_t = -(t + 1/4) c - 5 has k = -(t + 231)."""
    return (-(np.arange(32) + 0.25) * C32 - 5.0).astype(np.float32)


def reduction_k32(x):
    """k of glibc's expf reduction as the device evaluates it for the sigmoid: round(-|x| 32 / ln2), clamped at -104."""
    xd = np.maximum(-np.abs(np.asarray(x, dtype=np.float32)), np.float32(-104)).astype(np.float64)
    return np.rint(float.fromhex("0x1.71547652b82fep+0") * 32 * xd).astype(np.int64)


# ---- dealing --------------------------------------------------------------------------------------------------------------------
def n_passes(n_args, per_pass):
    return -(-int(n_args) // int(per_pass))


def deal(A, count, p, seed=SEED):
    """`count` entries of pass `p`: entry i takes A[perm[(i + p count) mod N]] (the last pass wraps round)."""
    perm = np.random.default_rng(seed + 2).permutation(A.size)
    return A[perm[(np.arange(count) + p * count) % A.size]]


def deal_lane_table(m, p):
    """Pass p of 32: SNP j takes table entry t = (j + p) mod 32."""
    return lane_table_arguments()[(np.arange(m) + p) % 32]


def scales(gamma_ref, T):
    """mu_mult = 2^e, e = min(cap, floor(-log2 gamma_ref)): gamma mu_mult lies in [1, 2) wherever the cap allows."""
    T = np.dtype(T)
    g = np.asarray(gamma_ref, dtype=np.longdouble)
    with np.errstate(divide="ignore"):
        e = np.where(g > 0, np.floor(-np.log2(np.where(g > 0, g, 1))), CAP[T])
    return np.ldexp(1.0, np.clip(e, 0, CAP[T]).astype(np.int64)).astype(T)


# ---- long-double references -----------------------------------------------------------------------------------------------------
def sigmoid_ref(x):
    """sigmoid of the float32 / float64 values `x` in long double."""
    xl = np.asarray(x).astype(np.longdouble)
    e = np.exp(-np.abs(xl))
    return np.where(xl < 0, e, np.longdouble(1)) / (1 + e)


def softmax_ref(u):
    """softmax over the last axis of `u` ((m, K + 1), the null slot last) with the reference's operations: the maximum and
    u - max in the type of `u` (the rounded difference IS the argument), exp, the sum in slot order and the divide in long
    double.  Returns (the K + 1 results, the arguments u - max)."""
    u = np.asarray(u)
    with np.errstate(invalid="ignore"):
        arg = u - u.max(axis=1, keepdims=True)
    e = np.exp(arg.astype(np.longdouble))
    s = np.zeros(u.shape[0], dtype=np.longdouble)
    for i in range(u.shape[1]):
        s = s + e[:, i]
    return e / s[:, None], arg


def unit(ref, T):
    """max(eps ref, the smallest denormal) of the state type: what the bounds are counted in."""
    T = np.dtype(T)
    return np.maximum(np.finfo(T).eps * np.asarray(ref, dtype=np.longdouble), TINY32 if T == np.float32 else TINY64)


def distance(got, ref, T):
    """|got - ref| in `unit`s."""
    return np.abs(np.asarray(got).astype(np.longdouble) - ref) / unit(ref, T)


# ---- bundles --------------------------------------------------------------------------------------------------------------------
def spike_slab(std_beta, args):
    """`EStepInputs` whose sigmoid argument is `args[j]`: sqrt_half_var_tau = 0, mu_mult = scales(sigmoid(args))."""
    T = std_beta.dtype
    m = std_beta.shape[0]
    args = np.asarray(args, dtype=T)
    z = lambda: np.zeros(m, dtype=T)
    return syn.EStepInputs(std_beta=std_beta.copy(), var_gamma=np.full(m, VAR_GAMMA0, dtype=T), var_mu=z(), eta=z(), q=z(),
                           eta_diff=z(), u_logs=args.copy(), sqrt_half_var_tau=z(), mu_mult=scales(sigmoid_ref(args), T),
                           pi=VAR_GAMMA0, sigma_epsilon=1.0, tau_beta=1.0)


def grid(args):
    """(inputs, state) as `per_snp_inputs.grid` returns them for the (m, G) arguments `args`: half_var_tau = 0."""
    T = args.dtype
    f = lambda a: np.asfortranarray(np.asarray(a, dtype=T))
    z = lambda: f(np.zeros(args.shape))
    inputs = dict(u_logs=f(args), hvt=z(), mu_mult=f(scales(sigmoid_ref(args), T)))
    return inputs, dict(var_gamma=f(np.full(args.shape, VAR_GAMMA0)), var_mu=z(), eta=z(), q=z(), eta_diff=z())


def grid_args(A, m, G, p):
    """Column g of pass p takes its own rotation of the list: deal number p G + g."""
    return np.asfortranarray(np.stack([deal(A, m, p * G + g) for g in range(G)], axis=1))


def mixture(A, m, K, p, seed=SEED):
    """(inputs, state, gamma_ref, arg) as `per_snp_inputs.mixture` returns the first two, pass `p`.  The slot that holds the
    maximum rotates with j over the K components and the null (slot K = log_null_pi).  On even j the maximum is 0 and the
    other slots hold entries a <= 0 of `A` themselves; on odd j the maximum is a seeded value in [-30, 30] and the other
    slots hold fl(max + a), so the subtraction rounds.  gamma_ref (m, K + 1) is `softmax_ref` of the slots, arg its
    arguments; mu_mult[j, k] = scales(gamma_ref[j, k]) / 2^ceil(log2 K): sum_k gamma_k mu_mult_k stays below 2 (the K terms
    of d each have the magnitude of std_beta / K; with a sum of 2 or more the sweep over-relaxes and q diverges along a block)."""
    T = A.dtype
    neg = A[(A <= 0)]
    a = deal(neg, m * (K + 1), p, seed).reshape(m, K + 1)
    j = np.arange(m)
    mx = np.where(j % 2 == 0, 0.0, np.random.default_rng(seed + 3 + p).uniform(-30, 30, m)).astype(T)
    u = (mx[:, None] + a).astype(T)
    u[j, j % (K + 1)] = mx
    return mixture_from_slots(u)


def mixture_from_slots(u):
    """(inputs, state, gamma_ref, arg) for the (m, K + 1) softmax slots `u` (slot K = log_null_pi)."""
    T = u.dtype
    m, K = u.shape[0], u.shape[1] - 1
    gamma_ref, arg = softmax_ref(u)
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=T))
    inputs = dict(log_null_pi=c(u[:, K]), u_logs=c(u[:, :K]), shvt=c(np.zeros((m, K))),
                  mu_mult=c(scales(gamma_ref[:, :K], T) / 2.0 ** int(np.ceil(np.log2(K)))))
    st = dict(var_gamma=c(np.full((m, K), VAR_GAMMA0)), var_mu=c(np.zeros((m, K))), eta=np.zeros(m, T), q=np.zeros(m, T),
              eta_diff=np.zeros(m, T))
    return inputs, st, gamma_ref, arg


def mixture_lane_table(m, K, p):
    """Pass p of 32 for a mixture: component k of SNP j takes table entry (j + p + k) mod 32, the null slot holds the
    maximum 0, so the softmax arguments are the lane-table arguments themselves."""
    x = lane_table_arguments()
    u = np.zeros((m, K + 1), dtype=np.float32)
    for k in range(K):
        u[:, k] = x[(np.arange(m) + p + k) % 32]
    return mixture_from_slots(u)


def block_problem(ld, bi):
    """The LD of block `bi` alone (a `SyntheticLD` of one block) and its SNP range."""
    s, e = int(ld.block_start[bi]), int(ld.block_start[bi + 1])
    lo, hi = int(ld.ld_indptr[s]), int(ld.ld_indptr[e])
    sub = syn.SyntheticLD(ld.ld_left_bound[s:e] - s, ld.ld_indptr[s:e + 1] - lo, ld.ld_data[lo:hi], np.array([0, e - s]),
                          np.zeros(1), ld.low_memory, ld.dq_scale)
    return sub, s, e


def with_singletons(ld, n):
    """`ld` with `n` blocks of one SNP appended (symmetric form: the diagonal entry; upper form: an empty row): where the
    bulk of a long list goes, beside the blocks with real LD."""
    m = ld.m
    j = np.arange(m, m + n)
    one = 1 if ld.dq_scale == 1.0 else int(round(1.0 / ld.dq_scale))
    if ld.low_memory:
        lb, rows, data = j + 1, np.zeros(n, dtype=np.int64), ld.ld_data
    else:
        lb, rows, data = j, np.ones(n, dtype=np.int64), np.concatenate([ld.ld_data, np.full(n, one, ld.ld_data.dtype)])
    indptr = np.concatenate([ld.ld_indptr, ld.ld_indptr[-1] + np.cumsum(rows)]).astype(ld.ld_indptr.dtype)
    return syn.SyntheticLD(np.concatenate([ld.ld_left_bound, lb.astype(np.int32)]), indptr, data,
                           np.concatenate([ld.block_start, j + 1]), np.concatenate([ld.rho, np.zeros(n)]), ld.low_memory,
                           ld.dq_scale)
