// C ABI, part 2 (include/viprs_hip.h): the device-resident variational state and the device-side pieces of
// the EM iteration around the E-step (host prep VIPRS.py:400-418, compute_zeta :888-897, the M-step / ELBO
// partial sums :426-581; VIPRSMix.py:169-260).
#include "internal.h"

using namespace viprs;

namespace {

// device-side re-initialisation to the standard start (VIPRS.py:344-358) in ONE launch
template <typename T>
__global__ void reset_state_kernel(T* var_gamma, T* var_mu, int64_t n_wide, T* eta, T* q, T* eta_diff, int64_t n_vec,
                                   T pi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_wide) { var_gamma[i] = pi; var_mu[i] = (T)0; }
    if (i < n_vec) { eta[i] = (T)0; q[i] = (T)0; eta_diff[i] = (T)0; }
}

// ---- the EM iteration around the sweep, as ROWS: a row is one model over a contiguous SNP range [i0, i1) of one column
// (the whole plan: one row over [0, m); a grid column: a row over [0, m) at the column's offset; an SNP group: a row over
// [group_start[g], group_start[g+1]); a grid (group, column) pair: both).  blockIdx.y picks the row -- of a table staged on
// the device, or the single row a one-model call passes as a kernel argument (`rows` == nullptr).  The kernels read the row
// from one place or the other in two branches: a select between the two addresses makes the row's fields per-lane values
// (sums_mixture_kernel: 40 more VGPRs, one wave per SIMD less), a local copy of a mixture row indexed by k goes to scratch.

// prep: VIPRS.py:400-418 on the device (float64, cast to T at the end)
struct PrepRow {
    int64_t i0, i1, off;                           // SNPs [i0, i1) of the column at element offset `off`
    double logit_pi, log_tau_beta, sigma_eps, tau_beta, one_plus_lambda;
};

// spike-and-slab: var_tau stored, sqrt(var_tau / 2) written.  GRID (columns of a grid state): var_tau / 2 written
// (e_step_grid takes it, e_step.hpp:616) and var_tau not stored -- m x G doubles to write here and to read back in the
// sums, which form it again from n_j and the row's scalars, the same expression, the same bits
template <typename T, bool GRID>
__global__ void prep_kernel(const double* __restrict__ n, PrepRow one, const PrepRow* __restrict__ rows,
                            T* __restrict__ mu_mult, T* __restrict__ u_logs, T* __restrict__ shvt,
                            double* __restrict__ var_tau) {
    PrepRow r;
    if (rows) r = rows[blockIdx.y];
    else r = one;
    for (int64_t i = r.i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.i1; i += (int64_t)gridDim.x * blockDim.x) {
        const double vt = n[i] * r.one_plus_lambda / r.sigma_eps + r.tau_beta;
        mu_mult[r.off + i] = (T)(n[i] / (vt * r.sigma_eps));
        u_logs[r.off + i] = (T)(r.logit_pi + 0.5 * (r.log_tau_beta - log(vt)));
        if (GRID) {
            shvt[r.off + i] = (T)(0.5 * vt);
        } else {
            shvt[r.off + i] = (T)sqrt(0.5 * vt);
            var_tau[i] = vt;
        }
    }
}

// ---- mixture (VIPRSMix.py:169-225 prep, :227-260 M-step, elbo) ----
constexpr int kMixResidentK = 8;                                  // = kPanelMaxK: the lane-parallel panel chain
constexpr int kMixSums(int K) { return 7 + 6 * K; }               // s[0..5] | kv[6][K] | max |eta_diff|
struct MixPrepRow {
    int64_t i0, i1;
    double log_null_pi, sigma_eps, one_plus_lambda;
    double logit_pi[kMixResidentK], log_tau[kMixResidentK], tau[kMixResidentK];
};

// per SNP and component (C-order (m, K)): var_tau = n (1 + lambda) / sigma_eps + tau_k and the three E-step inputs
template <typename T>
__device__ __forceinline__ void prep_mixture_body(const double* __restrict__ n, int K, const MixPrepRow& r, T* __restrict__ mu_mult,
                                                  T* __restrict__ u_logs, T* __restrict__ shvt, T* __restrict__ lnp,
                                                  double* __restrict__ var_tau) {
    for (int64_t i = r.i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.i1; i += (int64_t)gridDim.x * blockDim.x) {
        lnp[i] = (T)r.log_null_pi;
        for (int k = 0; k < K; ++k) {
            const double vt = n[i] * r.one_plus_lambda / r.sigma_eps + r.tau[k];
            var_tau[i * K + k] = vt;
            mu_mult[i * K + k] = (T)(n[i] / (vt * r.sigma_eps));
            u_logs[i * K + k] = (T)(r.logit_pi[k] + 0.5 * (r.log_tau[k] - log(vt)));
            shvt[i * K + k] = (T)sqrt(0.5 * vt);
        }
    }
}
template <typename T>
__global__ void prep_mixture_kernel(const double* __restrict__ n, int K, MixPrepRow one, const MixPrepRow* __restrict__ rows,
                                    T* __restrict__ mu_mult, T* __restrict__ u_logs, T* __restrict__ shvt,
                                    T* __restrict__ lnp, double* __restrict__ var_tau) {
    if (rows) prep_mixture_body(n, K, rows[blockIdx.y], mu_mult, u_logs, shvt, lnp, var_tau);
    else prep_mixture_body(n, K, one, mu_mult, u_logs, shvt, lnp, var_tau);
}

// ---- M-step / ELBO sums: stage 1, per-workgroup partials (fixed assignment of elements to threads, fixed tree);
// stage 2 (sums_final_kernel) adds the partials of a row in index order.  The workgroup count of a row fixes its summation
// order: `sums_blocks` for spike-and-slab and mixture rows, `grid_sums_blocks` for grid rows -- the counts a plan that
// holds only the row's SNPs uses, so a group's or pair's sums are bit-identical to those of a plan of its own.
constexpr int kSumsBlock = 256;
constexpr int kNSums = VIPRS_N_SUMS;
__host__ __device__ inline int sums_blocks(int64_t count) {
    const int64_t nb = (count + kSumsBlock - 1) / kSumsBlock;
    return (int)(nb < 1024 ? nb : 1024);
}
__host__ __device__ inline int grid_sums_blocks(int64_t count) {
    const int64_t nb = (count + kSumsBlock - 1) / kSumsBlock;
    return (int)(nb < 256 ? nb : 256);
}

struct SumsRow {
    int64_t i0, i1, off;                           // SNPs [i0, i1) of the column at element offset `off`
    int nb;                                        // workgroups of the row
    int weighted;                                  // d_weight applies to sum [0] (the whole plan / a grid column)
    int form_vt;                                   // grid: var_tau formed from n as the last prep did, from vt[] =
    double vt[3];                                  //   (one_plus_lambda, sigma_eps, tau_beta); otherwise the stored var_tau
    double one_plus_lambda;
};

// `sums_body`: workgroup `bx` of `nb` over SNPs [i0, i1), tree reduction in LDS
template <typename T>
__device__ __forceinline__ void sums_body(int64_t i0, int64_t i1, int nb, int bx, const T* __restrict__ gam,
                                          const T* __restrict__ mu, const T* __restrict__ eta, const T* __restrict__ q,
                                          const T* __restrict__ ed, const T* __restrict__ beta,
                                          const double* __restrict__ var_tau, double one_plus_lambda,
                                          const double* __restrict__ weight, double* __restrict__ out,
                                          const double* __restrict__ n_snp = nullptr, double p_lam1 = 0.0, double p_sig = 1.0,
                                          double p_tau = 0.0) {
    // n_snp != nullptr: var_tau is not stored (grid states) -- formed as the prep kernels form it, n (1 + lambda) / sigma_eps + tau_beta
    __shared__ double red[kNSums][kSumsBlock];
    double acc[kNSums];
#pragma unroll
    for (int k = 0; k < kNSums; ++k) acc[k] = 0.0;
    const double lo = 1e-15, hi = 1.0 - 1e-15;       // np.finfo(float64).resolution (VIPRS.py:509)
    for (int64_t i = i0 + (int64_t)bx * kSumsBlock + threadIdx.x; i < i1; i += (int64_t)nb * kSumsBlock) {
        const double g = (double)gam[i], mud = (double)mu[i];
        const double vt = n_snp ? n_snp[i] * p_lam1 / p_sig + p_tau : var_tau[i];
        const double zeta = g * (mud * mud + 1.0 / vt);                       // VIPRS.py:896
        acc[0] += weight ? g * weight[i] : g;                                  // sum_c mean(gamma_c) over merged chromosomes
        acc[1] += zeta;
        acc[2] += one_plus_lambda * zeta + (double)(q[i] * eta[i]);        // :455 (q*eta in T, as np.multiply)
        acc[3] += (double)beta[i] * (double)eta[i];
        acc[4] += (double)eta[i] * (double)eta[i];
        const double gc = fmin(fmax(g, lo), hi), ng = fmin(fmax(1.0 - g, lo), hi);
        acc[5] += gc * log(gc);
        acc[6] += ng * log(ng);
        acc[7] += gc;
        acc[8] += ng;
        acc[9] += gc * log(vt);
        acc[10] = fmax(acc[10], fabs((double)ed[i]));
    }
#pragma unroll
    for (int k = 0; k < kNSums; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = kSumsBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < kNSums - 1; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
            red[kNSums - 1][threadIdx.x] = fmax(red[kNSums - 1][threadIdx.x], red[kNSums - 1][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x < kNSums) out[threadIdx.x] = red[threadIdx.x][0];
}

// spike-and-slab / grid rows: row y's workgroups write their partials at slots y * gridDim.x + x (the rest of the row leaves)
template <typename T>
__global__ __launch_bounds__(kSumsBlock) void sums_kernel(SumsRow one, const SumsRow* __restrict__ rows,
                                                          const T* __restrict__ gam, const T* __restrict__ mu,
                                                          const T* __restrict__ eta, const T* __restrict__ q,
                                                          const T* __restrict__ ed, const T* __restrict__ beta,
                                                          const double* __restrict__ var_tau, const double* __restrict__ n_snp,
                                                          const double* __restrict__ weight, double* __restrict__ partials) {
    SumsRow r;
    if (rows) r = rows[blockIdx.y];
    else r = one;
    if ((int)blockIdx.x >= r.nb) return;
    sums_body<T>(r.i0, r.i1, r.nb, (int)blockIdx.x, gam + r.off, mu + r.off, eta + r.off, q + r.off, ed + r.off, beta,
                 r.form_vt ? nullptr : var_tau, r.one_plus_lambda, r.weighted ? weight : nullptr,
                 partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kNSums, r.form_vt ? n_snp : nullptr, r.vt[0],
                 r.vt[1], r.vt[2]);
}

// VIPRSMix._partial_sums on the device (float64): per-workgroup partials, fixed order.  `sums_mixture_body`: workgroup `bx`
// of `nb` over SNPs [i0, i1).
template <typename T>
__device__ __forceinline__ void sums_mixture_body(int64_t i0, int64_t i1, int nb, int bx, int K, const T* __restrict__ gam,
                                                  const T* __restrict__ mu, const T* __restrict__ eta,
                                                  const T* __restrict__ q, const T* __restrict__ ed,
                                                  const T* __restrict__ beta, const double* __restrict__ var_tau,
                                                  const double* __restrict__ log_var_tau0, double one_plus_lambda,
                                                  double* __restrict__ partials) {
    constexpr int NMAX = kMixSums(kMixResidentK);
    const int N = kMixSums(K);
    double acc[NMAX];
#pragma unroll
    for (int k = 0; k < NMAX; ++k) acc[k] = 0.0;
    const double lo = 1e-15, hi = 1.0 - 1e-15;
    for (int64_t i = i0 + (int64_t)bx * kSumsBlock + threadIdx.x; i < i1; i += (int64_t)nb * kSumsBlock) {
        double zeta = 0.0, gsum = 0.0;
#pragma unroll
        for (int k = 0; k < kMixResidentK; ++k) {
            if (k < K) {
                const double g = (double)gam[i * K + k], mud = (double)mu[i * K + k], vt = var_tau[i * K + k];
                const double z = g * (mud * mud + 1.0 / vt);
                zeta += z;
                gsum += g;
                const double gc = fmin(fmax(g, lo), hi);
                acc[6 + 0 * kMixResidentK + k] += g;
                acc[6 + 1 * kMixResidentK + k] += z;
                acc[6 + 2 * kMixResidentK + k] += gc * log(gc);
                acc[6 + 3 * kMixResidentK + k] += gc;
                acc[6 + 4 * kMixResidentK + k] += gc * log_var_tau0[i * K + k];
                acc[6 + 5 * kMixResidentK + k] += gc * (mud * mud + 1.0 / vt);
            }
        }
        acc[0] += zeta;
        acc[1] += one_plus_lambda * zeta + (double)(q[i] * eta[i]);
        acc[2] += (double)beta[i] * (double)eta[i];
        acc[3] += (double)eta[i] * (double)eta[i];
        const double ng = fmin(fmax(1.0 - gsum, lo), hi);
        acc[4] += ng * log(ng);
        acc[5] += ng;
        acc[NMAX - 1] = fmax(acc[NMAX - 1], fabs((double)ed[i]));
    }
    // wave shuffle tree, then the 4 waves in order: fixed summation order
    __shared__ double red[NMAX][kSumsBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NMAX; ++k) {
        double a = acc[k];
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(a, off, 64);
            a = (k == NMAX - 1) ? fmax(a, o) : a + o;
        }
        if (lane == 0) red[k][wave] = a;
    }
    __syncthreads();
    // compact to the K actually used: out index n -> internal index
    if ((int)threadIdx.x < N) {
        const int nidx = threadIdx.x;
        int src;
        if (nidx < 6) src = nidx;
        else if (nidx == N - 1) src = NMAX - 1;
        else src = 6 + ((nidx - 6) / K) * kMixResidentK + (nidx - 6) % K;
        double a = red[src][0];
        for (int w = 1; w < kSumsBlock / 64; ++w) a = (src == NMAX - 1) ? fmax(a, red[src][w]) : a + red[src][w];
        partials[nidx] = a;
    }
}

// mixture rows (the stored var_tau, no per-SNP weight): partial slots as in sums_kernel
template <typename T>
__global__ __launch_bounds__(kSumsBlock) void sums_mixture_kernel(int K, SumsRow one, const SumsRow* __restrict__ rows,
                                                                  const T* __restrict__ gam, const T* __restrict__ mu,
                                                                  const T* __restrict__ eta, const T* __restrict__ q,
                                                                  const T* __restrict__ ed, const T* __restrict__ beta,
                                                                  const double* __restrict__ var_tau,
                                                                  const double* __restrict__ log_var_tau0,
                                                                  double* __restrict__ partials) {
    SumsRow r;
    if (rows) r = rows[blockIdx.y];
    else r = one;
    if ((int)blockIdx.x >= r.nb) return;
    sums_mixture_body<T>(r.i0, r.i1, r.nb, (int)blockIdx.x, K, gam, mu, eta, q, ed, beta, var_tau, log_var_tau0,
                         r.one_plus_lambda, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kMixSums(K));
}

// The sums of the elastic-net sweep (viprs_state_enet_sums), fp32 states: the row scheme of sums_kernel -- workgroup `bx` of
// `nb` over SNPs [i0, i1), the same serial order per thread, the same tree -- with the maximum LAST in the partials, where
// sums_final_kernel and the all-rank reduction expect it (the entry point moves it to the front).
constexpr int kNEnetSums = VIPRS_N_ENET_SUMS;
__global__ __launch_bounds__(kSumsBlock) void enet_sums_kernel(SumsRow one, const SumsRow* __restrict__ rows,
                                                               const float* __restrict__ eta, const float* __restrict__ q,
                                                               const float* __restrict__ ed, const float* __restrict__ beta,
                                                               const float* __restrict__ pen, double* __restrict__ partials) {
    SumsRow r;
    if (rows) r = rows[blockIdx.y];
    else r = one;
    if ((int)blockIdx.x >= r.nb) return;
    __shared__ double red[kNEnetSums][kSumsBlock];
    double acc[kNEnetSums];
#pragma unroll
    for (int k = 0; k < kNEnetSums; ++k) acc[k] = 0.0;
    for (int64_t i = r.i0 + (int64_t)blockIdx.x * kSumsBlock + threadIdx.x; i < r.i1; i += (int64_t)r.nb * kSumsBlock) {
        const double e = (double)eta[r.off + i];
        acc[0] += (double)beta[i] * e;
        acc[1] += (double)q[r.off + i] * e;
        acc[2] += e * e;
        acc[3] += (double)pen[r.off + i] * fabs(e);
        acc[4] += e != 0.0 ? 1.0 : 0.0;
        acc[5] = fmax(acc[5], fabs((double)ed[r.off + i]));
    }
#pragma unroll
    for (int k = 0; k < kNEnetSums; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = kSumsBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < kNEnetSums - 1; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
            red[kNEnetSums - 1][threadIdx.x] = fmax(red[kNEnetSums - 1][threadIdx.x], red[kNEnetSums - 1][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x < kNEnetSums)
        partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kNEnetSums + threadIdx.x] = red[threadIdx.x][0];
}

// The sums of PRS-CS (viprs_state_cs_sums), fp32 grid states: the same row scheme once more.  The four sums travel with a
// fifth slot, a maximum over nothing (0), because sums_final_kernel takes the last sum of a row for one.
constexpr int kNCsSums = VIPRS_N_CS_SUMS + 1;
__global__ __launch_bounds__(kSumsBlock) void cs_sums_kernel(SumsRow one, const SumsRow* __restrict__ rows,
                                                             const float* __restrict__ eta, const float* __restrict__ psi,
                                                             const float* __restrict__ delta, const double* __restrict__ n_snp,
                                                             double* __restrict__ partials) {
    SumsRow r;
    if (rows) r = rows[blockIdx.y];
    else r = one;
    if ((int)blockIdx.x >= r.nb) return;
    __shared__ double red[VIPRS_N_CS_SUMS][kSumsBlock];
    double acc[VIPRS_N_CS_SUMS];
#pragma unroll
    for (int k = 0; k < VIPRS_N_CS_SUMS; ++k) acc[k] = 0.0;
    for (int64_t i = r.i0 + (int64_t)blockIdx.x * kSumsBlock + threadIdx.x; i < r.i1; i += (int64_t)r.nb * kSumsBlock) {
        const double e = (double)eta[r.off + i], p = (double)psi[r.off + i];
        const double t = e * e / p;
        acc[0] += t;
        acc[1] += n_snp[i] * t;
        acc[2] += (double)delta[r.off + i];
        acc[3] += p;
    }
#pragma unroll
    for (int k = 0; k < VIPRS_N_CS_SUMS; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = kSumsBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < VIPRS_N_CS_SUMS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < kNCsSums)
        partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kNCsSums + threadIdx.x] =
            threadIdx.x < VIPRS_N_CS_SUMS ? red[threadIdx.x % VIPRS_N_CS_SUMS][0] : 0.0;
}

// stage 2, every family: workgroup (k, y) is one wave adding sum k over the `nb` partials of row y (`stride` slots per row):
// lane l adds the partials of workgroups l, l + 64, ... in order, then a fixed xor-shuffle tree combines the 64 lanes -- a
// deterministic order whatever the timing; the last sum of a row is a maximum
__global__ void sums_final_kernel(const double* __restrict__ partials, int stride, int n_sums, SumsRow one,
                                  const SumsRow* __restrict__ rows, double* __restrict__ out) {
    int nb;
    if (rows) nb = rows[blockIdx.y].nb;
    else nb = one.nb;
    partials += (int64_t)blockIdx.y * stride * n_sums;
    const int k = blockIdx.x, lane = threadIdx.x;
    const bool is_max = (k == n_sums - 1);
    double a = 0.0;
    for (int b = lane; b < nb; b += 64) {
        const double v = partials[(int64_t)b * n_sums + k];
        a = is_max ? fmax(a, v) : a + v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(a, off, 64);
        a = is_max ? fmax(a, o) : a + o;
    }
    if (lane == 0) out[(int64_t)blockIdx.y * n_sums + k] = a;
}

}  // namespace

extern "C" {

// ---- state -------------------------------------------------------------------------------------
int viprs_state_create(viprs_state** out, viprs_plan* plan, int float_dtype, int model_kind, int width) {
    if (!out || !plan) return fail(VIPRS_EINVAL, "null argument");
    *out = nullptr;
    if (float_size(float_dtype) == 0) return fail(VIPRS_EINVAL, "bad float dtype code");
    if (model_kind < VIPRS_MODEL_SPIKE_SLAB || model_kind > VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "bad model kind");
    if (model_kind == VIPRS_MODEL_SPIKE_SLAB) width = 1;
    if (width < 1) return fail(VIPRS_EINVAL, "width must be >= 1");
    HIP_TRY(hipSetDevice(plan->device));
    (void)hipGetLastError();                 // (an error left behind by an earlier, unchecked call of this thread is not ours)
    std::unique_ptr<viprs_state> S(new viprs_state());
    S->plan = plan;
    S->device = plan->device;
    S->float_dtype = float_dtype;
    S->model_kind = model_kind;
    S->width = width;
    if (plan->n_granule_rows > 0) {
        HIP_TRY(S->eta_out.alloc(S->field_elems(VIPRS_FIELD_ETA) * float_size(float_dtype)));
        HIP_TRY(S->q_out.alloc(S->field_elems(VIPRS_FIELD_ETA) * float_size(float_dtype)));
    }
    for (int k = 0; k < VIPRS_FIELD_COUNT; ++k) {
        const size_t bytes = S->field_elems(k) * float_size(float_dtype);
        HIP_TRY(S->f[k].alloc(bytes));
        // on the plan's stream (non-blocking: the null stream is NOT ordered with it -- a late null-stream
        // memset would wipe data uploaded in the meantime)
        if (bytes) HIP_TRY(hipMemsetAsync(S->f[k].p, 0, bytes, plan->stream));
    }
    HIP_TRY(hipStreamSynchronize(plan->stream));
    *out = S.release();
    return VIPRS_OK;
}

int viprs_state_destroy(viprs_state* S) {
    if (!S) return VIPRS_OK;
    // (S->device, not S->plan->device: finalizers of a garbage collector run in any order, and a state destroyed after its
    //  plan would read freed memory here -- hipSetDevice(garbage) then leaves "invalid device ordinal" as the thread's last
    //  error, which the next hipGetLastError() behind a kernel launch reports as that launch's failure)
    (void)hipSetDevice(S->device);
    delete S;
    return VIPRS_OK;
}

int viprs_state_upload(viprs_state* S, int field, const void* host) {
    if (!S || field < 0 || field >= VIPRS_FIELD_COUNT) return fail(VIPRS_EINVAL, "bad state/field");
    const size_t bytes = S->field_elems(field) * float_size(S->float_dtype);
    if (bytes == 0) return VIPRS_OK;
    if (!host) return fail(VIPRS_EINVAL, "host buffer is null");
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(hipMemcpyAsync(S->f[field].p, host, bytes, hipMemcpyHostToDevice, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_download(viprs_state* S, int field, void* host) {
    if (!S || field < 0 || field >= VIPRS_FIELD_COUNT) return fail(VIPRS_EINVAL, "bad state/field");
    const size_t bytes = S->field_elems(field) * float_size(S->float_dtype);
    if (bytes == 0) return VIPRS_OK;
    if (!host) return fail(VIPRS_EINVAL, "host buffer is null");
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(hipMemcpyAsync(host, S->f[field].p, bytes, hipMemcpyDeviceToHost, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return check_device_error(S->plan);
}

int viprs_state_reset(viprs_state* S, double pi) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    const int64_t n_wide = (int64_t)S->field_elems(VIPRS_FIELD_VAR_GAMMA);
    const int64_t n_vec = (int64_t)S->field_elems(VIPRS_FIELD_ETA);
    const int64_t n = std::max(n_wide, n_vec);
    if (n == 0) return VIPRS_OK;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (S->float_dtype == VIPRS_F32)
        reset_state_kernel<float><<<grid, 256, 0, P->stream>>>(
            (float*)S->f[VIPRS_FIELD_VAR_GAMMA].p, (float*)S->f[VIPRS_FIELD_VAR_MU].p, n_wide,
            (float*)S->f[VIPRS_FIELD_ETA].p, (float*)S->f[VIPRS_FIELD_Q].p, (float*)S->f[VIPRS_FIELD_ETA_DIFF].p, n_vec,
            (float)pi);
    else
        reset_state_kernel<double><<<grid, 256, 0, P->stream>>>(
            (double*)S->f[VIPRS_FIELD_VAR_GAMMA].p, (double*)S->f[VIPRS_FIELD_VAR_MU].p, n_wide,
            (double*)S->f[VIPRS_FIELD_ETA].p, (double*)S->f[VIPRS_FIELD_Q].p, (double*)S->f[VIPRS_FIELD_ETA_DIFF].p, n_vec,
            pi);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

}  // extern "C"

namespace viprs {
// after a synchronisation point: did a team hand-off give up (bounded spin)?
int check_device_error(viprs_plan* P) {
    int32_t e = 0;
    HIP_TRY(hipMemcpy(&e, P->d_error.p, sizeof(e), hipMemcpyDeviceToHost));
    if (e != 0) {
        HIP_TRY(hipMemsetAsync(P->d_error.p, 0, sizeof(e), P->stream));
        HIP_TRY(hipStreamSynchronize(P->stream));
        return fail(VIPRS_EDEVICE, "E-step kernel: a team hand-off timed out (results of this sweep are invalid)");
    }
    return VIPRS_OK;
}
}  // namespace viprs

// ---- host side of the rows: staging, the launchers, the reduction in flight ----------------------------------------------
// Row tables of the batched calls go through ONE pinned staging area (prep rows, then sums rows) and one H2D copy per call;
// the one-model calls pass their row as a kernel argument.
static size_t prep_row_bytes(const viprs_state* S) {
    return S->model_kind == VIPRS_MODEL_MIXTURE ? sizeof(MixPrepRow) : sizeof(PrepRow);
}
static SumsRow* sums_staging(const viprs_state* S) {
    return reinterpret_cast<SumsRow*>(S->h_rows + S->rows_cap * prep_row_bytes(S));
}

// room for `n` rows (grown to the most a call can list: one per group, or per (group, column) pair / column of a grid state)
static int row_buffers(viprs_state* S, int n) {
    if ((size_t)n <= S->rows_cap) return VIPRS_OK;
    viprs_plan* P = S->plan;
    const size_t cap = std::max<size_t>((size_t)n, (size_t)std::max(1, S->n_groups) *
                                                       (S->model_kind == VIPRS_MODEL_GRID ? S->width : 1));
    HIP_TRY(hipStreamSynchronize(P->stream));                 // nothing in flight reads the old buffers
    HIP_TRY(S->d_prep_rows.alloc(cap * prep_row_bytes(S)));
    HIP_TRY(S->d_sum_rows.alloc(cap * sizeof(SumsRow)));
    if (S->h_rows) HIP_TRY(hipHostFree(S->h_rows));
    S->h_rows = nullptr;
    S->rows_cap = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S->h_rows), cap * (prep_row_bytes(S) + sizeof(SumsRow)),
                          hipHostMallocDefault));
    S->rows_cap = cap;
    return VIPRS_OK;
}

// the pinned staging of a batched prep's `n` rows, free once the previous batched prep launch has read its own
template <typename Row>
static int prep_staging(viprs_state* S, int n, Row** h) {
    const int rc = row_buffers(S, n);
    if (rc != VIPRS_OK) return rc;
    if (!S->ev_prep) HIP_TRY(hipEventCreateWithFlags(&S->ev_prep, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(S->ev_prep));
    *h = reinterpret_cast<Row*>(S->h_rows);
    return VIPRS_OK;
}

// grid of a prep launch: rows along y, the longest row's SNPs along x
template <typename Row>
static dim3 prep_grid(int n, const Row* rows) {
    int64_t longest = 0;
    for (int i = 0; i < n; ++i) longest = std::max(longest, rows[i].i1 - rows[i].i0);
    return dim3((unsigned)std::max<int64_t>(1, (longest + 255) / 256), (unsigned)n);
}

// spike-and-slab / grid prep of `one` (kernel argument) or of the `n` rows in the pinned staging (one H2D copy)
static int prep_launch(viprs_state* S, int n, const PrepRow* one) {
    viprs_plan* P = S->plan;
    const PrepRow* h = one ? one : reinterpret_cast<const PrepRow*>(S->h_rows);
    const PrepRow* rows = one ? nullptr : reinterpret_cast<const PrepRow*>(S->d_prep_rows.p);
    if (!one) HIP_TRY(hipMemcpyAsync(S->d_prep_rows.p, h, n * sizeof(PrepRow), hipMemcpyHostToDevice, P->stream));
    const dim3 grid = prep_grid(n, h);
    const bool g = S->model_kind == VIPRS_MODEL_GRID;
#define VIPRS_PREP_ARGS(T)                                                                                                    \
    S->d_n.p, *h, rows, (T*)S->f[VIPRS_FIELD_MU_MULT].p, (T*)S->f[VIPRS_FIELD_U_LOGS].p,                                     \
        (T*)S->f[VIPRS_FIELD_SQRT_HALF_VAR_TAU].p, S->d_var_tau.p
    if (S->float_dtype == VIPRS_F32 && g) prep_kernel<float, true><<<grid, 256, 0, P->stream>>>(VIPRS_PREP_ARGS(float));
    else if (S->float_dtype == VIPRS_F32) prep_kernel<float, false><<<grid, 256, 0, P->stream>>>(VIPRS_PREP_ARGS(float));
    else if (g) prep_kernel<double, true><<<grid, 256, 0, P->stream>>>(VIPRS_PREP_ARGS(double));
    else prep_kernel<double, false><<<grid, 256, 0, P->stream>>>(VIPRS_PREP_ARGS(double));
#undef VIPRS_PREP_ARGS
    HIP_TRY(hipGetLastError());
    if (!one) HIP_TRY(hipEventRecord(S->ev_prep, P->stream));
    return VIPRS_OK;
}

// the same for a mixture state
static int prep_mixture_launch(viprs_state* S, int n, const MixPrepRow* one) {
    viprs_plan* P = S->plan;
    const int K = S->width;
    if (S->d_var_tau.n < (size_t)P->m * K) {
        HIP_TRY(hipStreamSynchronize(P->stream));
        HIP_TRY(S->d_var_tau.alloc((size_t)P->m * K));
    }
    const MixPrepRow* h = one ? one : reinterpret_cast<const MixPrepRow*>(S->h_rows);
    const MixPrepRow* rows = one ? nullptr : reinterpret_cast<const MixPrepRow*>(S->d_prep_rows.p);
    if (!one) HIP_TRY(hipMemcpyAsync(S->d_prep_rows.p, h, n * sizeof(MixPrepRow), hipMemcpyHostToDevice, P->stream));
    const dim3 grid = prep_grid(n, h);
    if (S->float_dtype == VIPRS_F32)
        prep_mixture_kernel<float><<<grid, 256, 0, P->stream>>>(
            S->d_n.p, K, *h, rows, (float*)S->f[VIPRS_FIELD_MU_MULT].p, (float*)S->f[VIPRS_FIELD_U_LOGS].p,
            (float*)S->f[VIPRS_FIELD_SQRT_HALF_VAR_TAU].p, (float*)S->f[VIPRS_FIELD_LOG_NULL_PI].p, S->d_var_tau.p);
    else
        prep_mixture_kernel<double><<<grid, 256, 0, P->stream>>>(
            S->d_n.p, K, *h, rows, (double*)S->f[VIPRS_FIELD_MU_MULT].p, (double*)S->f[VIPRS_FIELD_U_LOGS].p,
            (double*)S->f[VIPRS_FIELD_SQRT_HALF_VAR_TAU].p, (double*)S->f[VIPRS_FIELD_LOG_NULL_PI].p, S->d_var_tau.p);
    HIP_TRY(hipGetLastError());
    if (!one) HIP_TRY(hipEventRecord(S->ev_prep, P->stream));
    return VIPRS_OK;
}

// one row of sums: SNPs [i0, i1) of column `col`; `vt`: the scalars of the grid column's / pair's last prep (var_tau is
// formed from them, the reduction takes grid_sums_blocks workgroups), nullptr: the stored var_tau, sums_blocks workgroups
static SumsRow sums_row(const viprs_state* S, int64_t i0, int64_t i1, int64_t col, double one_plus_lambda, bool weighted,
                        const double* vt) {
    SumsRow r{};
    r.i0 = i0;
    r.i1 = i1;
    r.off = col * S->plan->m;
    r.nb = vt ? grid_sums_blocks(i1 - i0) : sums_blocks(i1 - i0);
    r.weighted = weighted;
    r.one_plus_lambda = one_plus_lambda;
    if (vt) {
        r.form_vt = 1;
        for (int k = 0; k < 3; ++k) r.vt[k] = vt[k];
    }
    return r;
}

// d_partials, d_sums and the pinned landing buffer h_sums: `total` sums + the plan's device error word (no second
// synchronisation)
static int sums_buffers(viprs_state* S, size_t partials, size_t total) {
    if (S->d_partials.n < partials) HIP_TRY(S->d_partials.alloc(partials));
    if (S->d_sums.n < total) HIP_TRY(S->d_sums.alloc(total));
    if (S->h_sums_cap < total + 1) {
        if (S->h_sums) HIP_TRY(hipHostFree(S->h_sums));
        S->h_sums = nullptr;
        S->h_sums_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S->h_sums), (total + 1) * sizeof(double), hipHostMallocDefault));
        S->h_sums_cap = total + 1;
    }
    return VIPRS_OK;
}

// the first-stage kernel of a reduction (callers that pass a bool mean the first two)
enum { kSumsSpikeSlabOrGrid = 0, kSumsMixture = 1, kSumsElasticNet = 2, kSumsCs = 3 };

// Enqueues the reduction of `one` (kernel argument) or of the `n` rows in the sums staging (one H2D copy), n_sums sums per
// row, by the first-stage kernel `family`, then the all-rank reduction and the asynchronous copy into h_sums; sums_collect waits for it.  A rank whose plan
// holds no SNP contributes zeros to the collective of viprs_state_set_comm.
static int sums_enqueue(viprs_state* S, int family, int n, int n_sums, const SumsRow* one) {
    const bool mixture = family == kSumsMixture;
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    const size_t total = (size_t)n * n_sums;
    const SumsRow* h = one ? one : sums_staging(S);
    int nb = 1;                         // (a row of an empty group has none: its sums are zeros)
    for (int i = 0; P->m > 0 && i < n; ++i) nb = std::max(nb, h[i].nb);
    int rc = sums_buffers(S, (size_t)nb * total, total);
    if (rc != VIPRS_OK) return rc;
    if (P->m == 0) {
        HIP_TRY(hipMemsetAsync(S->d_sums.p, 0, total * sizeof(double), P->stream));
    } else {
        const SumsRow* rows = one ? nullptr : reinterpret_cast<const SumsRow*>(S->d_sum_rows.p);
        if (!one) HIP_TRY(hipMemcpyAsync(S->d_sum_rows.p, h, n * sizeof(SumsRow), hipMemcpyHostToDevice, P->stream));
        const dim3 grid((unsigned)nb, (unsigned)n);
#define VIPRS_SUMS_ARGS(T)                                                                                                     \
    *h, rows, (const T*)S->f[VIPRS_FIELD_VAR_GAMMA].p, (const T*)S->f[VIPRS_FIELD_VAR_MU].p, (const T*)S->f[VIPRS_FIELD_ETA].p, \
        (const T*)S->f[VIPRS_FIELD_Q].p, (const T*)S->f[VIPRS_FIELD_ETA_DIFF].p, (const T*)S->f[VIPRS_FIELD_STD_BETA].p,       \
        S->d_var_tau.p
        if (family == kSumsElasticNet)
            enet_sums_kernel<<<grid, kSumsBlock, 0, P->stream>>>(
                *h, rows, (const float*)S->f[VIPRS_FIELD_ETA].p, (const float*)S->f[VIPRS_FIELD_Q].p,
                (const float*)S->f[VIPRS_FIELD_ETA_DIFF].p, (const float*)S->f[VIPRS_FIELD_STD_BETA].p,
                (const float*)S->f[VIPRS_FIELD_ENET_PENALTY].p, S->d_partials.p);
        else if (family == kSumsCs)
            cs_sums_kernel<<<grid, kSumsBlock, 0, P->stream>>>(
                *h, rows, (const float*)S->f[VIPRS_FIELD_ETA].p, S->d_cs.p + (size_t)VIPRS_CS_PSI * P->m * S->width,
                S->d_cs.p + (size_t)VIPRS_CS_DELTA * P->m * S->width, S->d_n.p, S->d_partials.p);
        else if (mixture && S->float_dtype == VIPRS_F32)
            sums_mixture_kernel<float><<<grid, kSumsBlock, 0, P->stream>>>(S->width, VIPRS_SUMS_ARGS(float), S->d_log_var_tau0.p,
                                                                           S->d_partials.p);
        else if (mixture)
            sums_mixture_kernel<double><<<grid, kSumsBlock, 0, P->stream>>>(S->width, VIPRS_SUMS_ARGS(double),
                                                                            S->d_log_var_tau0.p, S->d_partials.p);
        else if (S->float_dtype == VIPRS_F32)
            sums_kernel<float><<<grid, kSumsBlock, 0, P->stream>>>(VIPRS_SUMS_ARGS(float), S->d_n.p, S->d_weight.p,
                                                                   S->d_partials.p);
        else
            sums_kernel<double><<<grid, kSumsBlock, 0, P->stream>>>(VIPRS_SUMS_ARGS(double), S->d_n.p, S->d_weight.p,
                                                                    S->d_partials.p);
#undef VIPRS_SUMS_ARGS
        HIP_TRY(hipGetLastError());
        sums_final_kernel<<<dim3((unsigned)n_sums, (unsigned)n), 64, 0, P->stream>>>(S->d_partials.p, nb, n_sums, *h, rows,
                                                                                     S->d_sums.p);
        HIP_TRY(hipGetLastError());
    }
    if (S->comm) {                      // all ranks: ONE all-gather + rank-ordered reduction, still on the plan's stream
        rc = comm_reduce_on_stream(S->comm, S->d_sums.p, (int)total, n_sums, P->stream);
        if (rc != VIPRS_OK) return rc;
    }
    // pinned host buffer: the copy is truly asynchronous, several plans' sums overlap
    HIP_TRY(hipMemcpyAsync(S->h_sums, S->d_sums.p, total * sizeof(double), hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipMemcpyAsync(S->h_sums + total, P->d_error.p, sizeof(int32_t), hipMemcpyDeviceToHost, P->stream));
    S->sums_total = total;
    S->sums_pending = true;
    S->sums_empty = false;
    return VIPRS_OK;
}

// a `begin` with nothing to reduce here: an empty rank still takes part in the collective (it contributes zeros),
// otherwise `end` returns zeros
static int sums_nothing(viprs_state* S, bool mixture, int n, int n_sums) {
    if (S->plan->m == 0 && n > 0 && S->comm) return sums_enqueue(S, mixture, n, n_sums, nullptr);
    S->sums_total = (size_t)n * n_sums;
    S->sums_pending = false;
    S->sums_empty = true;
    return VIPRS_OK;
}

// waits for the reduction `begin` enqueued and copies its sums (at most `room` doubles) to `out`
static int sums_collect(viprs_state* S, double* out, const char* begin, size_t room = SIZE_MAX) {
    const size_t n = std::min(S->sums_total, room);
    if (S->sums_empty) {
        for (size_t k = 0; k < n; ++k) out[k] = 0.0;
        return VIPRS_OK;
    }
    if (!S->sums_pending) return fail(VIPRS_EINVAL, std::string("no device sums in flight (") + begin + ")");
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipStreamSynchronize(P->stream));
    S->sums_pending = false;
    for (size_t k = 0; k < n; ++k) out[k] = S->h_sums[k];
    int32_t e = 0;
    memcpy(&e, S->h_sums + S->sums_total, sizeof(e));
    return e != 0 ? check_device_error(P) : VIPRS_OK;       // slow path only when a hand-off timed out
}

extern "C" {

int viprs_state_synchronize(viprs_state* S) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return check_device_error(S->plan);
}

int viprs_state_set_n_per_snp(viprs_state* S, const double* n) {
    if (!S || !n) return fail(VIPRS_EINVAL, "null argument");
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    const size_t m = (size_t)P->m;
    if (m == 0) return VIPRS_OK;
    HIP_TRY(S->d_n.alloc(m));
    HIP_TRY(S->d_var_tau.alloc(m));
    HIP_TRY(hipMemcpyAsync(S->d_n.p, n, m * sizeof(double), hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipMemsetAsync(S->d_var_tau.p, 0, m * sizeof(double), P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    return VIPRS_OK;
}

int viprs_state_set_snp_weights(viprs_state* S, const double* w) {
    if (!S) return fail(VIPRS_EINVAL, "null argument");
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    const size_t m = (size_t)P->m;
    if (!w || m == 0) { HIP_TRY(S->d_weight.alloc(0)); return VIPRS_OK; }
    HIP_TRY(S->d_weight.alloc(m));
    HIP_TRY(hipMemcpyAsync(S->d_weight.p, w, m * sizeof(double), hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    return VIPRS_OK;
}

int viprs_state_prep(viprs_state* S, double logit_pi, double log_tau_beta, double sigma_epsilon, double tau_beta,
                     double one_plus_lambda) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    if (S->model_kind != VIPRS_MODEL_SPIKE_SLAB) return fail(VIPRS_EUNSUPPORTED, "device prep: spike-and-slab only");
    viprs_plan* P = S->plan;
    if (P->m == 0) return VIPRS_OK;
    if (!S->d_n.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp has not been called");
    HIP_TRY(hipSetDevice(P->device));
    const PrepRow r{0, P->m, 0, logit_pi, log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda};
    return prep_launch(S, 1, &r);
}

int viprs_state_sums(viprs_state* S, double one_plus_lambda, double* out) {
    if (!S || !out) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_SPIKE_SLAB) return fail(VIPRS_EUNSUPPORTED, "device sums: spike-and-slab only");
    viprs_plan* P = S->plan;
    for (int k = 0; k < kNSums; ++k) out[k] = 0.0;
    if (P->m == 0 && !S->comm) return VIPRS_OK;
    if (P->m > 0 && !S->d_var_tau.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp / viprs_state_prep have not been called");
    const SumsRow r = sums_row(S, 0, P->m, 0, one_plus_lambda, true, nullptr);
    const int rc = sums_enqueue(S, false, 1, kNSums, &r);
    return rc != VIPRS_OK ? rc : sums_collect(S, out, "viprs_state_sums_begin");
}

int viprs_state_sums_begin(viprs_state* S, double one_plus_lambda) {
    if (!S) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_SPIKE_SLAB) return fail(VIPRS_EUNSUPPORTED, "device sums: spike-and-slab only");
    viprs_plan* P = S->plan;
    if (P->m == 0) return sums_nothing(S, false, 1, kNSums);
    if (!S->d_var_tau.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp / viprs_state_prep have not been called");
    const SumsRow r = sums_row(S, 0, P->m, 0, one_plus_lambda, true, nullptr);
    return sums_enqueue(S, false, 1, kNSums, &r);
}

int viprs_state_sums_end(viprs_state* S, double* out) {
    if (!S || !out) return fail(VIPRS_EINVAL, "null argument");
    return sums_collect(S, out, "viprs_state_sums_begin", kNSums);
}

// ---- grid states: one model per column -------------------------------------------------------------------------------
// (one_plus_lambda, sigma_eps, tau_beta) of a prep, kept for the sums (a grid state keeps no var_tau)
static void record_prep(double* slot, double one_plus_lambda, double sigma_eps, double tau_beta) {
    slot[0] = one_plus_lambda;
    slot[1] = sigma_eps;
    slot[2] = tau_beta;
}
static double* col_last_prep(viprs_state* S, int g) {
    if (S->col_prep.size() != (size_t)3 * S->width) S->col_prep.assign((size_t)3 * S->width, NAN);
    return S->col_prep.data() + 3 * (size_t)g;
}

static int grid_column_check(viprs_state* S, int g) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    if (S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "not a grid state");
    if (g < 0 || g >= S->width) return fail(VIPRS_EINVAL, "model index out of range");
    // (an empty plan has no per-SNP sample sizes to set: a rank without LD blocks passes)
    if (!S->d_n.p && S->plan->m > 0) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp has not been called");
    return VIPRS_OK;
}

int viprs_state_prep_column(viprs_state* S, int g, double logit_pi, double log_tau_beta, double sigma_epsilon,
                            double tau_beta, double one_plus_lambda) {
    int rc = grid_column_check(S, g);
    if (rc != VIPRS_OK) return rc;
    viprs_plan* P = S->plan;
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    record_prep(col_last_prep(S, g), one_plus_lambda, sigma_epsilon, tau_beta);
    const PrepRow r{0, P->m, (int64_t)g * P->m, logit_pi, log_tau_beta, sigma_epsilon, tau_beta, one_plus_lambda};
    return prep_launch(S, 1, &r);
}

int viprs_state_set_log_var_tau(viprs_state* S, const double* log_var_tau) {
    if (!S || !log_var_tau) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "not a mixture state");
    viprs_plan* P = S->plan;
    const size_t n = (size_t)P->m * S->width;
    if (n == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(S->d_log_var_tau0.alloc(n));
    HIP_TRY(hipMemcpyAsync(S->d_log_var_tau0.p, log_var_tau, n * sizeof(double), hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    return VIPRS_OK;
}

// a mixture prep row from (log_null_pi, sigma_eps, one_plus_lambda) and the K-vectors logit_pi, log_tau_beta, tau_beta
static MixPrepRow mix_prep_row(int64_t i0, int64_t i1, int K, const double* scalars, const double* logit_pi,
                               const double* log_tau_beta, const double* tau_beta) {
    MixPrepRow r{};
    r.i0 = i0;
    r.i1 = i1;
    r.log_null_pi = scalars[0];
    r.sigma_eps = scalars[1];
    r.one_plus_lambda = scalars[2];
    for (int k = 0; k < K; ++k) { r.logit_pi[k] = logit_pi[k]; r.log_tau[k] = log_tau_beta[k]; r.tau[k] = tau_beta[k]; }
    return r;
}

int viprs_state_prep_mixture(viprs_state* S, const double* logit_pi, const double* log_tau_beta, const double* tau_beta,
                             double log_null_pi, double sigma_epsilon, double one_plus_lambda) {
    if (!S || !logit_pi || !log_tau_beta || !tau_beta) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "not a mixture state");
    if (S->width > kMixResidentK) return fail(VIPRS_EUNSUPPORTED, "device-resident mixture iteration: K <= 8");
    if (!S->d_n.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp has not been called");
    viprs_plan* P = S->plan;
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    const double scalars[3] = {log_null_pi, sigma_epsilon, one_plus_lambda};
    const MixPrepRow r = mix_prep_row(0, P->m, S->width, scalars, logit_pi, log_tau_beta, tau_beta);
    return prep_mixture_launch(S, 1, &r);
}

int viprs_state_sums_mixture_begin(viprs_state* S, double one_plus_lambda) {
    if (!S) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "not a mixture state");
    if (S->width > kMixResidentK) return fail(VIPRS_EUNSUPPORTED, "device-resident mixture iteration: K <= 8");
    viprs_plan* P = S->plan;
    const int N = kMixSums(S->width);
    if (P->m == 0) return sums_nothing(S, true, 1, N);
    if (S->d_var_tau.n < (size_t)P->m * S->width || !S->d_log_var_tau0.p)
        return fail(VIPRS_EINVAL, "viprs_state_prep_mixture / viprs_state_set_log_var_tau have not been called");
    const SumsRow r = sums_row(S, 0, P->m, 0, one_plus_lambda, false, nullptr);
    return sums_enqueue(S, true, 1, N, &r);
}

int viprs_state_sums_mixture_end(viprs_state* S, double* out) {
    if (!S || !out) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "not a mixture state");
    return sums_collect(S, out, "viprs_state_sums_mixture_begin", kMixSums(S->width));
}

int viprs_state_prep_columns(viprs_state* S, int n, const double* params) {
    if (!S || !params) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "not a grid state");
    if (n < 0 || n > S->width) return fail(VIPRS_EINVAL, "bad column count");
    for (int i = 0; i < n; ++i)
        if (params[6 * i] < 0 || params[6 * i] >= S->width || params[6 * i] != floor(params[6 * i]))
            return fail(VIPRS_EINVAL, "model index out of range");
    if (!S->d_n.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp has not been called");
    viprs_plan* P = S->plan;
    if (P->m == 0 || n == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    PrepRow* h = nullptr;
    const int rc = prep_staging(S, n, &h);
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const double* p = params + (size_t)6 * i;
        record_prep(col_last_prep(S, (int)p[0]), p[5], p[3], p[4]);
        h[i] = PrepRow{0, P->m, (int64_t)p[0] * P->m, p[1], p[2], p[3], p[4], p[5]};
    }
    return prep_launch(S, n, nullptr);
}

int viprs_state_sums_columns_begin(viprs_state* S, int n, const double* cols) {
    if (!S || !cols) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "not a grid state");
    if (n < 0 || n > S->width) return fail(VIPRS_EINVAL, "bad column count");
    for (int i = 0; i < n; ++i)
        if (cols[2 * i] < 0 || cols[2 * i] >= S->width || cols[2 * i] != floor(cols[2 * i]))
            return fail(VIPRS_EINVAL, "model index out of range");
    viprs_plan* P = S->plan;
    if (P->m == 0 || n == 0) return sums_nothing(S, false, n, kNSums);
    for (int i = 0; i < n; ++i)
        if (std::isnan(*col_last_prep(S, (int)cols[2 * i]))) return fail(VIPRS_EINVAL, "viprs_state_prep_column(s) has not been called");
    HIP_TRY(hipSetDevice(P->device));
    // (the sums staging is free: the previous reduction that read it has been collected)
    const int rc = row_buffers(S, n);
    if (rc != VIPRS_OK) return rc;
    SumsRow* h = sums_staging(S);
    for (int i = 0; i < n; ++i)
        h[i] = sums_row(S, 0, P->m, (int64_t)cols[2 * i], cols[2 * i + 1], true, col_last_prep(S, (int)cols[2 * i]));
    return sums_enqueue(S, false, n, kNSums, nullptr);
}

int viprs_state_enet_sums(viprs_state* S, int n, const int32_t* cols, double* out) {
    if (!S || !out) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind == VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "elastic-net sums: not defined for a mixture state");
    if (S->float_dtype != VIPRS_F32) return fail(VIPRS_EUNSUPPORTED, "elastic-net sums: float64 states are not supported");
    const bool grid = S->model_kind == VIPRS_MODEL_GRID;
    if (n < 0 || n > S->width) return fail(VIPRS_EINVAL, "bad column count");
    if (!cols && n != S->width) return fail(VIPRS_EINVAL, "cols == NULL lists every column: n must be the state's width");
    for (int i = 0; cols && i < n; ++i)
        if (cols[i] < 0 || cols[i] >= S->width) return fail(VIPRS_EINVAL, "model index out of range");
    viprs_plan* P = S->plan;
    for (int k = 0; k < n * kNEnetSums; ++k) out[k] = 0.0;
    if (n == 0 || (P->m == 0 && !S->comm)) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    int rc = row_buffers(S, n);
    if (rc != VIPRS_OK) return rc;
    // (the sums staging is free: the previous reduction that read it has been collected)
    SumsRow* h = sums_staging(S);
    for (int i = 0; i < n; ++i) {
        h[i] = sums_row(S, 0, P->m, cols ? cols[i] : i, 0.0, false, nullptr);
        if (grid) h[i].nb = grid_sums_blocks(P->m);          // THE ORDER of a grid state's rows
    }
    rc = sums_enqueue(S, kSumsElasticNet, n, kNEnetSums, nullptr);
    if (rc != VIPRS_OK) return rc;
    std::vector<double> got((size_t)n * kNEnetSums);
    rc = sums_collect(S, got.data(), "viprs_state_enet_sums");
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i) {                             // the maximum travels last, the header has it first
        const double* g = got.data() + (size_t)i * kNEnetSums;
        out[i * kNEnetSums] = g[kNEnetSums - 1];
        for (int k = 1; k < kNEnetSums; ++k) out[i * kNEnetSums + k] = g[k - 1];
    }
    return VIPRS_OK;
}

int viprs_state_cs_sums(viprs_state* S, int n, const int32_t* cols, double* out) {
    int rc = cs_state_check(S, "sums");
    if (rc != VIPRS_OK) return rc;
    if (!out) return fail(VIPRS_EINVAL, "PRS-CS sums: out is null");
    if (n < 0 || n > S->width) return fail(VIPRS_EINVAL, "PRS-CS sums: bad column count");
    if (!cols && n != S->width) return fail(VIPRS_EINVAL, "PRS-CS sums: cols == NULL lists every column: n must be the state's width");
    std::vector<char> seen((size_t)S->width, 0);
    for (int i = 0; cols && i < n; ++i) {
        if (cols[i] < 0 || cols[i] >= S->width) return fail(VIPRS_EINVAL, "PRS-CS sums: column out of range");
        if (seen[(size_t)cols[i]]) return fail(VIPRS_EINVAL, "PRS-CS sums: a column is listed twice");
        seen[(size_t)cols[i]] = 1;
    }
    viprs_plan* P = S->plan;
    if (P->m > 0 && !S->d_n.p) return fail(VIPRS_EINVAL, "PRS-CS sums: viprs_state_set_n_per_snp has not been called");
    for (int k = 0; k < n * VIPRS_N_CS_SUMS; ++k) out[k] = 0.0;
    if (n == 0 || P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    rc = cs_ensure_buffers(S);
    if (rc != VIPRS_OK) return rc;
    rc = row_buffers(S, n);
    if (rc != VIPRS_OK) return rc;
    // (the sums staging is free: the previous reduction that read it has been collected)
    SumsRow* h = sums_staging(S);
    for (int i = 0; i < n; ++i) {
        h[i] = sums_row(S, 0, P->m, cols ? cols[i] : i, 0.0, false, nullptr);
        h[i].nb = grid_sums_blocks(P->m);                     // THE ORDER of a grid state's rows
    }
    rc = sums_enqueue(S, kSumsCs, n, kNCsSums, nullptr);
    if (rc != VIPRS_OK) return rc;
    std::vector<double> got((size_t)n * kNCsSums);
    rc = sums_collect(S, got.data(), "viprs_state_cs_sums");
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i)                               // (the fifth slot is the empty maximum of the final pass)
        for (int k = 0; k < VIPRS_N_CS_SUMS; ++k) out[i * VIPRS_N_CS_SUMS + k] = got[(size_t)i * kNCsSums + k];
    return VIPRS_OK;
}

int viprs_state_sums_columns_end(viprs_state* S, double* out) {
    if (!S || !out) return fail(VIPRS_EINVAL, "null argument");
    return sums_collect(S, out, "viprs_state_sums_columns_begin");
}

int viprs_state_sums_column(viprs_state* S, int g, double one_plus_lambda, double* out) {
    if (!out) return fail(VIPRS_EINVAL, "null argument");
    int rc = grid_column_check(S, g);
    if (rc != VIPRS_OK) return rc;
    viprs_plan* P = S->plan;
    for (int k = 0; k < kNSums; ++k) out[k] = 0.0;
    if (P->m == 0 && !S->comm) return VIPRS_OK;
    if (P->m > 0 && std::isnan(*col_last_prep(S, g))) return fail(VIPRS_EINVAL, "viprs_state_prep_column(s) has not been called");
    const SumsRow r = sums_row(S, 0, P->m, g, one_plus_lambda, true, col_last_prep(S, g));
    rc = sums_enqueue(S, false, 1, kNSums, &r);
    return rc != VIPRS_OK ? rc : sums_collect(S, out, "viprs_state_sums_columns_begin");
}

int viprs_state_reset_column(viprs_state* S, int g, double pi) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    if (S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "not a grid state");
    if (g < 0 || g >= S->width) return fail(VIPRS_EINVAL, "model index out of range");
    viprs_plan* P = S->plan;
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    const int64_t off = (int64_t)g * P->m, n = P->m;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (S->float_dtype == VIPRS_F32)
        reset_state_kernel<float><<<grid, 256, 0, P->stream>>>(
            (float*)S->f[VIPRS_FIELD_VAR_GAMMA].p + off, (float*)S->f[VIPRS_FIELD_VAR_MU].p + off, n,
            (float*)S->f[VIPRS_FIELD_ETA].p + off, (float*)S->f[VIPRS_FIELD_Q].p + off,
            (float*)S->f[VIPRS_FIELD_ETA_DIFF].p + off, n, (float)pi);
    else
        reset_state_kernel<double><<<grid, 256, 0, P->stream>>>(
            (double*)S->f[VIPRS_FIELD_VAR_GAMMA].p + off, (double*)S->f[VIPRS_FIELD_VAR_MU].p + off, n,
            (double*)S->f[VIPRS_FIELD_ETA].p + off, (double*)S->f[VIPRS_FIELD_Q].p + off,
            (double*)S->f[VIPRS_FIELD_ETA_DIFF].p + off, n, pi);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

// ---- SNP groups: one spike-and-slab (or mixture) model per chromosome, all of them in ONE plan / state (bin/viprs_fit:232-238 fits one
// model per chromosome unless --genomewide; the chromosomes' LD blocks are independent, so their E-steps share one sweep)
int viprs_state_set_groups(viprs_state* S, int n_groups, const int64_t* group_start) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    if (S->model_kind == VIPRS_MODEL_MIXTURE && S->width > kMixResidentK)
        return fail(VIPRS_EUNSUPPORTED, "device-resident mixture iteration: K <= 8");
    viprs_plan* P = S->plan;
    // (a grid state's pair scalars and mask belong to the groups they were given for: dropped once the new list is valid)
    auto drop_pairs = [&]() {
        S->pair_prep.clear();
        S->group_cols_h.clear();
        S->blk_group_gen = ~0ull;
    };
    if (n_groups == 0) {                         // back to one set of hyper-parameters
        drop_pairs();
        S->n_groups = 0;
        S->group_start.clear();
        return VIPRS_OK;
    }
    if (n_groups < 0 || !group_start) return fail(VIPRS_EINVAL, "bad group list");
    if (group_start[0] != 0 || group_start[n_groups] != P->m) return fail(VIPRS_EINVAL, "the groups must cover SNPs 0 .. m");
    for (int g = 0; g < n_groups; ++g)
        if (group_start[g + 1] < group_start[g]) return fail(VIPRS_EINVAL, "group_start must not decrease");
    // a group is a set of whole LD blocks (its hyper-parameters are fixed within a block's sweep)
    for (const Block& b : P->blocks) {
        const int64_t* it = std::upper_bound(group_start, group_start + n_groups + 1, b.start);      // first boundary > b.start
        if (it != group_start + n_groups + 1 && *it < b.end) return fail(VIPRS_EINVAL, "a group boundary cuts through an LD block");
    }
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipStreamSynchronize(P->stream));
    drop_pairs();
    S->n_groups = n_groups;
    S->group_start.assign(group_start, group_start + n_groups + 1);
    if (S->model_kind == VIPRS_MODEL_GRID) S->pair_prep.assign((size_t)3 * n_groups * S->width, NAN);
    return VIPRS_OK;
}

static int group_rows_check(const viprs_state* S, int n, const double* rows, int width) {
    if (!S || !rows) return fail(VIPRS_EINVAL, "null argument");
    if (S->n_groups == 0) return fail(VIPRS_EINVAL, "viprs_state_set_groups has not been called");
    if (n < 0 || n > S->n_groups) return fail(VIPRS_EINVAL, "bad group count");
    for (int i = 0; i < n; ++i) {
        const double g = rows[(size_t)width * i];
        if (g < 0 || g >= S->n_groups || g != floor(g)) return fail(VIPRS_EINVAL, "group index out of range");
    }
    return VIPRS_OK;
}

// the sums of the groups rows[2 i] with one_plus_lambda rows[2 i + 1] (spike-and-slab or mixture: the stored var_tau, no
// per-SNP weight)
static int sums_groups_enqueue(viprs_state* S, bool mixture, int n, const double* rows, int n_sums) {
    HIP_TRY(hipSetDevice(S->plan->device));
    // (the sums staging is free: the previous reduction that read it has been collected)
    const int rc = row_buffers(S, n);
    if (rc != VIPRS_OK) return rc;
    SumsRow* h = sums_staging(S);
    for (int i = 0; i < n; ++i) {
        const size_t g = (size_t)rows[2 * i];
        h[i] = sums_row(S, S->group_start[g], S->group_start[g + 1], 0, rows[2 * i + 1], false, nullptr);
    }
    return sums_enqueue(S, mixture, n, n_sums, nullptr);
}

int viprs_state_prep_groups(viprs_state* S, int n, const double* params) {
    int rc = group_rows_check(S, n, params, 6);
    if (rc != VIPRS_OK) return rc;
    if (S->model_kind != VIPRS_MODEL_SPIKE_SLAB) return fail(VIPRS_EINVAL, "not a spike-and-slab state (viprs_state_prep_mixture_groups)");
    viprs_plan* P = S->plan;
    if (P->m == 0 || n == 0) return VIPRS_OK;
    if (!S->d_n.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp has not been called");
    HIP_TRY(hipSetDevice(P->device));
    PrepRow* h = nullptr;
    rc = prep_staging(S, n, &h);
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const double* p = params + (size_t)6 * i;
        const size_t g = (size_t)p[0];
        h[i] = PrepRow{S->group_start[g], S->group_start[g + 1], 0, p[1], p[2], p[3], p[4], p[5]};
    }
    return prep_launch(S, n, nullptr);
}

int viprs_state_sums_groups_begin(viprs_state* S, int n, const double* rows) {
    int rc = group_rows_check(S, n, rows, 2);
    if (rc != VIPRS_OK) return rc;
    if (S->model_kind != VIPRS_MODEL_SPIKE_SLAB) return fail(VIPRS_EINVAL, "not a spike-and-slab state (viprs_state_sums_mixture_groups_begin)");
    viprs_plan* P = S->plan;
    if (P->m == 0 || n == 0) return sums_nothing(S, false, n, kNSums);
    if (!S->d_var_tau.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp / viprs_state_prep_groups have not been called");
    return sums_groups_enqueue(S, false, n, rows, kNSums);
}

int viprs_state_sums_groups_end(viprs_state* S, double* out) {
    if (S && S->n_groups == 0) return fail(VIPRS_EINVAL, "viprs_state_set_groups has not been called");
    return viprs_state_sums_columns_end(S, out);          // same landing buffer and bookkeeping: rows of VIPRS_N_SUMS
}

// ---- the same for a mixture state (VIPRSMix per chromosome) ----
int viprs_state_prep_mixture_groups(viprs_state* S, int n, const double* params) {
    if (!S) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "not a mixture state");
    const int K = S->width, W = 4 + 3 * K;
    int rc = group_rows_check(S, n, params, W);
    if (rc != VIPRS_OK) return rc;
    viprs_plan* P = S->plan;
    if (P->m == 0 || n == 0) return VIPRS_OK;
    if (!S->d_n.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp has not been called");
    HIP_TRY(hipSetDevice(P->device));
    MixPrepRow* h = nullptr;
    rc = prep_staging(S, n, &h);
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const double* p = params + (size_t)W * i;
        const size_t g = (size_t)p[0];
        h[i] = mix_prep_row(S->group_start[g], S->group_start[g + 1], K, p + 1, p + 4, p + 4 + K, p + 4 + 2 * K);
    }
    return prep_mixture_launch(S, n, nullptr);
}

int viprs_state_sums_mixture_groups_begin(viprs_state* S, int n, const double* rows) {
    if (!S) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "not a mixture state");
    int rc = group_rows_check(S, n, rows, 2);
    if (rc != VIPRS_OK) return rc;
    viprs_plan* P = S->plan;
    const int N = kMixSums(S->width);
    if (P->m == 0 || n == 0) return sums_nothing(S, true, n, N);
    if (S->d_var_tau.n < (size_t)P->m * S->width || !S->d_log_var_tau0.p)
        return fail(VIPRS_EINVAL, "viprs_state_prep_mixture_groups / viprs_state_set_log_var_tau have not been called");
    return sums_groups_enqueue(S, true, n, rows, N);
}

int viprs_state_sums_mixture_groups_end(viprs_state* S, double* out) {
    if (!S || !out) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "not a mixture state");
    if (S->n_groups == 0) return fail(VIPRS_EINVAL, "viprs_state_set_groups has not been called");
    return sums_collect(S, out, "viprs_state_sums_mixture_groups_begin");
}

// ---- SNP groups of a grid state: (group, column) pairs ------------------------------------------------------------------
static int pair_rows_check(const viprs_state* S, int n, const double* rows, int width) {
    if (!S || (n > 0 && !rows)) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "not a grid state");
    if (S->n_groups == 0) return fail(VIPRS_EINVAL, "viprs_state_set_groups has not been called");
    if (S->pair_prep.size() != (size_t)3 * S->n_groups * S->width)
        return fail(VIPRS_EINVAL, "the grid state's groups are not set up (viprs_state_set_groups)");
    if (n < 0 || (int64_t)n > (int64_t)S->n_groups * S->width) return fail(VIPRS_EINVAL, "bad row count");
    for (int i = 0; i < n; ++i) {
        const double g = rows[(size_t)width * i], c = rows[(size_t)width * i + 1];
        if (g < 0 || g >= S->n_groups || g != floor(g)) return fail(VIPRS_EINVAL, "group index out of range");
        if (c < 0 || c >= S->width || c != floor(c)) return fail(VIPRS_EINVAL, "model index out of range");
    }
    return VIPRS_OK;
}

// (one_plus_lambda, sigma_eps, tau_beta) of the pair's last prep
static double* pair_last_prep(viprs_state* S, double g, double c) {
    return S->pair_prep.data() + 3 * ((size_t)g * (size_t)S->width + (size_t)c);
}

int viprs_state_prep_grid_groups(viprs_state* S, int n, const double* params) {
    int rc = pair_rows_check(S, n, params, 7);
    if (rc != VIPRS_OK) return rc;
    viprs_plan* P = S->plan;
    if (P->m == 0 || n == 0) return VIPRS_OK;
    if (!S->d_n.p) return fail(VIPRS_EINVAL, "viprs_state_set_n_per_snp has not been called");
    HIP_TRY(hipSetDevice(P->device));
    PrepRow* h = nullptr;
    rc = prep_staging(S, n, &h);
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const double* p = params + (size_t)7 * i;
        const size_t g = (size_t)p[0];
        record_prep(pair_last_prep(S, p[0], p[1]), p[6], p[4], p[5]);
        h[i] = PrepRow{S->group_start[g], S->group_start[g + 1], (int64_t)p[1] * P->m, p[2], p[3], p[4], p[5], p[6]};
    }
    return prep_launch(S, n, nullptr);
}

int viprs_state_sums_grid_groups_begin(viprs_state* S, int n, const double* rows) {
    int rc = pair_rows_check(S, n, rows, 3);
    if (rc != VIPRS_OK) return rc;
    viprs_plan* P = S->plan;
    if (P->m == 0 || n == 0) return sums_nothing(S, false, n, kNSums);
    for (int i = 0; i < n; ++i)
        if (std::isnan(*pair_last_prep(S, rows[(size_t)3 * i], rows[(size_t)3 * i + 1])))
            return fail(VIPRS_EINVAL, "viprs_state_prep_grid_groups has not been called for this (group, column) pair");
    HIP_TRY(hipSetDevice(P->device));
    // (the sums staging is free: the previous reduction that read it has been collected)
    rc = row_buffers(S, n);
    if (rc != VIPRS_OK) return rc;
    SumsRow* h = sums_staging(S);
    for (int i = 0; i < n; ++i) {
        const double* r = rows + (size_t)3 * i;
        const size_t g = (size_t)r[0];
        h[i] = sums_row(S, S->group_start[g], S->group_start[g + 1], (int64_t)r[1], r[2], false, pair_last_prep(S, r[0], r[1]));
    }
    return sums_enqueue(S, false, n, kNSums, nullptr);
}

int viprs_state_sums_grid_groups_end(viprs_state* S, double* out) {
    if (!S || !out) return fail(VIPRS_EINVAL, "null argument");
    if (S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "not a grid state");
    if (S->n_groups == 0) return fail(VIPRS_EINVAL, "viprs_state_set_groups has not been called");
    return viprs_state_sums_columns_end(S, out);          // same landing buffer and bookkeeping: rows of VIPRS_N_SUMS
}

int viprs_state_set_group_columns(viprs_state* S, int n_groups, int width, const uint8_t* active) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    if (S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "not a grid state");
    if (n_groups == 0) { S->group_cols_h.clear(); return VIPRS_OK; }
    if (!active) return fail(VIPRS_EINVAL, "null argument");
    if (S->n_groups == 0) return fail(VIPRS_EINVAL, "viprs_state_set_groups has not been called");
    if (n_groups != S->n_groups || width != S->width) return fail(VIPRS_EINVAL, "the mask must be n_groups x width of the state");
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    const size_t n = (size_t)n_groups * (size_t)width;
    HIP_TRY(hipStreamSynchronize(P->stream));              // (a sweep in flight reads the old mask)
    if (S->d_group_cols.n != n) HIP_TRY(S->d_group_cols.alloc(n));
    S->group_cols_h.assign(active, active + n);
    for (uint8_t& v : S->group_cols_h) v = v ? 1 : 0;
    HIP_TRY(hipMemcpy(S->d_group_cols.p, S->group_cols_h.data(), n, hipMemcpyHostToDevice));
    return VIPRS_OK;
}

}  // extern "C"

// ---- committing SNP groups of a spike-and-slab state into columns of a grid state (the pathwise grid search per chromosome:
// a chromosome whose grid point has stopped stores its state as column `column` of its (m_c, G) result) -------------------
namespace {

struct CommitRow {
    int64_t src, dst, len;                         // element offsets into a field of the source / destination state, length
};

struct CommitFields {
    const void* src[5];
    void* dst[5];
};

// blockIdx.z: the field, blockIdx.y (+ gridDim.y strides): the row, x: the row's elements.  A destination range is split into a
// scalar head up to the first 16-byte boundary, 16-byte vector stores and a scalar tail; the source is read as 16-byte
// vectors where it shares the destination's alignment, element by element otherwise.
template <typename T>
__global__ __launch_bounds__(256) void commit_groups_kernel(CommitFields f, const CommitRow* __restrict__ rows, int n) {
    constexpr int V = 16 / sizeof(T);
    using Vec = typename std::conditional<sizeof(T) == 4, float4, double2>::type;
    const T* __restrict__ src_f = static_cast<const T*>(f.src[blockIdx.z]);
    T* __restrict__ dst_f = static_cast<T*>(f.dst[blockIdx.z]);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int r = blockIdx.y; r < n; r += gridDim.y) {
        const CommitRow row = rows[r];
        const T* __restrict__ s = src_f + row.src;
        T* __restrict__ d = dst_f + row.dst;
        const int64_t head = std::min<int64_t>(row.len, (V - (int64_t)((reinterpret_cast<uintptr_t>(d) / sizeof(T)) % V)) % V);
        const int64_t nv = (row.len - head) / V;
        const int64_t body_end = head + nv * V;
        const bool aligned = ((reinterpret_cast<uintptr_t>(s + head)) % 16) == 0;
        for (int64_t u = tid; u < nv; u += stride) {
            Vec v;
            if (aligned) {
                v = *reinterpret_cast<const Vec*>(s + head + u * V);
            } else {
                T t[V];
#pragma unroll
                for (int k = 0; k < V; ++k) t[k] = s[head + u * V + k];
                if constexpr (V == 4) v = Vec{t[0], t[1], t[2], t[3]};
                else v = Vec{t[0], t[1]};
            }
            *reinterpret_cast<Vec*>(d + head + u * V) = v;
        }
        if (tid < head) d[tid] = s[tid];
        if (tid < row.len - body_end) d[body_end + tid] = s[body_end + tid];
    }
}

}  // namespace

extern "C" {

int viprs_state_commit_groups(viprs_state* dst, const viprs_state* src, int n, const int32_t* pairs) {
    if (!dst || !src) return fail(VIPRS_EINVAL, "null state");
    if (n < 0) return fail(VIPRS_EINVAL, "bad pair count");
    if (n > 0 && !pairs) return fail(VIPRS_EINVAL, "null argument");
    if (dst->plan != src->plan) return fail(VIPRS_EINVAL, "the two states are on different plans");
    if (dst->float_dtype != src->float_dtype) return fail(VIPRS_EINVAL, "the two states have different float dtypes");
    if (src->model_kind != VIPRS_MODEL_SPIKE_SLAB) return fail(VIPRS_EINVAL, "the source is not a spike-and-slab state");
    if (dst->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "the destination is not a grid state");
    if (src->n_groups == 0) return fail(VIPRS_EINVAL, "viprs_state_set_groups has not been called on the source");
    for (int i = 0; i < n; ++i) {
        if (pairs[2 * i] < 0 || pairs[2 * i] >= src->n_groups) return fail(VIPRS_EINVAL, "group index out of range");
        if (pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= dst->width) return fail(VIPRS_EINVAL, "column index out of range");
    }
    viprs_plan* P = src->plan;
    if (P->m == 0 || n == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    // the rows go through the source's pinned staging of batched prep rows (free once its last batched prep has read it)
    viprs_state* S = const_cast<viprs_state*>(src);
    CommitRow* h = nullptr;
    int rc = prep_staging(S, n, &h);
    if (rc != VIPRS_OK) return rc;
    static_assert(sizeof(CommitRow) <= sizeof(PrepRow), "a commit row must fit a prep row's room in the staging");
    int64_t longest = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t g = pairs[2 * i], c = pairs[2 * i + 1];
        const int64_t i0 = S->group_start[g], i1 = S->group_start[g + 1];
        h[i] = CommitRow{i0, c * P->m + i0, i1 - i0};
        longest = std::max(longest, i1 - i0);
    }
    HIP_TRY(hipMemcpyAsync(S->d_prep_rows.p, h, (size_t)n * sizeof(CommitRow), hipMemcpyHostToDevice, P->stream));
    CommitFields f;
    const int fields[5] = {VIPRS_FIELD_VAR_GAMMA, VIPRS_FIELD_VAR_MU, VIPRS_FIELD_ETA, VIPRS_FIELD_Q, VIPRS_FIELD_ETA_DIFF};
    for (int k = 0; k < 5; ++k) {
        f.src[k] = src->f[fields[k]].p;
        f.dst[k] = dst->f[fields[k]].p;
    }
    const int V = 16 / (int)float_size(src->float_dtype);
    const int64_t units = (longest + V - 1) / V + 1;
    const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(1, (units + 255) / 256), 1024),
                    (unsigned)std::min(n, 65535), 5);
    const CommitRow* rows = reinterpret_cast<const CommitRow*>(S->d_prep_rows.p);
    if (src->float_dtype == VIPRS_F32) commit_groups_kernel<float><<<grid, 256, 0, P->stream>>>(f, rows, n);
    else commit_groups_kernel<double><<<grid, 256, 0, P->stream>>>(f, rows, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S->ev_prep, P->stream));      // (the next batched prep reuses the staging once this copy is done)
    return VIPRS_OK;
}

}  // extern "C"
