// C ABI, SBayesR (include/viprs_hip.h): the draws kernel -- one Philox4x32-10 block per SNP --, the state's draw allocation
// and its upload / download, the sums of a sweep and the accumulators of the posterior mean and the inclusion probability.
// The sweep itself is viprs_state_bayesr_sweep (abi_estep.hip) on the policy of panel_bayesr.h.
#include "internal.h"
#include "panel_bayesr.h"
#include "philox.h"

using namespace viprs;

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kStreamTag = 0x40000000u;     // counter word 1: the Gibbs draws carry a column < 2^30 there, PRS-CS bit 31

// Thread t of the grid-stride walk takes SNPs t, t + threads, ... < m: every write lands inside the (m,) buffers.
__global__ __launch_bounds__(kBlock) void bayesr_draws_kernel(int64_t m, uint32_t k0, uint32_t k1, uint32_t d_lo, uint32_t d_hi,
                                                              float* __restrict__ unif, float* __restrict__ z) {
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (int64_t)gridDim.x * kBlock) {
        uint32_t c[4] = {(uint32_t)j, kStreamTag, d_lo, d_hi};
        philox4x32_10(c, k0, k1);
        const float u1 = open_unit(c[1]), u2 = open_unit(c[2]);
        const float t = -2.0f * logf(u1);
        unif[j] = open_unit(c[0]);
        z[j] = sqrtf(t) * cospif(2.0f * u2);
    }
}

__global__ __launch_bounds__(kBlock) void bayesr_accumulate_kernel(int64_t m, int K, const float* __restrict__ gamma,
                                                                   const float* __restrict__ mu, double* __restrict__ mean,
                                                                   double* __restrict__ pip) {
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (int64_t)gridDim.x * kBlock) {
        double s = 0.0, g = 0.0;
        for (int k = 0; k < K; ++k) {
            s += (double)gamma[j * K + k] * (double)mu[j * K + k];
            g += (double)gamma[j * K + k];
        }
        mean[j] += s;
        pip[j] += g;
    }
}

// The sums of a sweep: the row scheme and THE ORDER of enet_sums_kernel (abi_state.hip) for the one row [0, m) of a mixture
// state -- workgroup bx of nb takes SNPs bx * 256 + t, + nb * 256, ... in thread t, serially; the 256 threads are combined by
// the halving tree in LDS; stage 2 adds the nb partials of a sum on one wave, lane l taking partials l, l + 64, ... in order,
// then the xor-shuffle tree 32, 16, .., 1.  Slots (kSlots of them, whatever K): counts of k* = 0..4 | sum eta^2 [k* = k],
// k = 1..4 | sum q eta | sum eta^2 | sum std_beta eta.
constexpr int kSlots = 2 * kBayesRMaxK + 1 + 3;
__host__ __device__ inline int bayesr_sums_blocks(int64_t count) {
    const int64_t nb = (count + kBlock - 1) / kBlock;
    return (int)(nb < 1024 ? nb : 1024);
}

__global__ __launch_bounds__(kBlock) void bayesr_sums_kernel(int64_t m, int nb, const int32_t* __restrict__ kstar,
                                                             const float* __restrict__ eta, const float* __restrict__ q,
                                                             const float* __restrict__ beta, double* __restrict__ partials) {
    __shared__ double red[kSlots][kBlock];
    double acc[kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)nb * kBlock) {
        const double e = (double)eta[i];
        const int ks = kstar[i];
#pragma unroll
        for (int k = 0; k <= kBayesRMaxK; ++k) acc[k] += ks == k ? 1.0 : 0.0;
#pragma unroll
        for (int k = 1; k <= kBayesRMaxK; ++k) acc[kBayesRMaxK + k] += ks == k ? e * e : 0.0;
        acc[2 * kBayesRMaxK + 1] += (double)q[i] * e;
        acc[2 * kBayesRMaxK + 2] += e * e;
        acc[2 * kBayesRMaxK + 3] += (double)beta[i] * e;
    }
#pragma unroll
    for (int k = 0; k < kSlots; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < kSlots; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < kSlots) partials[(int64_t)blockIdx.x * kSlots + threadIdx.x] = red[threadIdx.x][0];
}

// one wave per slot
__global__ void bayesr_sums_final_kernel(const double* __restrict__ partials, int nb, double* __restrict__ out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    double a = 0.0;
    for (int b = lane; b < nb; b += 64) a += partials[(int64_t)b * kSlots + k];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) out[k] = a;
}

unsigned walk_grid(int64_t total) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + kBlock - 1) / kBlock, 8192));
}

int ensure_acc(viprs_state* S) {
    const size_t m = (size_t)S->plan->m;
    if (S->d_bayesr_acc.p || m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(S->d_bayesr_acc.alloc(2 * m));
    HIP_TRY(hipMemsetAsync(S->d_bayesr_acc.p, 0, 2 * m * sizeof(double), S->plan->stream));
    return VIPRS_OK;
}

// the device buffer of a viprs_bayesr_buffer code and its size in bytes; the buffers come into being here as well (zeros)
int bayesr_buffer(viprs_state* S, int which, void** p, size_t* bytes) {
    const size_t m = (size_t)S->plan->m;
    int rc;
    switch (which) {
        case VIPRS_BAYESR_UNIF: case VIPRS_BAYESR_Z: case VIPRS_BAYESR_KSTAR:
            rc = bayesr_ensure_draws(S);
            if (rc != VIPRS_OK) return rc;
            *p = S->d_bayesr.p ? S->d_bayesr.p + (size_t)which * m : nullptr;
            *bytes = m * sizeof(float);
            return VIPRS_OK;
        case VIPRS_BAYESR_MEAN_SUM: case VIPRS_BAYESR_PIP_SUM:
            rc = ensure_acc(S);
            if (rc != VIPRS_OK) return rc;
            *p = S->d_bayesr_acc.p ? S->d_bayesr_acc.p + (which == VIPRS_BAYESR_PIP_SUM ? m : 0) : nullptr;
            *bytes = m * sizeof(double);
            return VIPRS_OK;
        default: return fail(VIPRS_EINVAL, "bad SBayesR buffer code");
    }
}

}  // namespace

namespace viprs {

static_assert(VIPRS_BAYESR_UNIF == 0 && VIPRS_BAYESR_Z == 1 && VIPRS_BAYESR_KSTAR == 2, "the order of the draw allocation");
static_assert(VIPRS_BAYESR_MAX_K == kBayesRMaxK, "the header's K limit is the policy's");
static_assert(sizeof(int32_t) == sizeof(float), "U | z | k* share one allocation of four-byte words");

int bayesr_state_check(const viprs_state* S, const char* what) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    const std::string w(what);
    if (S->model_kind != VIPRS_MODEL_MIXTURE)
        return fail(VIPRS_EINVAL, w + ": a state of kind VIPRS_MODEL_MIXTURE is needed (spike-and-slab and grid states are refused)");
    if (S->float_dtype != VIPRS_F32) return fail(VIPRS_EINVAL, w + ": float64 states are not supported (the kernels are float32)");
    if (S->width > kBayesRMaxK) return fail(VIPRS_EINVAL, w + ": more than 4 non-null components are not supported");
    if (S->n_groups > 0) return fail(VIPRS_EINVAL, w + ": a state with SNP groups is not supported");
    if (S->comm) return fail(VIPRS_EINVAL, w + ": a state with a communicator is not supported (several ranks are not built)");
    if (S->plan->m > 0 && !S->d_n.p) return fail(VIPRS_EINVAL, w + ": viprs_state_set_n_per_snp has not been called");
    return VIPRS_OK;
}

int bayesr_ensure_draws(viprs_state* S) {
    const size_t m = (size_t)S->plan->m;
    if (S->d_bayesr.p || m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(S->d_bayesr.alloc(3 * m));
    HIP_TRY(hipMemsetAsync(S->d_bayesr.p, 0, 3 * m * sizeof(float), S->plan->stream));
    return VIPRS_OK;
}

int bayesr_enqueue_draws(viprs_state* S, uint64_t seed, uint64_t draw_index) {
    viprs_plan* P = S->plan;
    int rc = bayesr_ensure_draws(S);
    if (rc != VIPRS_OK || P->m == 0) return rc;
    rc = P->time_bayesr_draws.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    bayesr_draws_kernel<<<walk_grid(P->m), kBlock, 0, P->stream>>>(P->m, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw_index,
                                                                   (uint32_t)(draw_index >> 32), S->d_bayesr.p, S->d_bayesr.p + P->m);
    HIP_TRY(hipGetLastError());
    return P->time_bayesr_draws.stop(P->stream);
}

}  // namespace viprs

extern "C" {

int viprs_state_bayesr_draws(viprs_state* S, uint64_t seed, uint64_t draw_index) {
    int rc = bayesr_state_check(S, "SBayesR draws");
    if (rc != VIPRS_OK || S->plan->m == 0) return rc;
    HIP_TRY(hipSetDevice(S->plan->device));
    rc = bayesr_enqueue_draws(S, seed, draw_index);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_bayesr_sums(viprs_state* S, double* out) {
    int rc = bayesr_state_check(S, "SBayesR sums");
    if (rc != VIPRS_OK) return rc;
    if (!out) return fail(VIPRS_EINVAL, "SBayesR sums: out is null");
    viprs_plan* P = S->plan;
    const int K = S->width, n_out = 2 * K + 1 + 3;
    if (P->m > 0 && !S->d_bayesr.p)
        return fail(VIPRS_EINVAL, "SBayesR sums: the draw buffers do not exist (no draws call, sweep or upload yet)");
    for (int k = 0; k < n_out; ++k) out[k] = 0.0;
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    const int nb = bayesr_sums_blocks(P->m);
    HIP_TRY(S->d_bayesr_sums.reserve((size_t)(nb + 1) * kSlots));
    double* d_out = S->d_bayesr_sums.p + (size_t)nb * kSlots;
    bayesr_sums_kernel<<<nb, kBlock, 0, P->stream>>>(P->m, nb, reinterpret_cast<const int32_t*>(S->d_bayesr.p) + 2 * P->m,
                                                     (const float*)S->f[VIPRS_FIELD_ETA].p, (const float*)S->f[VIPRS_FIELD_Q].p,
                                                     (const float*)S->f[VIPRS_FIELD_STD_BETA].p, S->d_bayesr_sums.p);
    HIP_TRY(hipGetLastError());
    bayesr_sums_final_kernel<<<kSlots, 64, 0, P->stream>>>(S->d_bayesr_sums.p, nb, d_out);
    HIP_TRY(hipGetLastError());
    double got[kSlots];
    HIP_TRY(hipMemcpyAsync(got, d_out, sizeof(got), hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    rc = check_device_error(P);
    if (rc != VIPRS_OK) return rc;
    for (int k = 0; k <= K; ++k) out[k] = got[k];
    for (int k = 1; k <= K; ++k) out[K + k] = got[kBayesRMaxK + k];
    for (int k = 0; k < 3; ++k) out[2 * K + 1 + k] = got[2 * kBayesRMaxK + 1 + k];
    return VIPRS_OK;
}

int viprs_state_bayesr_accumulate(viprs_state* S) {
    int rc = bayesr_state_check(S, "SBayesR accumulate");
    if (rc != VIPRS_OK || S->plan->m == 0) return rc;
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    rc = ensure_acc(S);
    if (rc != VIPRS_OK) return rc;
    bayesr_accumulate_kernel<<<walk_grid(P->m), kBlock, 0, P->stream>>>(
        P->m, S->width, (const float*)S->f[VIPRS_FIELD_VAR_GAMMA].p, (const float*)S->f[VIPRS_FIELD_VAR_MU].p, S->d_bayesr_acc.p,
        S->d_bayesr_acc.p + P->m);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

int viprs_state_bayesr_reset_mean(viprs_state* S) {
    int rc = bayesr_state_check(S, "SBayesR reset_mean");
    if (rc != VIPRS_OK || S->plan->m == 0) return rc;
    if (!S->d_bayesr_acc.p) return ensure_acc(S);
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(hipMemsetAsync(S->d_bayesr_acc.p, 0, 2 * (size_t)S->plan->m * sizeof(double), S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_bayesr_upload(viprs_state* S, int which, const void* host) {
    int rc = bayesr_state_check(S, "SBayesR upload");
    if (rc != VIPRS_OK) return rc;
    if (which < 0 || which >= VIPRS_BAYESR_BUFFER_COUNT) return fail(VIPRS_EINVAL, "bad SBayesR buffer code");
    if (!host) return fail(VIPRS_EINVAL, "host buffer is null");
    void* p = nullptr;
    size_t bytes = 0;
    rc = bayesr_buffer(S, which, &p, &bytes);
    if (rc != VIPRS_OK || bytes == 0) return rc;
    HIP_TRY(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_bayesr_download(viprs_state* S, int which, void* host) {
    int rc = bayesr_state_check(S, "SBayesR download");
    if (rc != VIPRS_OK) return rc;
    if (which < 0 || which >= VIPRS_BAYESR_BUFFER_COUNT) return fail(VIPRS_EINVAL, "bad SBayesR buffer code");
    if (!host) return fail(VIPRS_EINVAL, "host buffer is null");
    void* p = nullptr;
    size_t bytes = 0;
    rc = bayesr_buffer(S, which, &p, &bytes);
    if (rc != VIPRS_OK || bytes == 0) return rc;
    HIP_TRY(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return check_device_error(S->plan);
}

int viprs_plan_last_bayesr_draws_ms(viprs_plan* P, double* ms) {
    if (!P || !ms) return fail(VIPRS_EINVAL, "null argument");
    return P->time_bayesr_draws.elapsed(P->device, ms, "no timed SBayesR draws call yet");
}

}  // extern "C"
