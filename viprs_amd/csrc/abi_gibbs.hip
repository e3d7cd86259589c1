// C ABI, LDpred2 Gibbs sweeps (include/viprs_hip.h): the draws kernel -- one Philox4x32-10 block per (SNP, column) --, the
// state's draw buffers and their upload / download, the accumulator of the Rao-Blackwellised means.  The sweep itself is
// viprs_state_gibbs_sweep (abi_estep.hip) on the policy of panel_gibbs.h.
#include "internal.h"
#include "philox.h"

using namespace viprs;

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace {

constexpr int kDrawsBlock = 256;

// Thread t of the grid-stride walk takes element i = t, t + threads, ... of the n_active x m rectangle: column
// active[i / m], SNP i % m.  Every write lands inside column active[.] < width of the (m, width) buffers (the entry point
// has checked the list).
__global__ __launch_bounds__(kDrawsBlock) void gibbs_draws_kernel(int64_t m, int width, const int32_t* __restrict__ active,
                                                                  int n_active, uint32_t k0, uint32_t k1, uint32_t d_lo,
                                                                  uint32_t d_hi, const float* __restrict__ hvt,
                                                                  float* __restrict__ unif, float* __restrict__ noise) {
    const int64_t total = m * n_active;
    for (int64_t i = (int64_t)blockIdx.x * kDrawsBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kDrawsBlock) {
        const int g = active[i / m];
        const int64_t j = i % m;
        if (g < 0 || g >= width) continue;
        uint32_t c[4] = {(uint32_t)j, (uint32_t)g, d_lo, d_hi};
        philox4x32_10(c, k0, k1);
        const float u1 = open_unit(c[1]), u2 = open_unit(c[2]);
        const float t = -2.0f * logf(u1);
        const float z = sqrtf(t) * cospif(2.0f * u2);
        const int64_t at = (int64_t)g * m + j;
        const float sd = 1.0f / sqrtf(2.0f * hvt[at]);
        unif[at] = open_unit(c[0]);
        noise[at] = z * sd;
    }
}

__global__ __launch_bounds__(kDrawsBlock) void gibbs_accumulate_kernel(int64_t m, int width, const int32_t* __restrict__ active,
                                                                       int n_active, const float* __restrict__ gamma,
                                                                       const float* __restrict__ mu, double* __restrict__ mean) {
    const int64_t total = m * n_active;
    for (int64_t i = (int64_t)blockIdx.x * kDrawsBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kDrawsBlock) {
        const int g = active[i / m];
        if (g < 0 || g >= width) continue;
        const int64_t at = (int64_t)g * m + i % m;
        mean[at] += (double)gamma[at] * (double)mu[at];
    }
}

unsigned walk_grid(int64_t total) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + kDrawsBlock - 1) / kDrawsBlock, 8192));
}

// what every Gibbs entry point refuses, in one place (the sweep adds the mask and the route)
int gibbs_state_check(const viprs_state* S, const char* what) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    if (S->model_kind != VIPRS_MODEL_GRID)
        return fail(VIPRS_EINVAL, std::string(what) + ": a state of kind VIPRS_MODEL_GRID is needed (spike-and-slab-kind and "
                                  "mixture states are refused)");
    if (S->float_dtype != VIPRS_F32) return fail(VIPRS_EINVAL, std::string(what) + ": float64 states are not supported");
    return VIPRS_OK;
}

// the active list of a call, checked and on the device (S->d_active); null = every column
int gibbs_active(viprs_state* S, const int32_t* active, int& n_active) {
    std::vector<int32_t> all;
    if (!active) {
        all.resize((size_t)S->width);
        for (int g = 0; g < S->width; ++g) all[(size_t)g] = g;
        active = all.data();
        n_active = S->width;
    }
    if (n_active < 0) return fail(VIPRS_EINVAL, "bad active_model_idx");
    for (int i = 0; i < n_active; ++i)
        if (active[i] < 0 || active[i] >= S->width) return fail(VIPRS_EINVAL, "active_model_idx out of range");
    if (n_active == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(S->plan->device));
    if (S->d_active.n < (size_t)n_active) HIP_TRY(S->d_active.alloc((size_t)std::max(n_active, S->width)));
    HIP_TRY(hipMemcpyAsync(S->d_active.p, active, sizeof(int32_t) * (size_t)n_active, hipMemcpyHostToDevice, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int gibbs_ensure_mean(viprs_state* S) {
    const size_t n = (size_t)S->plan->m * (size_t)S->width;
    if (S->d_gibbs_mean.p || n == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(S->d_gibbs_mean.alloc(n));
    HIP_TRY(hipMemsetAsync(S->d_gibbs_mean.p, 0, n * sizeof(double), S->plan->stream));
    return VIPRS_OK;
}

}  // namespace

namespace viprs {

int gibbs_ensure_draws(viprs_state* S) {
    const size_t n = (size_t)S->plan->m * (size_t)S->width;
    if (S->d_gibbs_draws.p || n == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(S->d_gibbs_draws.alloc(2 * n));
    HIP_TRY(hipMemsetAsync(S->d_gibbs_draws.p, 0, 2 * n * sizeof(float), S->plan->stream));
    return VIPRS_OK;
}

int gibbs_enqueue_draws(viprs_state* S, uint64_t seed, uint64_t draw_index, const int32_t* d_active, int n_active) {
    viprs_plan* P = S->plan;
    int rc = gibbs_ensure_draws(S);
    if (rc != VIPRS_OK) return rc;
    const int64_t total = P->m * n_active;
    if (total == 0) return VIPRS_OK;
    rc = P->time_gibbs_draws.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    const size_t n = (size_t)P->m * (size_t)S->width;
    gibbs_draws_kernel<<<walk_grid(total), kDrawsBlock, 0, P->stream>>>(
        P->m, S->width, d_active, n_active, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw_index,
        (uint32_t)(draw_index >> 32), (const float*)S->f[VIPRS_FIELD_SQRT_HALF_VAR_TAU].p, S->d_gibbs_draws.p,
        S->d_gibbs_draws.p + n);
    HIP_TRY(hipGetLastError());
    return P->time_gibbs_draws.stop(P->stream);
}

const float* gibbs_draws_slot(const viprs_state* S) {
    return reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(S->d_gibbs_draws.p) -
                                          reinterpret_cast<uintptr_t>(S->f[VIPRS_FIELD_MU_MULT].p));
}

}  // namespace viprs

extern "C" {

int viprs_state_gibbs_draws(viprs_state* S, uint64_t seed, uint64_t draw_index, const int32_t* active, int n_active) {
    int rc = gibbs_state_check(S, "Gibbs draws");
    if (rc != VIPRS_OK) return rc;
    rc = gibbs_active(S, active, n_active);
    if (rc != VIPRS_OK || n_active == 0) return rc;
    rc = gibbs_enqueue_draws(S, seed, draw_index, S->d_active.p, n_active);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_gibbs_accumulate(viprs_state* S, const int32_t* active, int n_active) {
    int rc = gibbs_state_check(S, "Gibbs accumulate");
    if (rc != VIPRS_OK) return rc;
    rc = gibbs_active(S, active, n_active);
    if (rc != VIPRS_OK || n_active == 0) return rc;
    viprs_plan* P = S->plan;
    rc = gibbs_ensure_mean(S);
    if (rc != VIPRS_OK) return rc;
    const int64_t total = P->m * n_active;
    if (total == 0) return VIPRS_OK;
    gibbs_accumulate_kernel<<<walk_grid(total), kDrawsBlock, 0, P->stream>>>(
        P->m, S->width, S->d_active.p, n_active, (const float*)S->f[VIPRS_FIELD_VAR_GAMMA].p,
        (const float*)S->f[VIPRS_FIELD_VAR_MU].p, S->d_gibbs_mean.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(P->stream));        // (the next call may overwrite d_active)
    return VIPRS_OK;
}

int viprs_state_gibbs_reset_mean(viprs_state* S) {
    int rc = gibbs_state_check(S, "Gibbs reset_mean");
    if (rc != VIPRS_OK) return rc;
    const size_t n = (size_t)S->plan->m * (size_t)S->width;
    if (!S->d_gibbs_mean.p) return gibbs_ensure_mean(S);
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(hipMemsetAsync(S->d_gibbs_mean.p, 0, n * sizeof(double), S->plan->stream));
    return VIPRS_OK;
}

// the device buffer, its size in bytes; the buffers come into being here as well (zeros)
static int gibbs_buffer(viprs_state* S, int which, void** p, size_t* bytes) {
    const size_t n = (size_t)S->plan->m * (size_t)S->width;
    int rc;
    switch (which) {
        case VIPRS_GIBBS_UNIF: case VIPRS_GIBBS_NOISE:
            rc = gibbs_ensure_draws(S);
            if (rc != VIPRS_OK) return rc;
            *p = S->d_gibbs_draws.p ? S->d_gibbs_draws.p + (which == VIPRS_GIBBS_NOISE ? n : 0) : nullptr;
            *bytes = n * sizeof(float);
            return VIPRS_OK;
        case VIPRS_GIBBS_MEAN_SUM:
            rc = gibbs_ensure_mean(S);
            if (rc != VIPRS_OK) return rc;
            *p = S->d_gibbs_mean.p;
            *bytes = n * sizeof(double);
            return VIPRS_OK;
        default: return fail(VIPRS_EINVAL, "bad Gibbs buffer code");
    }
}

int viprs_state_gibbs_upload(viprs_state* S, int which, const void* host) {
    int rc = gibbs_state_check(S, "Gibbs upload");
    if (rc != VIPRS_OK) return rc;
    if (which < 0 || which >= VIPRS_GIBBS_BUFFER_COUNT) return fail(VIPRS_EINVAL, "bad Gibbs buffer code");
    if (!host) return fail(VIPRS_EINVAL, "host buffer is null");
    void* p = nullptr;
    size_t bytes = 0;
    rc = gibbs_buffer(S, which, &p, &bytes);
    if (rc != VIPRS_OK || bytes == 0) return rc;
    HIP_TRY(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_gibbs_download(viprs_state* S, int which, void* host) {
    int rc = gibbs_state_check(S, "Gibbs download");
    if (rc != VIPRS_OK) return rc;
    if (which < 0 || which >= VIPRS_GIBBS_BUFFER_COUNT) return fail(VIPRS_EINVAL, "bad Gibbs buffer code");
    if (!host) return fail(VIPRS_EINVAL, "host buffer is null");
    void* p = nullptr;
    size_t bytes = 0;
    rc = gibbs_buffer(S, which, &p, &bytes);
    if (rc != VIPRS_OK || bytes == 0) return rc;
    HIP_TRY(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return check_device_error(S->plan);
}

int viprs_plan_last_gibbs_draws_ms(viprs_plan* P, double* ms) {
    if (!P || !ms) return fail(VIPRS_EINVAL, "null argument");
    return P->time_gibbs_draws.elapsed(P->device, ms, "no timed Gibbs draws call yet");
}

}  // extern "C"
