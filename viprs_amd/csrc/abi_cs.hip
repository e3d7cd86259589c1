// C ABI, PRS-CS (include/viprs_hip.h): the half of the sampler the Gibbs sweep does not do.  After every sweep each SNP of
// each chain takes a new local scale psi from a generalised inverse Gaussian -- for a = 1, b = 1/2 a closed form in one
// normal and one uniform --, and the three E-step inputs of viprs_state_gibbs_sweep are rewritten from it.  The variates
// kernel (one Philox4x32-10 block per (SNP, column), float32), the update kernel (float64, every operation separately
// rounded: the translation unit is built with -ffp-contract=off), the state's six cs buffers and their upload / download.
// The sums are viprs_state_cs_sums (abi_state.hip: the row reductions live there).
#include "internal.h"
#include "philox.h"

#include <cmath>

using namespace viprs;

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace {

constexpr int kCsBlock = 256;
constexpr double kPsiMin = 0x1p-40;

// Thread t of the grid-stride walk takes element i = t, t + threads, ... of the n x m rectangle: the column of row i / m of
// `rows` ((column, sigma2, phi) triples), SNP i % m.  Every access lands inside column g < width of the (m, width) buffers
// (the entry points have checked the rows; the kernels check again).  `cs`: the six buffers, `plane` = m * width apart.
__global__ __launch_bounds__(kCsBlock) void cs_variates_kernel(int64_t m, int width, const double* __restrict__ rows, int n,
                                                               uint32_t k0, uint32_t k1, uint32_t d_lo, uint32_t d_hi,
                                                               float* __restrict__ cs, int64_t plane) {
    const int64_t total = m * n;
    for (int64_t i = (int64_t)blockIdx.x * kCsBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kCsBlock) {
        const int g = (int)rows[3 * (i / m)];
        const int64_t j = i % m;
        if (g < 0 || g >= width) continue;
        uint32_t c[4] = {(uint32_t)j, (uint32_t)g | 0x80000000u, d_lo, d_hi};
        philox4x32_10(c, k0, k1);
        const float u1 = open_unit(c[1]), u2 = open_unit(c[2]), u3 = open_unit(c[3]);
        const float t = -2.0f * logf(u1);
        const float r = sqrtf(t);
        const float a = 2.0f * u2;
        const int64_t at = (int64_t)g * m + j;
        cs[VIPRS_CS_UB * plane + at] = open_unit(c[0]);
        cs[VIPRS_CS_Z1 * plane + at] = r * cospif(a);
        cs[VIPRS_CS_Z2 * plane + at] = r * sinpif(a);
        cs[VIPRS_CS_E * plane + at] = -logf(u3);
    }
}

__global__ __launch_bounds__(kCsBlock) void cs_update_kernel(int64_t m, int width, const double* __restrict__ rows, int n,
                                                             double psi_max, int prepare_only, const double* __restrict__ n_snp,
                                                             const float* __restrict__ eta, float* __restrict__ cs, int64_t plane,
                                                             float* __restrict__ mu_mult, float* __restrict__ hvt,
                                                             float* __restrict__ u_logs) {
    const int64_t total = m * n;
    for (int64_t i = (int64_t)blockIdx.x * kCsBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kCsBlock) {
        const int64_t row = i / m, j = i % m;
        const int g = (int)rows[3 * row];
        if (g < 0 || g >= width) continue;
        const double sigma2 = rows[3 * row + 1], phi = rows[3 * row + 2];
        const int64_t at = (int64_t)g * m + j;
        const double nj = n_snp[j];
        float psi32 = cs[VIPRS_CS_PSI * plane + at];
        if (!prepare_only) {
            const double ub = (double)cs[VIPRS_CS_UB * plane + at], z1 = (double)cs[VIPRS_CS_Z1 * plane + at];
            const double z2 = (double)cs[VIPRS_CS_Z2 * plane + at], e = (double)cs[VIPRS_CS_E * plane + at];
            const double g15 = 0.5 * z2 * z2 + e;
            const double delta = g15 / ((double)psi32 + phi);
            const double lam = 2.0 * delta;
            const double s = fabs((double)eta[at]) * sqrt(nj / (lam * sigma2));
            const double y = z1 * z1;
            const double A = s + (y + sqrt(y * (4.0 * lam * s + y))) / (2.0 * lam);
            double psi = (ub * (A + s) <= A) ? A : s * s / A;
            psi = psi < kPsiMin ? kPsiMin : psi;                 // (comparisons: a NaN stays a NaN)
            psi = psi > psi_max ? psi_max : psi;
            psi32 = (float)psi;
            cs[VIPRS_CS_PSI * plane + at] = psi32;
            cs[VIPRS_CS_DELTA * plane + at] = (float)delta;
        }
        const double p = (double)psi32;
        mu_mult[at] = (float)(p / (1.0 + p));
        hvt[at] = (float)(nj * (1.0 + 1.0 / p) / (2.0 * sigma2));
        u_logs[at] = 32.0f;
    }
}

unsigned walk_grid(int64_t total) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + kCsBlock - 1) / kCsBlock, 8192));
}

// the (column, sigma2, phi) rows of a call on the device (S->d_cs_rows); the stream is synchronised: the caller's array is free
int cs_upload_rows(viprs_state* S, const double* rows, int n) {
    HIP_TRY(hipSetDevice(S->plan->device));
    if (S->d_cs_rows.n < (size_t)3 * n) {
        HIP_TRY(hipStreamSynchronize(S->plan->stream));          // nothing in flight reads the old table
        HIP_TRY(S->d_cs_rows.alloc((size_t)3 * std::max(n, S->width)));
    }
    HIP_TRY(hipMemcpyAsync(S->d_cs_rows.p, rows, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int cs_enqueue_variates(viprs_state* S, uint64_t seed, uint64_t draw_index, int n) {
    viprs_plan* P = S->plan;
    const int64_t total = P->m * n;
    if (total == 0) return VIPRS_OK;
    int rc = P->time_cs_variates.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    cs_variates_kernel<<<walk_grid(total), kCsBlock, 0, P->stream>>>(
        P->m, S->width, S->d_cs_rows.p, n, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw_index,
        (uint32_t)(draw_index >> 32), S->d_cs.p, (int64_t)P->m * S->width);
    HIP_TRY(hipGetLastError());
    return P->time_cs_variates.stop(P->stream);
}

// distinct columns of the state in column 0 of the `stride`-wide rows
int cs_columns_check(const viprs_state* S, const double* rows, int n, int stride) {
    if (n < 0 || n > S->width) return fail(VIPRS_EINVAL, "PRS-CS: bad column count");
    std::vector<char> seen((size_t)S->width, 0);
    for (int i = 0; i < n; ++i) {
        const double c = rows[(size_t)stride * i];
        if (!(c >= 0 && c < S->width) || c != std::floor(c)) return fail(VIPRS_EINVAL, "PRS-CS: column out of range");
        if (seen[(size_t)c]) return fail(VIPRS_EINVAL, "PRS-CS: a column is listed twice");
        seen[(size_t)c] = 1;
    }
    return VIPRS_OK;
}

}  // namespace

namespace viprs {

int cs_state_check(const viprs_state* S, const char* what) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    const std::string w = std::string("PRS-CS ") + what;
    if (S->model_kind != VIPRS_MODEL_GRID)
        return fail(VIPRS_EINVAL, w + ": a state of kind VIPRS_MODEL_GRID is needed (spike-and-slab-kind and mixture states "
                                      "are refused)");
    if (S->float_dtype != VIPRS_F32) return fail(VIPRS_EINVAL, w + ": float64 states are not supported");
    if (!S->group_cols_h.empty()) return fail(VIPRS_EINVAL, w + ": a grid state under a (group, column) mask is not supported");
    if (S->comm) return fail(VIPRS_EINVAL, w + ": a state with a communicator is not supported (several ranks: not built)");
    return VIPRS_OK;
}

int cs_ensure_buffers(viprs_state* S) {
    const size_t plane = (size_t)S->plan->m * (size_t)S->width;
    if (S->d_cs.p || plane == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(S->plan->device));
    HIP_TRY(S->d_cs.alloc(VIPRS_CS_BUFFER_COUNT * plane));
    static_assert(VIPRS_CS_PSI == 0, "psi is the first plane");
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(S->d_cs.p), 0x3F800000, plane, S->plan->stream));   // 1.0f
    HIP_TRY(hipMemsetAsync(S->d_cs.p + plane, 0, (VIPRS_CS_BUFFER_COUNT - 1) * plane * sizeof(float), S->plan->stream));
    return VIPRS_OK;
}

}  // namespace viprs

extern "C" {

int viprs_state_cs_variates(viprs_state* S, uint64_t seed, uint64_t draw_index, const int32_t* active, int n_active) {
    int rc = cs_state_check(S, "variates");
    if (rc != VIPRS_OK) return rc;
    if (!active) n_active = S->width;
    std::vector<double> rows((size_t)3 * std::max(n_active, 0), 0.0);
    for (int i = 0; i < n_active; ++i) rows[(size_t)3 * i] = active ? (double)active[i] : (double)i;
    rc = cs_columns_check(S, rows.data(), n_active, 3);
    if (rc != VIPRS_OK) return rc;
    if (n_active == 0 || S->plan->m == 0) return VIPRS_OK;
    rc = cs_ensure_buffers(S);
    if (rc != VIPRS_OK) return rc;
    rc = cs_upload_rows(S, rows.data(), n_active);
    if (rc != VIPRS_OK) return rc;
    rc = cs_enqueue_variates(S, seed, draw_index, n_active);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_cs_update(viprs_state* S, int n, const double* params, double psi_max, uint64_t seed, uint64_t draw_index,
                          int flags, int sync) {
    int rc = cs_state_check(S, "update");
    if (rc != VIPRS_OK) return rc;
    if (!params) return fail(VIPRS_EINVAL, "PRS-CS update: params is null");
    if (flags & ~(VIPRS_CS_KEEP_VARIATES | VIPRS_CS_PREPARE_ONLY)) return fail(VIPRS_EINVAL, "PRS-CS update: unknown flag");
    if (!(psi_max > kPsiMin) || !std::isfinite(psi_max)) return fail(VIPRS_EINVAL, "PRS-CS update: psi_max must lie in (2^-40, inf)");
    rc = cs_columns_check(S, params, n, 3);
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const double sigma2 = params[3 * i + 1], phi = params[3 * i + 2];
        if (!(sigma2 > 0) || !std::isfinite(sigma2)) return fail(VIPRS_EINVAL, "PRS-CS update: sigma2 must be positive and finite");
        if (!(phi > 0) || !std::isfinite(phi)) return fail(VIPRS_EINVAL, "PRS-CS update: phi must be positive and finite");
    }
    viprs_plan* P = S->plan;
    const bool prepare = (flags & VIPRS_CS_PREPARE_ONLY) != 0, keep = (flags & VIPRS_CS_KEEP_VARIATES) != 0;
    if (P->m > 0 && !S->d_n.p) return fail(VIPRS_EINVAL, "PRS-CS update: viprs_state_set_n_per_snp has not been called");
    if (keep && !prepare && !S->d_cs.p && P->m > 0)
        return fail(VIPRS_EINVAL, "PRS-CS update: VIPRS_CS_KEEP_VARIATES before the cs buffers exist (no cs call yet)");
    if (n == 0 || P->m == 0) return VIPRS_OK;
    rc = cs_ensure_buffers(S);
    if (rc != VIPRS_OK) return rc;
    rc = cs_upload_rows(S, params, n);
    if (rc != VIPRS_OK) return rc;
    if (!prepare && !keep) {
        rc = cs_enqueue_variates(S, seed, draw_index, n);
        if (rc != VIPRS_OK) return rc;
    }
    const int64_t total = P->m * n;
    rc = P->time_cs_update.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    cs_update_kernel<<<walk_grid(total), kCsBlock, 0, P->stream>>>(
        P->m, S->width, S->d_cs_rows.p, n, psi_max, prepare ? 1 : 0, S->d_n.p, (const float*)S->f[VIPRS_FIELD_ETA].p, S->d_cs.p,
        (int64_t)P->m * S->width, (float*)S->f[VIPRS_FIELD_MU_MULT].p, (float*)S->f[VIPRS_FIELD_SQRT_HALF_VAR_TAU].p,
        (float*)S->f[VIPRS_FIELD_U_LOGS].p);
    HIP_TRY(hipGetLastError());
    rc = P->time_cs_update.stop(P->stream);
    if (rc != VIPRS_OK) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(P->stream));
    return VIPRS_OK;
}

static int cs_transfer(viprs_state* S, int which, void* host, bool up) {
    int rc = cs_state_check(S, up ? "upload" : "download");
    if (rc != VIPRS_OK) return rc;
    if (which < 0 || which >= VIPRS_CS_BUFFER_COUNT) return fail(VIPRS_EINVAL, "PRS-CS: bad buffer code");
    if (!host) return fail(VIPRS_EINVAL, "PRS-CS: host buffer is null");
    const size_t plane = (size_t)S->plan->m * (size_t)S->width;
    if (plane == 0) return VIPRS_OK;
    rc = cs_ensure_buffers(S);
    if (rc != VIPRS_OK) return rc;
    float* d = S->d_cs.p + (size_t)which * plane;
    hipStream_t st = S->plan->stream;
    if (up) HIP_TRY(hipMemcpyAsync(d, host, plane * sizeof(float), hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpyAsync(host, d, plane * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return up ? VIPRS_OK : check_device_error(S->plan);
}

int viprs_state_cs_upload(viprs_state* S, int which, const void* host) { return cs_transfer(S, which, const_cast<void*>(host), true); }
int viprs_state_cs_download(viprs_state* S, int which, void* host) { return cs_transfer(S, which, host, false); }

int viprs_plan_last_cs_ms(viprs_plan* P, double* variates_ms, double* update_ms) {
    if (!P || !variates_ms || !update_ms) return fail(VIPRS_EINVAL, "null argument");
    if (!P->time_cs_variates.timed && !P->time_cs_update.timed) return fail(VIPRS_EINVAL, "no timed PRS-CS call yet");
    double v = 0.0, u = 0.0;                             // (a kernel that has not run yet reports 0)
    int rc = P->time_cs_variates.timed ? P->time_cs_variates.elapsed(P->device, &v, "") : VIPRS_OK;
    if (rc != VIPRS_OK) return rc;
    rc = P->time_cs_update.timed ? P->time_cs_update.elapsed(P->device, &u, "") : VIPRS_OK;
    if (rc != VIPRS_OK) return rc;
    *variates_ms = v;
    *update_ms = u;
    return VIPRS_OK;
}

}  // extern "C"
