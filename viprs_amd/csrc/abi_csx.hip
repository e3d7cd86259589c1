// C ABI, PRS-CSx (include/viprs_hip.h): P PRS-CS chains, one per population and each a grid state on a plan of its own, coupled
// through ONE local scale psi per SNP of the union of their SNP sets.  The per-population half is viprs_state_gibbs_sweep,
// untouched; this translation unit is the other half: one pass over the union that gathers eta from the P states, draws delta
// and psi -- K = 1 carrying population: the closed form of abi_cs.hip, operation for operation; K >= 2: GIG(1 - K/2, 2 delta, B)
// by Devroye's (2014) rejection sampler in float64, at most 32 attempts, one Philox block per attempt -- and scatters psi,
// delta and the three sweep inputs back into the P states.  Built with -ffp-contract=off: every operation separately rounded.
#include "internal.h"
#include "philox.h"

#include <cmath>

using namespace viprs;

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

struct viprs_csx {
    int n_pop = 0, width = 0, device = 0;
    int64_t m_union = 0;
    std::vector<viprs_state*> states;
    DevBuf<int64_t> d_row_of;                      // (n_pop, m_union)
    DevBuf<float> d_shared;                        // psi, then delta: (m_union, G) each, column-major
    DevBuf<uint8_t> d_attempts;                    // (m_union, G)
    DevBuf<double> d_rows;                         // the (column, phi, sigma2_0 .. sigma2_{P-1}) rows of the call in flight
    DevBuf<unsigned long long> d_capped;           // draws of the last update that ended at the attempt cap
    DevBuf<double> d_partials, d_sums;             // viprs_csx_sums
    DevBuf<int32_t> d_cols;
    EventBracket time;                             // the update kernel, on the stream of population 0
    std::vector<DevEvent> ev_member;               // one per population: its stream up to the update
    DevEvent ev_done;                              // the update: every member stream waits for it
    bool updated = false;
};

namespace {

constexpr int kCsxBlock = 256;
constexpr int kCsxMaxPop = VIPRS_CSX_MAX_POP;
constexpr int kCsxAttempts = VIPRS_CSX_MAX_ATTEMPTS;
constexpr double kPsiMin = 0x1p-40;
// cosh(1), exp(1), exp(-1) rounded to float64: the breakpoint rule evaluates psi(+-1) from them
constexpr double kCosh1 = 0x1.8b07551d9f55p+0, kExp1 = 0x1.5bf0a8b145769p+1, kExpM1 = 0x1.78b56362cef38p-2;

// what the kernel reads and writes of one population (device pointers of its state; plane = m_k * G)
struct CsxMember {
    const float* eta;
    const double* n_snp;
    float* cs;
    float* mu_mult;
    float* hvt;
    float* u_logs;
    int64_t m;
};
struct CsxMembers {
    CsxMember p[kCsxMaxPop];
};

// psi(x) = -alpha (cosh x - 1) - lambda (exp x - x - 1) and its derivative (Devroye 2014, section 5)
__device__ __forceinline__ double gig_psi(double x, double alpha, double lambda) {
    return -alpha * (cosh(x) - 1.0) - lambda * (exp(x) - x - 1.0);
}
__device__ __forceinline__ double gig_dpsi(double x, double alpha, double lambda) {
    return -alpha * sinh(x) - lambda * (exp(x) - 1.0);
}

// Thread t of the grid-stride walk takes element i = t, t + threads, ... of the n x m_union rectangle: the column of row
// i / m_union of `rows` (stride 2 + n_pop), union SNP i % m_union.  Every access lands inside column g < width of the (m, width)
// buffers and at a row r < m_k that viprs_csx_create has checked.
__global__ __launch_bounds__(kCsxBlock) void csx_update_kernel(
    int64_t mu, int width, int n_pop, const double* __restrict__ rows, int n, double psi_max, int prepare_only, int keep,
    uint32_t k0, uint32_t k1, uint32_t d_lo, uint32_t d_hi, const int64_t* __restrict__ row_of, CsxMembers M,
    float* __restrict__ shared, uint8_t* __restrict__ attempts, unsigned long long* __restrict__ capped) {
    const int stride = 2 + n_pop;
    const int64_t total = mu * n, splane = mu * width;
    for (int64_t i = (int64_t)blockIdx.x * kCsxBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kCsxBlock) {
        const int64_t row = i / mu, u = i % mu;
        const double* par = rows + (int64_t)stride * row;
        const int g = (int)par[0];
        if (g < 0 || g >= width) continue;
        const double phi = par[1];
        const int64_t at = (int64_t)g * mu + u;
        float psi32 = shared[at], delta32 = shared[splane + at];
        if (!prepare_only) {
            // the carrying populations: K, B, and what the closed form takes from the first of them
            int K = 0, k_first = 0;
            int64_t r_first = 0;
            double B = 0.0;
            for (int k = 0; k < n_pop; ++k) {
                const int64_t r = row_of[(int64_t)k * mu + u];
                if (r < 0) continue;
                const double e = (double)M.p[k].eta[(int64_t)g * M.p[k].m + r];
                B = B + M.p[k].n_snp[r] * e * e / par[2 + k];
                if (K == 0) { k_first = k; r_first = r; }
                ++K;
            }
            float ubf, z1f, z2f, ef;
            if (keep) {
                const float* cs = M.p[k_first].cs;
                const int64_t plane = M.p[k_first].m * width, a1 = (int64_t)g * M.p[k_first].m + r_first;
                ubf = cs[VIPRS_CS_UB * plane + a1];
                z1f = cs[VIPRS_CS_Z1 * plane + a1];
                z2f = cs[VIPRS_CS_Z2 * plane + a1];
                ef = cs[VIPRS_CS_E * plane + a1];
            } else {
                uint32_t c[4] = {(uint32_t)u, (uint32_t)g | 0x80000000u, d_lo, d_hi};
                philox4x32_10(c, k0, k1);
                const float u1 = open_unit(c[1]), u2 = open_unit(c[2]), u3 = open_unit(c[3]);
                const float t = -2.0f * logf(u1);
                const float rr = sqrtf(t);
                const float a = 2.0f * u2;
                ubf = open_unit(c[0]);
                z1f = rr * cospif(a);
                z2f = rr * sinpif(a);
                ef = -logf(u3);
            }
            const double ub = (double)ubf, z1 = (double)z1f, z2 = (double)z2f, e = (double)ef;
            const double g15 = 0.5 * z2 * z2 + e;
            const double delta = g15 / ((double)psi32 + phi);
            const double lam = 2.0 * delta;
            double psi;
            int tries = 0;
            if (K == 1) {
                const double eta1 = (double)M.p[k_first].eta[(int64_t)g * M.p[k_first].m + r_first];
                const double s = fabs(eta1) * sqrt(M.p[k_first].n_snp[r_first] / (lam * par[2 + k_first]));
                const double y = z1 * z1;
                const double A = s + (y + sqrt(y * (4.0 * lam * s + y))) / (2.0 * lam);
                psi = (ub * (A + s) <= A) ? A : s * s / A;
            } else if (B == 0.0) {
                psi = kPsiMin;                                   // improper conditional: the floor, nothing drawn
            } else {
                // set-up, once per draw: breakpoints t, s and the envelope (eta, zeta, theta, xi -> pe, re, td, sd, q)
                const double lambda = 0.5 * (double)K - 1.0;     // |p|, p = 1 - K / 2 <= 0
                const double omega = sqrt(lam * B);
                const double alpha = sqrt(omega * omega + lambda * lambda) - lambda;
                const double al = alpha + lambda;
                double x = alpha * (kCosh1 - 1.0) + lambda * (kExp1 - 1.0 - 1.0);           // -psi(1)
                double t = 1.0;
                if (x > 2.0) t = sqrt(2.0 / al);
                else if (x < 0.5) t = log(4.0 / (alpha + 2.0 * lambda));
                x = alpha * (kCosh1 - 1.0) + lambda * kExpM1;                               // -psi(-1)
                double s = 1.0;
                if (x > 2.0) s = sqrt(4.0 / (alpha * kCosh1 + lambda));
                else if (x < 0.5) {
                    const double ia = 1.0 / alpha;
                    s = log(1.0 + ia + sqrt(ia * ia + 2.0 * ia));
                    if (lambda > 0.0) s = fmin(1.0 / lambda, s);
                }
                const double eta_g = -gig_psi(t, alpha, lambda), zeta = -gig_dpsi(t, alpha, lambda);
                const double theta = -gig_psi(-s, alpha, lambda), xi = gig_dpsi(-s, alpha, lambda);
                const double pe = 1.0 / xi, re = 1.0 / zeta;
                const double td = t - re * eta_g, sd = s - pe * theta;
                const double q = td + sd;
                const double norm = pe + q + re;
                const double cut1 = q / norm, cut2 = (q + re) / norm;
                bool accepted = false;
                for (int a = 0; a < kCsxAttempts && !accepted; ++a) {
                    uint32_t c[4] = {(uint32_t)u, (uint32_t)g | 0x80000000u | ((uint32_t)(a + 1) << 16), d_lo, d_hi};
                    philox4x32_10(c, k0, k1);
                    const double U = (double)open_unit(c[0]), V = (double)open_unit(c[1]), W = (double)open_unit(c[2]);
                    double gx = 1.0;
                    if (U < cut1) {
                        x = -sd + q * V;
                    } else if (U < cut2) {
                        x = td - re * log(V);
                    } else {
                        x = -sd + pe * log(V);
                    }
                    if (x > td) gx = exp(-eta_g - zeta * (x - t));
                    else if (x < -sd) gx = exp(-theta + xi * (x + s));
                    accepted = W * gx <= exp(gig_psi(x, alpha, lambda));
                    tries = a + 1;
                }
                if (!accepted) atomicAdd(capped, 1ull);          // (the last proposal stands)
                const double lo = lambda / omega;
                psi = exp(x) * (lo + sqrt(1.0 + lo * lo));
                if (K > 2) psi = 1.0 / psi;
                psi = psi / sqrt(lam / B);
            }
            psi = psi < kPsiMin ? kPsiMin : psi;                 // (comparisons: a NaN stays a NaN)
            psi = psi > psi_max ? psi_max : psi;
            psi32 = (float)psi;
            delta32 = (float)delta;
            shared[at] = psi32;
            shared[splane + at] = delta32;
            attempts[at] = (uint8_t)tries;
            if (!keep) {
                for (int k = 0; k < n_pop; ++k) {
                    const int64_t r = row_of[(int64_t)k * mu + u];
                    if (r < 0) continue;
                    float* cs = M.p[k].cs;
                    const int64_t plane = M.p[k].m * width, ak = (int64_t)g * M.p[k].m + r;
                    cs[VIPRS_CS_UB * plane + ak] = ubf;
                    cs[VIPRS_CS_Z1 * plane + ak] = z1f;
                    cs[VIPRS_CS_Z2 * plane + ak] = z2f;
                    cs[VIPRS_CS_E * plane + ak] = ef;
                }
            }
        }
        const double p = (double)psi32;
        const float mm = (float)(p / (1.0 + p));
        const double hv = 1.0 + 1.0 / p;
        for (int k = 0; k < n_pop; ++k) {
            const int64_t r = row_of[(int64_t)k * mu + u];
            if (r < 0) continue;
            const int64_t plane = M.p[k].m * width, ak = (int64_t)g * M.p[k].m + r;
            M.p[k].cs[VIPRS_CS_PSI * plane + ak] = psi32;
            M.p[k].cs[VIPRS_CS_DELTA * plane + ak] = delta32;
            M.p[k].mu_mult[ak] = mm;
            M.p[k].hvt[ak] = (float)(M.p[k].n_snp[r] * hv / (2.0 * par[2 + k]));
            M.p[k].u_logs[ak] = 32.0f;
        }
    }
}

// viprs_csx_sums, stage 1: THE ORDER of a grid state's rows over the union -- workgroup b of nb takes SNPs b * 256 + t,
// + nb * 256, ... serially per thread, then the binary tree in LDS; slot 0 sum delta, slot 1 sum psi
__global__ __launch_bounds__(kCsxBlock) void csx_sums_kernel(int64_t mu, int width, const int32_t* __restrict__ cols,
                                                             const float* __restrict__ shared, double* __restrict__ partials) {
    __shared__ double red[VIPRS_N_CSX_SUMS][kCsxBlock];
    const int g = cols[blockIdx.y], nb = (int)gridDim.x;
    const float* psi = shared + (int64_t)g * mu;
    const float* delta = psi + mu * width;
    double acc[VIPRS_N_CSX_SUMS] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kCsxBlock + threadIdx.x; i < mu; i += (int64_t)nb * kCsxBlock) {
        acc[0] += (double)delta[i];
        acc[1] += (double)psi[i];
    }
#pragma unroll
    for (int k = 0; k < VIPRS_N_CSX_SUMS; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = kCsxBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < VIPRS_N_CSX_SUMS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < VIPRS_N_CSX_SUMS)
        partials[((int64_t)blockIdx.y * nb + blockIdx.x) * VIPRS_N_CSX_SUMS + threadIdx.x] = red[threadIdx.x][0];
}

// stage 2: workgroup (k, y) is one wave adding sum k over the nb partials of row y -- lane l adds partials l, l + 64, ... in
// order, then the xor-shuffle tree (the order of the final pass of every sums call of the library)
__global__ void csx_sums_final_kernel(const double* __restrict__ partials, int nb, double* __restrict__ out) {
    partials += (int64_t)blockIdx.y * nb * VIPRS_N_CSX_SUMS;
    const int k = blockIdx.x, lane = threadIdx.x;
    double a = 0.0;
    for (int b = lane; b < nb; b += 64) a = a + partials[(int64_t)b * VIPRS_N_CSX_SUMS + k];
    for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off, 64);
    if (lane == 0) out[(int64_t)blockIdx.y * VIPRS_N_CSX_SUMS + k] = a;
}

unsigned walk_grid(int64_t total) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + kCsxBlock - 1) / kCsxBlock, 8192));
}

int csx_check(const viprs_csx* X) { return X ? VIPRS_OK : fail(VIPRS_EINVAL, "PRS-CSx: null coupling handle"); }

hipStream_t csx_stream(const viprs_csx* X) { return X->states[0]->plan->stream; }

// distinct columns of the handle in column 0 of the `stride`-wide rows
int csx_columns_check(const viprs_csx* X, const double* rows, int n, int stride) {
    if (n < 0 || n > X->width) return fail(VIPRS_EINVAL, "PRS-CSx: bad column count");
    std::vector<char> seen((size_t)X->width, 0);
    for (int i = 0; i < n; ++i) {
        const double c = rows[(size_t)stride * i];
        if (!(c >= 0 && c < X->width) || c != std::floor(c)) return fail(VIPRS_EINVAL, "PRS-CSx: column out of range");
        if (seen[(size_t)c]) return fail(VIPRS_EINVAL, "PRS-CSx: a column is listed twice");
        seen[(size_t)c] = 1;
    }
    return VIPRS_OK;
}

}  // namespace

extern "C" {

int viprs_csx_create(viprs_csx** out, int n_pop, viprs_state* const* states, int64_t m_union, const int64_t* row_of) {
    if (!out) return fail(VIPRS_EINVAL, "PRS-CSx create: null argument");
    *out = nullptr;
    if (n_pop < 1 || n_pop > kCsxMaxPop) return fail(VIPRS_EINVAL, "PRS-CSx create: n_pop must lie in 1..8");
    if (!states || !row_of) return fail(VIPRS_EINVAL, "PRS-CSx create: null argument");
    if (m_union < 0) return fail(VIPRS_EINVAL, "PRS-CSx create: m_union is negative");
    for (int k = 0; k < n_pop; ++k) {
        int rc = cs_state_check(states[k], "coupling");
        if (rc != VIPRS_OK) return rc;
        const viprs_state* S = states[k];
        if (S->width != states[0]->width) return fail(VIPRS_EINVAL, "PRS-CSx create: the states must have one common width");
        if (S->plan->device != states[0]->plan->device)
            return fail(VIPRS_EINVAL, "PRS-CSx create: the states sit on different devices (not built)");
        if (S->plan->m > 0 && !S->d_n.p)
            return fail(VIPRS_EINVAL, "PRS-CSx create: viprs_state_set_n_per_snp has not been called on every state");
        for (int l = 0; l < k; ++l)
            if (states[l] == S) return fail(VIPRS_EINVAL, "PRS-CSx create: a state is listed twice");
    }
    const int G = states[0]->width;
    if (G >= (1 << 16)) return fail(VIPRS_EINVAL, "PRS-CSx create: the width must be below 2^16 (the attempt index shares the counter word)");
    if (m_union >= ((int64_t)1 << 32)) return fail(VIPRS_EINVAL, "PRS-CSx create: m_union must be below 2^32");
    for (int k = 0; k < n_pop; ++k) {
        const int64_t mk = states[k]->plan->m;
        std::vector<char> seen((size_t)mk, 0);
        for (int64_t u = 0; u < m_union; ++u) {
            const int64_t r = row_of[(int64_t)k * m_union + u];
            if (r == -1) continue;
            if (r < 0 || r >= mk) return fail(VIPRS_EINVAL, "PRS-CSx create: a row index is out of range");
            if (seen[(size_t)r]) return fail(VIPRS_EINVAL, "PRS-CSx create: a row is listed twice within one population");
            seen[(size_t)r] = 1;
        }
    }
    for (int64_t u = 0; u < m_union; ++u) {
        bool carried = false;
        for (int k = 0; k < n_pop && !carried; ++k) carried = row_of[(int64_t)k * m_union + u] >= 0;
        if (!carried) return fail(VIPRS_EINVAL, "PRS-CSx create: a union row is carried by no population");
    }
    std::unique_ptr<viprs_csx> X(new viprs_csx());
    X->n_pop = n_pop;
    X->width = G;
    X->m_union = m_union;
    X->device = states[0]->plan->device;
    X->states.assign(states, states + n_pop);
    X->ev_member.resize((size_t)n_pop);
    HIP_TRY(hipSetDevice(X->device));
    for (auto& e : X->ev_member) HIP_TRY(hipEventCreateWithFlags(&e.e, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&X->ev_done.e, hipEventDisableTiming));
    hipStream_t st = csx_stream(X.get());
    const size_t plane = (size_t)m_union * (size_t)G;
    HIP_TRY(X->d_capped.alloc(1));
    HIP_TRY(hipMemsetAsync(X->d_capped.p, 0, sizeof(unsigned long long), st));
    HIP_TRY(X->d_rows.alloc((size_t)(2 + n_pop) * (size_t)G));
    HIP_TRY(X->d_cols.alloc((size_t)G));
    if (plane > 0) {
        HIP_TRY(X->d_row_of.alloc((size_t)n_pop * (size_t)m_union));
        HIP_TRY(hipMemcpyAsync(X->d_row_of.p, row_of, sizeof(int64_t) * (size_t)n_pop * (size_t)m_union, hipMemcpyHostToDevice, st));
        HIP_TRY(X->d_shared.alloc(2 * plane));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(X->d_shared.p), 0x3F800000, plane, st));          // psi = 1.0f
        HIP_TRY(hipMemsetAsync(X->d_shared.p + plane, 0, plane * sizeof(float), st));
        HIP_TRY(X->d_attempts.alloc(plane));
        HIP_TRY(hipMemsetAsync(X->d_attempts.p, 0, plane, st));
        const int nb = (int)std::min<int64_t>((m_union + kCsxBlock - 1) / kCsxBlock, 256);
        HIP_TRY(X->d_partials.alloc((size_t)nb * (size_t)G * VIPRS_N_CSX_SUMS));
        HIP_TRY(X->d_sums.alloc((size_t)G * VIPRS_N_CSX_SUMS));
    }
    for (int k = 0; k < n_pop; ++k) {
        int rc = cs_ensure_buffers(states[k]);
        if (rc != VIPRS_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));                           // the caller's row_of is free
    *out = X.release();
    return VIPRS_OK;
}

int viprs_csx_destroy(viprs_csx* X) {
    if (!X) return VIPRS_OK;
    (void)hipSetDevice(X->device);
    (void)hipDeviceSynchronize();
    delete X;
    return VIPRS_OK;
}

int viprs_csx_update(viprs_csx* X, int n, const double* params, double psi_max, uint64_t seed, uint64_t draw_index, int flags,
                     int sync) {
    int rc = csx_check(X);
    if (rc != VIPRS_OK) return rc;
    if (!params) return fail(VIPRS_EINVAL, "PRS-CSx update: params is null");
    if (flags & ~(VIPRS_CS_KEEP_VARIATES | VIPRS_CS_PREPARE_ONLY)) return fail(VIPRS_EINVAL, "PRS-CSx update: unknown flag");
    if (!(psi_max > kPsiMin) || !std::isfinite(psi_max)) return fail(VIPRS_EINVAL, "PRS-CSx update: psi_max must lie in (2^-40, inf)");
    const int P = X->n_pop, stride = 2 + P;
    rc = csx_columns_check(X, params, n, stride);
    if (rc != VIPRS_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const double phi = params[(size_t)stride * i + 1];
        if (!(phi > 0) || !std::isfinite(phi)) return fail(VIPRS_EINVAL, "PRS-CSx update: phi must be positive and finite");
        for (int k = 0; k < P; ++k) {
            const double sigma2 = params[(size_t)stride * i + 2 + k];
            if (!(sigma2 > 0) || !std::isfinite(sigma2)) return fail(VIPRS_EINVAL, "PRS-CSx update: sigma2 must be positive and finite");
        }
    }
    CsxMembers M;
    for (int k = 0; k < kCsxMaxPop; ++k) M.p[k] = CsxMember{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    for (int k = 0; k < P; ++k) {
        viprs_state* S = X->states[k];
        rc = cs_state_check(S, "coupled update");
        if (rc != VIPRS_OK) return rc;
        if (S->plan->m > 0 && !S->d_n.p) return fail(VIPRS_EINVAL, "PRS-CSx update: viprs_state_set_n_per_snp has not been called");
        rc = cs_ensure_buffers(S);
        if (rc != VIPRS_OK) return rc;
        M.p[k] = CsxMember{(const float*)S->f[VIPRS_FIELD_ETA].p, S->d_n.p, S->d_cs.p, (float*)S->f[VIPRS_FIELD_MU_MULT].p,
                           (float*)S->f[VIPRS_FIELD_SQRT_HALF_VAR_TAU].p, (float*)S->f[VIPRS_FIELD_U_LOGS].p, S->plan->m};
    }
    const int64_t total = X->m_union * n;
    if (total == 0) return VIPRS_OK;
    const bool prepare = (flags & VIPRS_CS_PREPARE_ONLY) != 0, keep = (flags & VIPRS_CS_KEEP_VARIATES) != 0;
    HIP_TRY(hipSetDevice(X->device));
    hipStream_t st = csx_stream(X);
    // the rows of the call: the previous update that read the table has been waited for below (the copy is ordered on `st`)
    HIP_TRY(hipMemcpyAsync(X->d_rows.p, params, sizeof(double) * (size_t)stride * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                           // the caller's array is free
    // the update reads eta of every member: it waits for what every member stream has been given so far
    for (int k = 1; k < P; ++k) {
        hipStream_t sk = X->states[k]->plan->stream;
        if (sk == st) continue;
        HIP_TRY(hipEventRecord(X->ev_member[(size_t)k].e, sk));
        HIP_TRY(hipStreamWaitEvent(st, X->ev_member[(size_t)k].e, 0));
    }
    HIP_TRY(hipMemsetAsync(X->d_capped.p, 0, sizeof(unsigned long long), st));
    rc = X->time.start(st);
    if (rc != VIPRS_OK) return rc;
    csx_update_kernel<<<walk_grid(total), kCsxBlock, 0, st>>>(
        X->m_union, X->width, P, X->d_rows.p, n, psi_max, prepare ? 1 : 0, keep ? 1 : 0, (uint32_t)seed, (uint32_t)(seed >> 32),
        (uint32_t)draw_index, (uint32_t)(draw_index >> 32), X->d_row_of.p, M, X->d_shared.p, X->d_attempts.p, X->d_capped.p);
    HIP_TRY(hipGetLastError());
    rc = X->time.stop(st);
    if (rc != VIPRS_OK) return rc;
    X->updated = true;
    // ... and every member stream waits for the update before whatever it is given next (its next sweep)
    HIP_TRY(hipEventRecord(X->ev_done.e, st));
    for (int k = 1; k < P; ++k) {
        hipStream_t sk = X->states[k]->plan->stream;
        if (sk != st) HIP_TRY(hipStreamWaitEvent(sk, X->ev_done.e, 0));
    }
    if (sync) HIP_TRY(hipStreamSynchronize(st));
    return VIPRS_OK;
}

int viprs_csx_sums(viprs_csx* X, int n, const int32_t* cols, double* out) {
    int rc = csx_check(X);
    if (rc != VIPRS_OK) return rc;
    if (!out) return fail(VIPRS_EINVAL, "PRS-CSx sums: out is null");
    if (n < 0 || n > X->width) return fail(VIPRS_EINVAL, "PRS-CSx sums: bad column count");
    if (!cols && n != X->width) return fail(VIPRS_EINVAL, "PRS-CSx sums: cols == NULL lists every column: n must be the handle's width");
    std::vector<int32_t> list((size_t)n);
    std::vector<char> seen((size_t)X->width, 0);
    for (int i = 0; i < n; ++i) {
        list[(size_t)i] = cols ? cols[i] : i;
        if (list[(size_t)i] < 0 || list[(size_t)i] >= X->width) return fail(VIPRS_EINVAL, "PRS-CSx sums: column out of range");
        if (seen[(size_t)list[(size_t)i]]) return fail(VIPRS_EINVAL, "PRS-CSx sums: a column is listed twice");
        seen[(size_t)list[(size_t)i]] = 1;
    }
    for (int k = 0; k < n * VIPRS_N_CSX_SUMS; ++k) out[k] = 0.0;
    if (n == 0 || X->m_union == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(X->device));
    hipStream_t st = csx_stream(X);
    const int nb = (int)std::min<int64_t>((X->m_union + kCsxBlock - 1) / kCsxBlock, 256);     // THE ORDER of a grid state's rows
    HIP_TRY(hipMemcpyAsync(X->d_cols.p, list.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    csx_sums_kernel<<<dim3((unsigned)nb, (unsigned)n), kCsxBlock, 0, st>>>(X->m_union, X->width, X->d_cols.p, X->d_shared.p,
                                                                           X->d_partials.p);
    HIP_TRY(hipGetLastError());
    csx_sums_final_kernel<<<dim3(VIPRS_N_CSX_SUMS, (unsigned)n), 64, 0, st>>>(X->d_partials.p, nb, X->d_sums.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, X->d_sums.p, sizeof(double) * (size_t)n * VIPRS_N_CSX_SUMS, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VIPRS_OK;
}

static int csx_transfer(viprs_csx* X, int which, void* host, bool up) {
    int rc = csx_check(X);
    if (rc != VIPRS_OK) return rc;
    if (which < 0 || which >= VIPRS_CSX_BUFFER_COUNT) return fail(VIPRS_EINVAL, "PRS-CSx: bad buffer code");
    if (!host) return fail(VIPRS_EINVAL, "PRS-CSx: host buffer is null");
    const size_t plane = (size_t)X->m_union * (size_t)X->width;
    if (plane == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(X->device));
    hipStream_t st = csx_stream(X);
    void* d = which == VIPRS_CSX_ATTEMPTS ? (void*)X->d_attempts.p : (void*)(X->d_shared.p + (size_t)which * plane);
    const size_t bytes = which == VIPRS_CSX_ATTEMPTS ? plane : plane * sizeof(float);
    if (up) HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VIPRS_OK;
}

int viprs_csx_upload(viprs_csx* X, int which, const void* host) { return csx_transfer(X, which, const_cast<void*>(host), true); }
int viprs_csx_download(viprs_csx* X, int which, void* host) { return csx_transfer(X, which, host, false); }

int viprs_csx_last(viprs_csx* X, double* ms, int64_t* n_capped) {
    int rc = csx_check(X);
    if (rc != VIPRS_OK) return rc;
    if (!ms || !n_capped) return fail(VIPRS_EINVAL, "PRS-CSx: null argument");
    if (!X->updated) return fail(VIPRS_EINVAL, "no timed PRS-CSx update yet");
    double t = 0.0;
    rc = X->time.elapsed(X->device, &t, "no timed PRS-CSx update yet");
    if (rc != VIPRS_OK) return rc;
    unsigned long long c = 0;
    HIP_TRY(hipMemcpyAsync(&c, X->d_capped.p, sizeof(c), hipMemcpyDeviceToHost, csx_stream(X)));
    HIP_TRY(hipStreamSynchronize(csx_stream(X)));
    *ms = t;
    *n_capped = (int64_t)c;
    return VIPRS_OK;
}

}  // extern "C"
