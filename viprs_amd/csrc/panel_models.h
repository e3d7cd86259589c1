// Model policies of the panel scheme: what one SNP update computes for the spike-and-slab, grid-column and mixture
// E-steps (estep_panel.h, estep_band.h).
#pragma once
#include <type_traits>

#include "device_math.h"
#include "kernels_common.h"
#include "panel_loads.h"       // stage_store

namespace viprs {

// ---------------------------------------------------------------------------------------------
// Model policies: what one SNP update computes (the serial chain evaluates `update` with the
// lane-select table lookup; after the 64 steps every lane replays its own SNP with the per-lane
// lookup -- same operations, same inputs, same bits -- and `finish` stores the outputs).
//   load    per-SNP inputs of SNP j (lane-resident for a whole panel)
//   update  d = new eta - old eta from the current q[j];  returns false on the skip branch
//   finish  replay + stores; returns the scaled eta_diff (0 for skipped SNPs)
// ---------------------------------------------------------------------------------------------
template <bool EXACT>
struct SpikeSlabModel {                      // e_step, e_step.hpp:387-433
    static constexpr bool kLaneParallel = false;
    struct In { float mm, beta, sv, ulog, eta_old; };
    static __device__ __forceinline__ In load(const EStepArgs<float>& A, int64_t j, bool live) {
        In in;
        in.mm = live ? A.mu_mult[j] : 0.0f;
        in.beta = live ? A.std_beta[j] : 0.0f;
        in.sv = live ? A.shvt[j] : 0.0f;
        in.ulog = live ? A.u_logs[j] : 0.0f;
        in.eta_old = live ? A.eta[j] : 0.0f;
        return in;
    }
    static constexpr bool kHasSkip = true;     // e_step.hpp:410-413
    // d = new eta - old eta of the lane's SNP from the current q (no skip handling)
    template <int LOOKUP>
    static __device__ __forceinline__ float delta(const In& in, float q, const ExpTab& tab, int sel) {
        float mu, gamma, d;
        snp_update<EXACT, LOOKUP>(in.mm, in.beta, in.sv, in.ulog, in.eta_old, q, tab, mu, gamma, d, sel);
        return d;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ bool update(const In& in, float q, const ExpTab& tab, float& d, int sel) {
        d = delta<LOOKUP>(in, q, tab, sel);
        return !(fabsf(d) < Eps<float>::value);                       // :410
    }
    template <bool TEAM>
    static __device__ __forceinline__ float finish(const EStepArgs<float>& A, int64_t j, const In& in, float q,
                                                   const ExpTab& tab, bool live, bool writer, bool& skipped,
                                                   float* d_out = nullptr) {
        float mu, gamma, d;
        snp_update<EXACT, kLookupPerLane>(in.mm, in.beta, in.sv, in.ulog, in.eta_old, q, tab, mu, gamma, d);
        const bool skip = fabsf(d) < Eps<float>::value;
        if (live && writer) {
            if (!skip) {
                A.var_mu[j] = mu;                                         // :416-418
                A.var_gamma[j] = gamma;
                A.eta_diff[j] = d;
                if (!TEAM) A.eta[j] = in.eta_old + d;                     // :431
            } else {
                A.eta_diff[j] = 0.0f;                                     // :412
            }
            if (TEAM) stage_store(A.eta_out + j, skip ? in.eta_old : in.eta_old + d);
        }
        skipped = live && skip;
        if (d_out) *d_out = (live && !skip) ? d : 0.0f;
        return (live && !skip) ? A.dq * d : 0.0f;
    }
};

// One column of e_step_grid (e_step.hpp:599-635): models of a grid are independent, so the host runs
// this policy once per active model with the (m, G) column-major arrays offset to that column.
// Different arithmetic from e_step: no fma in mu / the logit / d, half_var_tau instead of its
// square root, no skip branch.  EXACT = false (math_mode = fast): the sigmoid on v_exp_f32 / v_rcp_f32.
template <bool EXACT = true>
struct GridColumnModel {
    static constexpr bool kLaneParallel = false;
    struct In { float mm, beta, hvt, ulog, eta_old; };
    static __device__ __forceinline__ In load(const EStepArgs<float>& A, int64_t j, bool live) {
        In in;
        in.mm = live ? A.mu_mult[j] : 0.0f;
        in.beta = live ? A.std_beta[j] : 0.0f;
        in.hvt = live ? A.shvt[j] : 0.0f;
        in.ulog = live ? A.u_logs[j] : 0.0f;
        in.eta_old = live ? A.eta[j] : 0.0f;
        return in;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ void core(const In& in, float q, const ExpTab& tab, float& mu, float& gamma,
                                                float& d, int sel) {
        mu = in.mm * (in.beta - q);                                       // :613
        const float u = in.ulog + in.hvt * mu * mu;                       // :616
        gamma = EXACT ? sigmoid_exact<LOOKUP>(u, tab, sel) : sigmoid_fast(u);   // :617
        d = gamma * mu - in.eta_old;                                      // :620
    }
    static constexpr bool kHasSkip = false;
    template <int LOOKUP>
    static __device__ __forceinline__ float delta(const In& in, float q, const ExpTab& tab, int sel) {
        float mu, gamma, d;
        core<LOOKUP>(in, q, tab, mu, gamma, d, sel);
        return d;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ bool update(const In& in, float q, const ExpTab& tab, float& d, int sel) {
        d = delta<LOOKUP>(in, q, tab, sel);
        return true;
    }
    template <bool TEAM>
    static __device__ __forceinline__ float finish(const EStepArgs<float>& A, int64_t j, const In& in, float q,
                                                   const ExpTab& tab, bool live, bool writer, bool& skipped,
                                                   float* d_out = nullptr) {
        float mu, gamma, d;
        core<kLookupPerLane>(in, q, tab, mu, gamma, d, 0);
        if (d_out) *d_out = live ? d : 0.0f;
        if (live && writer) {
            A.var_mu[j] = mu;
            A.var_gamma[j] = gamma;
            A.eta_diff[j] = d;
            if (TEAM) stage_store(A.eta_out + j, in.eta_old + d); else A.eta[j] = in.eta_old + d;   // :633
        }
        skipped = false;
        return live ? A.dq * d : 0.0f;
    }
};

template <typename MODEL> struct IsGridColumn : std::false_type {};
template <bool EXACT> struct IsGridColumn<GridColumnModel<EXACT>> : std::true_type {};

// exp(x), x <= 0, of the softmax (e_step.hpp:231-240): glibc's expf bit for bit, or v_exp_f32 (math_mode = fast)
template <bool EXACT, int LOOKUP>
__device__ __forceinline__ float softmax_exp(float x, const ExpTab& tab, int sel = 0) {
    if constexpr (EXACT) return expf_glibc_nonpos<LOOKUP>(x, tab, sel);
    else return expf_fast_nonpos(x);
}
// e / ssum of the softmax (:239): the IEEE fp32 divide, or e * v_rcp_f32(ssum) (math_mode = fast; 1 ulp + 1 rounding)
template <bool EXACT>
__device__ __forceinline__ float softmax_div(float e, float ssum) {
    if constexpr (EXACT) return e / ssum;
    else return e * __builtin_amdgcn_rcpf(ssum);
}

// e_step_mixture (e_step.hpp:496-537) for K <= kPanelMaxK components ((m, K) arrays C-ordered).
template <bool EXACT = true>
struct MixtureModel {
    static constexpr bool kExact = EXACT;
    // the chain evaluates the K + 1 components of ONE SNP on K + 1 lanes (see the chain in panel_role)
    static constexpr bool kLaneParallel = true;
    struct In { float mm[kPanelMaxK], sv[kPanelMaxK], ulog[kPanelMaxK]; float lnp, beta, eta_old; int K; };
    static __device__ __forceinline__ In load(const EStepArgs<float>& A, int64_t j, bool live) {
        In in;
        in.K = A.width;
#pragma unroll
        for (int k = 0; k < kPanelMaxK; ++k) {
            const bool on = live && k < in.K;
            const int64_t idx = on ? j * in.K + k : 0;
            in.mm[k] = on ? A.mu_mult[idx] : 0.0f;
            in.sv[k] = on ? A.shvt[idx] : 0.0f;
            in.ulog[k] = on ? A.u_logs[idx] : 0.0f;
        }
        in.lnp = live ? A.log_null_pi[j] : 0.0f;
        in.beta = live ? A.std_beta[j] : 0.0f;
        in.eta_old = live ? A.eta[j] : 0.0f;
        return in;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ void core(const In& in, float q, const ExpTab& tab, float (&mu)[kPanelMaxK],
                                                float (&gam)[kPanelMaxK], float& d, int sel) {
        const float r = in.beta - q;                                      // :505
        float u[kPanelMaxK];
        float mx = in.lnp;                                                // max over u_0..u_K (c_max, :58-71)
#pragma unroll
        for (int k = 0; k < kPanelMaxK; ++k) {
            mu[k] = in.mm[k] * r;                                         // :509
            const float t = in.sv[k] * mu[k];
            u[k] = __builtin_fmaf(t, t, in.ulog[k]);                      // :511
            if (k < in.K) mx = fmaxf(mx, u[k]);
        }
        float ssum = 0.0f;                                                // softmax, :231-240: k = 0..K in order
#pragma unroll
        for (int k = 0; k < kPanelMaxK; ++k) {
            if (k < in.K) {
                u[k] = softmax_exp<EXACT, LOOKUP>(u[k] - mx, tab, sel);
                ssum += u[k];
            }
        }
        ssum += softmax_exp<EXACT, LOOKUP>(in.lnp - mx, tab, sel);
        d = -in.eta_old;                                                  // :519
#pragma unroll
        for (int k = 0; k < kPanelMaxK; ++k) {
            if (k < in.K) {
                gam[k] = softmax_div<EXACT>(u[k], ssum);                  // :239
                d = __builtin_fmaf(gam[k], mu[k], d);                     // :523
            }
        }
    }
    template <int LOOKUP>
    static __device__ __forceinline__ bool update(const In& in, float q, const ExpTab& tab, float& d, int sel) {
        float mu[kPanelMaxK], gam[kPanelMaxK];
        core<LOOKUP>(in, q, tab, mu, gam, d, sel);
        return true;
    }
    template <bool TEAM>
    static __device__ __forceinline__ float finish(const EStepArgs<float>& A, int64_t j, const In& in, float q,
                                                   const ExpTab& tab, bool live, bool writer, bool& skipped) {
        float mu[kPanelMaxK], gam[kPanelMaxK], d;
        core<kLookupPerLane>(in, q, tab, mu, gam, d, 0);
        if (live && writer) {
#pragma unroll
            for (int k = 0; k < kPanelMaxK; ++k) {
                if (k < in.K) {
                    A.var_mu[j * in.K + k] = mu[k];
                    A.var_gamma[j * in.K + k] = gam[k];
                }
            }
            A.eta_diff[j] = d;
            if (TEAM) stage_store(A.eta_out + j, in.eta_old + d); else A.eta[j] = in.eta_old + d;   // :536
        }
        skipped = false;
        return live ? A.dq * d : 0.0f;
    }
};

// e_step_mixture for kPanelMaxK < K <= kPanelWideMaxK components: the K + 1 components of one SNP on K + 1 lanes as
// in MixtureModel, but (i) the component inputs of the coming SNPs are prefetched from global memory into a ring of
// registers (the (m, K) arrays keep a SNP's K values contiguous: one 128-byte line per SNP and array) and the
// per-component outputs are stored straight from the chain -- no LDS staging that would grow with K; (ii) the
// reference's ordered sums (softmax denominator e_step.hpp:231-240, eta :519-523) run as scalar chains over
// v_readlane values: KMAX terms whatever K is -- the terms of lanes > K are exactly neutral (e = +0, gamma = 0).
template <int KMAX>
struct MixtureWideModel {
    static constexpr bool kLaneParallel = true;
    static constexpr bool kWide = true;
    static constexpr int kMax = KMAX;
    struct In { float lnp, beta, eta_old; int K; };
    static __device__ __forceinline__ In load(const EStepArgs<float>& A, int64_t j, bool live) {
        In in;
        in.K = A.width;
        in.lnp = live ? A.log_null_pi[j] : 0.0f;
        in.beta = live ? A.std_beta[j] : 0.0f;
        in.eta_old = live ? A.eta[j] : 0.0f;
        return in;
    }
};
template <typename M, typename = void> struct is_wide_mixture { static constexpr bool value = false; };
template <typename M> struct is_wide_mixture<M, std::enable_if_t<M::kWide>> { static constexpr bool value = true; };

}  // namespace viprs
