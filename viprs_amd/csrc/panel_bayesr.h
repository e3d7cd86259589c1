// Model policy of the SBayesR Gibbs sweep, viprs_state_bayesr_sweep (include/viprs_hip.h): the mixture E-step with a draw of
// the component and of the effect where the E-step stores an expectation.  A policy like those of panel_gibbs.h and
// panel_enet.h: the panel sweep (estep_panel.h) and the band kernel (estep_band.h) stream LD, hand panels between team members
// and run the upper form's second pass for it unchanged.
#pragma once
#include "panel_models.h"

namespace viprs {

constexpr int kBayesRMaxK = 4;      // non-null components one lane evaluates in registers

// One SNP j of a mixture state of K <= kBayesRMaxK components, lane-per-SNP: the lane evaluates all K components one after
// the other.  mu_k and gamma_k are MixtureModel<true>::core's term by term (e_step.hpp:496-537) -- every operation separately
// rounded in float32 (the translation units are built with -ffp-contract=off), fma only where written, glibc's expf, the
// IEEE divide:
//   r = beta - q
//   mu_k = mu_mult_k * r;  t_k = sqrt_half_var_tau_k * mu_k;  u_k = fma(t_k, t_k, u_logs_k)                       k = 1..K
//   mx = max(log_null_pi, u_1, .., u_K)        (fmaxf from log_null_pi, k ascending)
//   e_k = expf(u_k - mx);  ssum = ((0 + e_1) + .. + e_K) + expf(log_null_pi - mx)       (the null term LAST)
//   gamma_k = e_k / ssum
// THE DRAW, from the SNP's U, z of the state's draw buffers (abi_bayesr.hip):
//   c_1 = gamma_1;  c_k = c_{k-1} + gamma_k
//   k* = the smallest k in 1..K with U < c_k (strict), 0 if there is none
//   sd = 0x1.6a09e6p-1f / sqrt_half_var_tau_{k*}        (ONE IEEE divide, after the selection; the constant is
//   n  = z * sd                                           float32(1 / sqrt 2): sd^2 = 1 / (2 shvt^2), the conditional variance)
//   b = k* ? mu_{k*} + n : +0
//   d = b - eta_old
// (k* = 0: the divide runs on 1.0f and its result is not used.)
// Stores: var_mu[j, k] = mu_k, var_gamma[j, k] = gamma_k, eta_diff[j] = d, eta[j] = b (the draw itself, not eta_old + d)
// and kstar[j] = k*.
//
// WHERE THE DRAWS COME FROM.  A mixture state is swept with n_active == 0: select_model (kernels_common.h) then never reads
// `active`, nor does the panel sweep (its only other read is under IsGridColumn, estep_panel.h) or the band kernel, and the
// launchers pass it through untouched.  The slot carries the state's draw allocation: 3 m four-byte words, U | z | k*.
// select_model moves nothing for n_active == 0, so -- unlike the (m, G) columns of GibbsModel -- a plain pointer does.
struct BayesRModel {
    static constexpr bool kLaneParallel = false;
    static constexpr bool kHasSkip = false;
    struct In { float mm[kBayesRMaxK], sv[kBayesRMaxK], ulog[kBayesRMaxK]; float lnp, beta, eta_old, unif, z; int K; };
    // (a lane past the end of its block carries zeros and U = 1: mu_k = 0 (0 - q) = +-0, t_k = +-0, u_k = +0, mx = 0, e_k = 1,
    //  ssum = K + 1, c_K = K / (K + 1) up to rounding < 1 = U, so k* = 0, b = +0 and d = +0 - 0 = +0 whatever finite q it
    //  meets -- what the chain of estep_panel.h relies on.  With U = 0 it would pick k* = 1 and divide by shvt = 0.)
    static __device__ __forceinline__ In load(const EStepArgs<float>& A, int64_t j, bool live) {
        In in;
        in.K = A.width;
        const float* draws = reinterpret_cast<const float*>(A.active);
        in.z = live ? draws[A.m + j] : 0.0f;
#pragma unroll
        for (int k = 0; k < kBayesRMaxK; ++k) {
            const bool on = live && k < in.K;
            const int64_t idx = on ? j * in.K + k : 0;
            in.mm[k] = on ? A.mu_mult[idx] : 0.0f;
            in.sv[k] = on ? A.shvt[idx] : 0.0f;
            in.ulog[k] = on ? A.u_logs[idx] : 0.0f;
        }
        in.lnp = live ? A.log_null_pi[j] : 0.0f;
        in.beta = live ? A.std_beta[j] : 0.0f;
        in.eta_old = live ? A.eta[j] : 0.0f;
        in.unif = live ? draws[j] : 1.0f;
        return in;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ void core(const In& in, float q, const ExpTab& tab, float (&mu)[kBayesRMaxK],
                                                float (&gam)[kBayesRMaxK], int& kstar, float& b, float& d, int sel) {
        const float r = in.beta - q;
        float u[kBayesRMaxK];
        float mx = in.lnp;
#pragma unroll
        for (int k = 0; k < kBayesRMaxK; ++k) {
            mu[k] = in.mm[k] * r;
            const float t = in.sv[k] * mu[k];
            u[k] = __builtin_fmaf(t, t, in.ulog[k]);
            if (k < in.K) mx = fmaxf(mx, u[k]);
        }
        float ssum = 0.0f;
#pragma unroll
        for (int k = 0; k < kBayesRMaxK; ++k) {
            if (k < in.K) {
                u[k] = softmax_exp<true, LOOKUP>(u[k] - mx, tab, sel);
                ssum += u[k];
            }
        }
        ssum += softmax_exp<true, LOOKUP>(in.lnp - mx, tab, sel);
        float c = 0.0f, mu_s = 0.0f, sv_s = 1.0f;
        kstar = 0;
#pragma unroll
        for (int k = 0; k < kBayesRMaxK; ++k) {
            gam[k] = 0.0f;
            if (k < in.K) {
                gam[k] = softmax_div<true>(u[k], ssum);
                c = k == 0 ? gam[k] : c + gam[k];
                const bool hit = kstar == 0 && in.unif < c;
                mu_s = hit ? mu[k] : mu_s;
                sv_s = hit ? in.sv[k] : sv_s;
                kstar = hit ? k + 1 : kstar;
            }
        }
        const float sd = 0x1.6a09e6p-1f / sv_s;
        const float nz = in.z * sd;
        b = kstar != 0 ? mu_s + nz : 0.0f;
        d = b - in.eta_old;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ float delta(const In& in, float q, const ExpTab& tab, int sel) {
        float mu[kBayesRMaxK], gam[kBayesRMaxK], b, d;
        int kstar;
        core<LOOKUP>(in, q, tab, mu, gam, kstar, b, d, sel);
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
        float mu[kBayesRMaxK], gam[kBayesRMaxK], b, d;
        int kstar;
        core<kLookupPerLane>(in, q, tab, mu, gam, kstar, b, d, 0);
        if (d_out) *d_out = live ? d : 0.0f;
        if (live && writer) {
#pragma unroll
            for (int k = 0; k < kBayesRMaxK; ++k) {
                if (k < in.K) {
                    A.var_mu[j * in.K + k] = mu[k];
                    A.var_gamma[j * in.K + k] = gam[k];
                }
            }
            A.eta_diff[j] = d;
            if (TEAM) stage_store(A.eta_out + j, b); else A.eta[j] = b;      // (the draw itself, not eta_old + d)
            const_cast<int32_t*>(A.active)[2 * A.m + j] = kstar;
        }
        skipped = false;
        return live ? A.dq * d : 0.0f;
    }
};

}  // namespace viprs
