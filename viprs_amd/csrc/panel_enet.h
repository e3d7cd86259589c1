// Model policy of the elastic-net (lassosum) sweep, viprs_state_enet_sweep (include/viprs_hip.h): cyclic coordinate
// descent over each LD block with the running q = (R - I) beta -- the serial chain of the E-step with a soft threshold
// where the E-step has a sigmoid.  A policy like those of panel_models.h: the panel sweep (estep_panel.h) and the band
// kernel (estep_band.h) stream LD, hand panels between team members and run the upper form's second pass for it unchanged.
#pragma once
#include "panel_models.h"

namespace viprs {

// One SNP, every operation separately rounded in float32 (the translation units are built with -ffp-contract=off):
//   t = c q;  u = beta - t;  a = |u| - pen;  b = a > 0 ? copysign(a, u) : +0;  d = b - eta_old
// c = mu_mult (lassosum's 1 - s), pen = the field of sqrt_half_var_tau (lambda times a per-SNP factor, >= 0); u_logs is
// not read.  No skip branch: a zero d is added like any other.  No transcendental function: ExpTab is not used.
struct ElasticNetModel {
    static constexpr bool kLaneParallel = false;
    static constexpr bool kHasSkip = false;
    struct In { float c, beta, pen, eta_old; };
    // (a lane past the end of its block carries zeros: u = a = b = d = 0 whatever finite q it meets)
    static __device__ __forceinline__ In load(const EStepArgs<float>& A, int64_t j, bool live) {
        In in;
        in.c = live ? A.mu_mult[j] : 0.0f;
        in.beta = live ? A.std_beta[j] : 0.0f;
        in.pen = live ? A.shvt[j] : 0.0f;
        in.eta_old = live ? A.eta[j] : 0.0f;
        return in;
    }
    static __device__ __forceinline__ void core(const In& in, float q, float& u, float& b, float& d) {
        const float t = in.c * q;
        u = in.beta - t;
        const float a = fabsf(u) - in.pen;
        b = a > 0.0f ? copysignf(a, u) : 0.0f;
        d = b - in.eta_old;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ float delta(const In& in, float q, const ExpTab&, int) {
        float u, b, d;
        core(in, q, u, b, d);
        return d;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ bool update(const In& in, float q, const ExpTab& tab, float& d, int sel) {
        d = delta<LOOKUP>(in, q, tab, sel);
        return true;
    }
    template <bool TEAM>
    static __device__ __forceinline__ float finish(const EStepArgs<float>& A, int64_t j, const In& in, float q,
                                                   const ExpTab&, bool live, bool writer, bool& skipped,
                                                   float* d_out = nullptr) {
        float u, b, d;
        core(in, q, u, b, d);
        if (d_out) *d_out = live ? d : 0.0f;
        if (live && writer) {
            A.var_mu[j] = u;
            A.var_gamma[j] = b != 0.0f ? 1.0f : 0.0f;
            A.eta_diff[j] = d;
            if (TEAM) stage_store(A.eta_out + j, in.eta_old + d); else A.eta[j] = in.eta_old + d;
        }
        skipped = false;
        return live ? A.dq * d : 0.0f;
    }
};

}  // namespace viprs
