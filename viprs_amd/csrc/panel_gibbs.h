// Model policy of the LDpred2 Gibbs sweep, viprs_state_gibbs_sweep (include/viprs_hip.h): the grid-column E-step with a draw
// where the E-step stores an expectation.  A policy like those of panel_models.h and panel_enet.h: the panel sweep
// (estep_panel.h) and the band kernel (estep_band.h) stream LD, hand panels between team members and run the upper form's
// second pass for it unchanged.
#pragma once
#include "panel_models.h"

namespace viprs {

// One SNP: mu and gamma are GridColumnModel<true>::core's (exact sigmoid, no fma; the translation units are built with
// -ffp-contract=off), then
//   b = gamma > U ? mu + noise : +0;  d = b - eta_old
// with U and noise the SNP's entries of the state's two (m, G) draw buffers (gibbs_draws.hip).  No skip branch.
//
// WHERE THE DRAWS COME FROM.  A grid state has no log_null_pi, and select_model (kernels_common.h) leaves that slot of
// EStepArgs alone, so the slot carries the draws without a new member (the E-step kernels' argument block, and with it their
// generated code, stays as it is).  It cannot carry a pointer to column 0 of U: the policy sees the arguments AFTER
// select_model has moved the (m, G) fields to the item's column, and does not know which column that is.  It carries the
// DISTANCE in bytes from the state's mu_mult buffer to its U buffer instead (gibbs_args, internal.h): the column's U entry of
// SNP j then lies that far behind the column's mu_mult entry, and its noise entry m * G floats further (the two buffers are
// the two halves of one allocation).
struct GibbsModel {
    using Core = GridColumnModel<true>;
    static constexpr bool kLaneParallel = false;
    static constexpr bool kHasSkip = false;
    struct In { Core::In c; float unif, noise; };
    // (a lane past the end of its block carries zeros: mu = 0 (q - 0) = +-0, gamma = sigmoid(0) = 0.5 > U = 0, b = mu + 0,
    //  d = +-0 whatever finite q it meets -- what the chain of estep_panel.h relies on)
    static __device__ __forceinline__ In load(const EStepArgs<float>& A, int64_t j, bool live) {
        In in;
        in.c = Core::load(A, j, live);
        const float* u = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(A.mu_mult + j) +
                                                        reinterpret_cast<uintptr_t>(A.log_null_pi));
        in.unif = live ? u[0] : 0.0f;
        in.noise = live ? u[A.m * (int64_t)A.width] : 0.0f;
        return in;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ void core(const In& in, float q, const ExpTab& tab, float& mu, float& gamma, float& b,
                                                float& d, int sel) {
        float d_mean;
        Core::core<LOOKUP>(in.c, q, tab, mu, gamma, d_mean, sel);
        b = gamma > in.unif ? mu + in.noise : 0.0f;
        d = b - in.c.eta_old;
    }
    template <int LOOKUP>
    static __device__ __forceinline__ float delta(const In& in, float q, const ExpTab& tab, int sel) {
        float mu, gamma, b, d;
        core<LOOKUP>(in, q, tab, mu, gamma, b, d, sel);
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
        float mu, gamma, b, d;
        core<kLookupPerLane>(in, q, tab, mu, gamma, b, d, 0);
        if (d_out) *d_out = live ? d : 0.0f;
        if (live && writer) {
            A.var_mu[j] = mu;
            A.var_gamma[j] = gamma;
            A.eta_diff[j] = d;
            if (TEAM) stage_store(A.eta_out + j, b); else A.eta[j] = b;      // (the draw itself, not eta_old + d)
        }
        skipped = false;
        return live ? A.dq * d : 0.0f;
    }
};

}  // namespace viprs
