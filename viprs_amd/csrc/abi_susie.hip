// C ABI, SuSiE fine-mapping (include/viprs_hip.h): L single effects per LD block by iterative Bayesian stepwise selection on
// z-scores (susie_rss with the residual variance fixed at 1), all blocks in lock step.  Kernels: susie.h; the product of
// every step: abi_dot.hip.  The reference tree has no fine-mapping model: the header's definition is the contract.
#include <cmath>

#include "internal.h"
#include "susie.h"

using namespace viprs;

namespace {

int build_susie_workspace(viprs_plan* P, size_t elem, int L) {
    SusieWork& W = P->susie;
    const size_t nb = P->blocks.size(), m = (size_t)P->m;
    int rc = ensure_solver_blocks(P);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(W.d_rec.reserve(nb * sizeof(SusieRec)));
    HIP_TRY(W.d_live.reserve(1));
    for (DevBuf<char>* b : {&W.d_alpha, &W.d_mu, &W.d_rb}) HIP_TRY(b->reserve(m * (size_t)L * elem));
    for (DevBuf<char>* b : {&W.d_bbar, &W.d_y}) HIP_TRY(b->reserve(m * elem));
    for (DevBuf<double>* b : {&W.d_w, &W.d_z, &W.d_log_pi}) HIP_TRY(b->reserve(m));
    for (DevBuf<double>* b : {&W.d_v, &W.d_v0, &W.d_post_var}) HIP_TRY(b->reserve(nb * (size_t)L));
    return VIPRS_OK;
}

template <typename T>
int susie_typed(viprs_plan* P, int float_dtype, int L, const double* z, const double* log_pi, const double* v0,
                int estimate, double dq_scale, double tol, int max_iter, int check_every) {
    SusieWork& W = P->susie;
    const size_t m = (size_t)P->m;
    const unsigned nb = (unsigned)P->blocks.size();
    HIP_TRY(hipMemcpyAsync(W.d_z.p, z, m * sizeof(double), hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipMemcpyAsync(W.d_log_pi.p, log_pi, m * sizeof(double), hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipMemcpyAsync(W.d_v0.p, v0, (size_t)nb * (size_t)L * sizeof(double), hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipMemsetAsync(W.d_live.p, 0, sizeof(int32_t), P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));       // (the caller's staging vectors go out of use here)

    SusieArgs<T> A;
    A.blocks = P->d_solver_blocks.p;
    A.rec = reinterpret_cast<SusieRec*>(W.d_rec.p);
    A.live = W.d_live.p;
    A.Y = reinterpret_cast<const T*>(W.d_y.p);
    A.alpha = reinterpret_cast<T*>(W.d_alpha.p);
    A.mu = reinterpret_cast<T*>(W.d_mu.p);
    A.Rb = reinterpret_cast<T*>(W.d_rb.p);
    A.bbar = reinterpret_cast<T*>(W.d_bbar.p);
    A.w = W.d_w.p;
    A.z = W.d_z.p;
    A.log_pi = W.d_log_pi.p;
    A.V = W.d_v.p;
    A.post_var = W.d_post_var.p;
    A.V0 = W.d_v0.p;
    A.m = P->m;
    A.tol = tol;
    A.L = L;
    A.l = 0;
    A.it = 0;
    A.max_iter = max_iter;
    A.store_prev = 0;
    A.estimate = estimate;

    int rc = W.time.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    susie_init_kernel<T><<<nb, kRidgeThreads, 0, P->stream>>>(A);
    HIP_TRY(hipGetLastError());
    W.steps = 0;
    bool done = false;
    for (int it = 1; it <= max_iter && !done; ++it) {
        for (int l = 0; l < L; ++l) {
            A.it = it;
            A.l = l;
            A.store_prev = W.steps > 0;
            const bool timed = it == 1 && l == L - 1;
            if (timed) {
                rc = W.time_step.start(P->stream);
                if (rc != VIPRS_OK) return rc;
            }
            susie_step_kernel<T><<<nb, kRidgeThreads, 0, P->stream>>>(A);
            HIP_TRY(hipGetLastError());
            if (timed) {
                rc = W.time_step.stop(P->stream);
                if (rc != VIPRS_OK) return rc;
            }
            W.steps++;
            if (it == max_iter && l == L - 1) break;            // (nobody reads the product of the last step)
            rc = enqueue_dot(P, float_dtype, 1, A.bbar, W.d_y.p, dq_scale, 1);
            if (rc != VIPRS_OK) return rc;
        }
        if (it % check_every == 0 && it < max_iter) {
            int32_t live = 0;
            HIP_TRY(hipMemcpyAsync(&live, W.d_live.p, sizeof(live), hipMemcpyDeviceToHost, P->stream));
            HIP_TRY(hipStreamSynchronize(P->stream));
            done = live == 0;
        }
    }
    rc = W.time.stop(P->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(P->stream));
    return check_device_error(P);
}

}  // namespace

extern "C" {

int viprs_plan_susie(viprs_plan* P, int float_dtype, int L, const double* z_host, const double* log_prior_host,
                     const double* prior_variance_host, double prior_variance0, int estimate_prior_variance, double dq_scale,
                     double tol, int max_iter, int check_every, void* alpha_host, void* mu_host, double* prior_variance_out,
                     double* post_var_out, int32_t* block_iters, double* block_delta, int32_t* block_status) {
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    const size_t elem = float_size(float_dtype);
    if (elem == 0) return fail(VIPRS_EINVAL, "bad float dtype code");
    if (L < 1 || L > kSusieMaxL) return fail(VIPRS_EINVAL, "L must be in 1..32");
    if (!(tol > 0.0)) return fail(VIPRS_EINVAL, "tol must be positive");
    if (max_iter < 1) return fail(VIPRS_EINVAL, "max_iter must be at least 1");
    if (check_every < 1) return fail(VIPRS_EINVAL, "check_every must be at least 1");
    if (!std::isfinite(dq_scale) || !(dq_scale > 0.0)) return fail(VIPRS_EINVAL, "dq_scale must be finite and positive");
    if (!prior_variance_host && (!std::isfinite(prior_variance0) || prior_variance0 < 0.0))
        return fail(VIPRS_EINVAL, "prior variance must be finite and >= 0");
    if (!z_host || !alpha_host || !mu_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (P->m == 0) return VIPRS_OK;
    // the checks of the values, still on the host
    const size_t m = (size_t)P->m, nb = P->blocks.size();
    for (size_t j = 0; j < m; ++j)
        if (!std::isfinite(z_host[j])) return fail(VIPRS_EINVAL, "z must be finite");
    std::vector<double> log_pi(m);
    for (size_t k = 0; k < nb; ++k) {
        const size_t s = (size_t)P->blocks[k].start, e = (size_t)P->blocks[k].end;
        bool any = false;
        for (size_t j = s; j < e; ++j) {
            const double lp = log_prior_host ? log_prior_host[j] : -std::log((double)(e - s));
            if (std::isnan(lp) || lp == HUGE_VAL) return fail(VIPRS_EINVAL, "log_prior must be finite or -inf");
            any = any || std::isfinite(lp);
            log_pi[j] = lp;
        }
        if (!any) return fail(VIPRS_EINVAL, "log_prior is -inf for every SNP of an LD block");
    }
    std::vector<double> v0(nb * (size_t)L, prior_variance0);
    if (prior_variance_host)
        for (size_t i = 0; i < v0.size(); ++i) {
            v0[i] = prior_variance_host[i];
            if (!std::isfinite(v0[i]) || v0[i] < 0.0) return fail(VIPRS_EINVAL, "prior variance must be finite and >= 0");
        }
    HIP_TRY(hipSetDevice(P->device));
    int rc = build_susie_workspace(P, elem, L);
    if (rc != VIPRS_OK) return rc;
    if (float_dtype == VIPRS_F32)
        rc = susie_typed<float>(P, float_dtype, L, z_host, log_pi.data(), v0.data(), estimate_prior_variance != 0, dq_scale,
                                tol, max_iter, check_every);
    else
        rc = susie_typed<double>(P, float_dtype, L, z_host, log_pi.data(), v0.data(), estimate_prior_variance != 0, dq_scale,
                                 tol, max_iter, check_every);
    if (rc != VIPRS_OK) return rc;
    SusieWork& W = P->susie;
    HIP_TRY(hipMemcpy(alpha_host, W.d_alpha.p, m * (size_t)L * elem, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mu_host, W.d_mu.p, m * (size_t)L * elem, hipMemcpyDeviceToHost));
    if (prior_variance_out)
        HIP_TRY(hipMemcpy(prior_variance_out, W.d_v.p, nb * (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
    if (post_var_out)
        HIP_TRY(hipMemcpy(post_var_out, W.d_post_var.p, nb * (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<SusieRec> rec(nb);
    HIP_TRY(hipMemcpy(rec.data(), W.d_rec.p, nb * sizeof(SusieRec), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nb; ++k) {
        if (block_iters) block_iters[k] = rec[k].iters;
        if (block_delta) block_delta[k] = rec[k].delta;
        if (block_status) block_status[k] = rec[k].status;
    }
    return VIPRS_OK;
}

int viprs_plan_last_susie_ms(viprs_plan* P, double* total_ms, int* steps, double* step_kernel_ms) {
    if (!P || !total_ms) return fail(VIPRS_EINVAL, "null argument");
    int rc = P->susie.time.elapsed(P->device, total_ms, "no timed fine-mapping call yet");
    if (rc != VIPRS_OK) return rc;
    if (steps) *steps = P->susie.steps;
    if (step_kernel_ms) rc = P->susie.time_step.elapsed(P->device, step_kernel_ms, "no timed fine-mapping call yet");
    return rc;
}

}  // extern "C"
