// C ABI, LD scores (include/viprs_hip.h): l_j = sum_k a_k r_jk^2 over every block of a plan -- what the reference gets from
// magenpy's `compute_ld_scores` and feeds to `simple_ldsc`.  Kernels: ld_score.h on ld_rows.h; tables: those of the product (abi_dot.hip).
#include "internal.h"

using namespace viprs;

extern "C" {

int viprs_plan_ld_scores(viprs_plan* P, int float_dtype, int n_cols, const void* a_host, const double* corr_host,
                         void* scores_host, double dq_scale) {
    if (float_size(float_dtype) == 0) return fail(VIPRS_EINVAL, "bad float dtype code");
    if (n_cols < 1) return fail(VIPRS_EINVAL, "n_cols must be at least 1");
    if (!a_host && n_cols != 1) return fail(VIPRS_EINVAL, "unit weights (null a_host) are one column: n_cols must be 1");
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    if (!scores_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    const size_t m = (size_t)P->m;
    const size_t bytes = m * (size_t)n_cols * float_size(float_dtype);
    if (a_host && P->d_score_a.n < bytes) HIP_TRY(P->d_score_a.alloc(bytes));
    if (P->d_score_y.n < bytes) HIP_TRY(P->d_score_y.alloc(bytes));
    if (corr_host && P->d_score_corr.n < m) HIP_TRY(P->d_score_corr.alloc(m));
    int rc = prepare_ld_rows(P);
    if (rc != VIPRS_OK) return rc;
    if (a_host) HIP_TRY(hipMemcpyAsync(P->d_score_a.p, a_host, bytes, hipMemcpyHostToDevice, P->stream));
    if (corr_host) HIP_TRY(hipMemcpyAsync(P->d_score_corr.p, corr_host, m * sizeof(double), hipMemcpyHostToDevice, P->stream));
    const void* dA = a_host ? P->d_score_a.p : nullptr;
    const double* dC = corr_host ? P->d_score_corr.p : nullptr;
    rc = P->time_score.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    switch (P->ld_dtype) {
        case VIPRS_LD_I8: rc = launch_ld_score<int8_t>(P, float_dtype, n_cols, dA, dC, P->d_score_y.p, dq_scale); break;
        case VIPRS_LD_I16: rc = launch_ld_score<int16_t>(P, float_dtype, n_cols, dA, dC, P->d_score_y.p, dq_scale); break;
        case VIPRS_LD_I32: rc = launch_ld_score<int32_t>(P, float_dtype, n_cols, dA, dC, P->d_score_y.p, dq_scale); break;
        case VIPRS_LD_I64: rc = launch_ld_score<int64_t>(P, float_dtype, n_cols, dA, dC, P->d_score_y.p, dq_scale); break;
        case VIPRS_LD_F32: rc = launch_ld_score<float>(P, float_dtype, n_cols, dA, dC, P->d_score_y.p, dq_scale); break;
        case VIPRS_LD_F64: rc = launch_ld_score<double>(P, float_dtype, n_cols, dA, dC, P->d_score_y.p, dq_scale); break;
        default: return fail(VIPRS_EINVAL, "bad LD dtype code");
    }
    if (rc != VIPRS_OK) return rc;
    rc = P->time_score.stop(P->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(P->stream));
    rc = check_device_error(P);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpy(scores_host, P->d_score_y.p, bytes, hipMemcpyDeviceToHost));
    return VIPRS_OK;
}

int viprs_plan_last_ld_score_ms(viprs_plan* P, double* ms) {
    if (!P || !ms) return fail(VIPRS_EINVAL, "null argument");
    return P->time_score.elapsed(P->device, ms, "no timed LD-score call yet");
}

}  // extern "C"
