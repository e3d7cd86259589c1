// C ABI, LD product (include/viprs_hip.h): Y = R B over every block of a plan -- what the reference computes with
// `ld.dot(B)` (viprs/eval/pseudo_metrics.py:122-127, BayesPRSModel.py:397-404).  Kernels: ld_dot.h.
#include "internal.h"

using namespace viprs;

// Tables of the product: every block of the plan (the active-block filter of the sweeps does not apply), one work item per
// row, in the order of the plan's full block lists (the dense blocks as the schedule sorted them, then the windowed ones).
static int build_dot_tables(viprs_plan* P) {
    if (P->dot_built) return VIPRS_OK;
    std::vector<BlockDesc> blocks(P->dense_all_h);
    blocks.insert(blocks.end(), P->ragged_all_h.begin(), P->ragged_all_h.end());
    std::vector<int64_t> rows_dense[3], rows_ragged;
    for (size_t k = 0; k < blocks.size(); ++k) {
        const bool dense = k < P->dense_all_h.size();
        for (int r = 0; r < blocks[k].size; ++r) {
            const int64_t item = (int64_t)k << 32 | (int64_t)r;
            if (!dense) { rows_ragged.push_back(item); continue; }
            for (int c = 0; c < 3; ++c)
                if (r % (1 << c) == 0) rows_dense[c].push_back(item);
        }
    }
    HIP_TRY(P->d_dot_blocks.alloc(blocks.size()));
    if (!blocks.empty())
        HIP_TRY(hipMemcpy(P->d_dot_blocks.p, blocks.data(), sizeof(BlockDesc) * blocks.size(), hipMemcpyHostToDevice));
    for (int c = 0; c < 3; ++c) {
        HIP_TRY(P->d_dot_rows_dense[c].alloc(rows_dense[c].size()));
        if (!rows_dense[c].empty())
            HIP_TRY(hipMemcpy(P->d_dot_rows_dense[c].p, rows_dense[c].data(), sizeof(int64_t) * rows_dense[c].size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(P->d_dot_rows_ragged.alloc(rows_ragged.size()));
    if (!rows_ragged.empty())
        HIP_TRY(hipMemcpy(P->d_dot_rows_ragged.p, rows_ragged.data(), sizeof(int64_t) * rows_ragged.size(), hipMemcpyHostToDevice));
    if (P->low_memory && !rows_ragged.empty()) {
        // upper form, windowed rows: row j also holds the entries (i, j) of the rows i < j that reach it; first[j] = the
        // lowest such row (j itself if there is none).  Rows in ascending order: the first row to cover j is the lowest.
        const size_t m = (size_t)P->m;
        std::vector<int64_t> ip(m + 1);
        HIP_TRY(hipMemcpy(ip.data(), P->d_ip.p, sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost));
        std::vector<int32_t> first(m);
        for (size_t j = 0; j < m; ++j) first[j] = (int32_t)j;
        int64_t covered = -1;
        for (int64_t i = 0; i < (int64_t)m; ++i) {
            const int64_t hi = std::min<int64_t>(i + (ip[(size_t)i + 1] - ip[(size_t)i]), (int64_t)m - 1);
            for (int64_t j = std::max(i + 1, covered + 1); j <= hi; ++j) first[(size_t)j] = (int32_t)i;
            covered = std::max(covered, hi);
        }
        HIP_TRY(P->d_dot_first.alloc(m));
        HIP_TRY(hipMemcpy(P->d_dot_first.p, first.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
    }
    P->dot_built = true;
    return VIPRS_OK;
}

int viprs::prepare_ld_rows(viprs_plan* P) {
    int rc = build_dot_tables(P);
    if (rc != VIPRS_OK) return rc;
    // Upper form: a plan nobody has swept yet holds the zero lower triangle only because the repack left it so -- mirror it
    // once, as the first fp32 sweep would.  A plan whose last sweep asked for the zero lower triangle (float64 state) keeps
    // it: the product reads that storage in place instead of converting the whole LD back and forth between EM rounds.
    if (P->low_memory && !P->mirror && !P->unmirrored_wanted) return ensure_upper_storage(P, true);
    return VIPRS_OK;
}

// the kernels of one product on the plan's stream, between the product's own two events (internal.h: the solvers call it too)
int viprs::enqueue_dot(viprs_plan* P, int float_dtype, int n_cols, const void* dB, void* dY, double dq_scale, int include_diagonal) {
    int rc = prepare_ld_rows(P);
    if (rc != VIPRS_OK) return rc;
    rc = P->time_dot.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    switch (P->ld_dtype) {
        case VIPRS_LD_I8: rc = launch_ld_dot<int8_t>(P, float_dtype, n_cols, dB, dY, dq_scale, include_diagonal); break;
        case VIPRS_LD_I16: rc = launch_ld_dot<int16_t>(P, float_dtype, n_cols, dB, dY, dq_scale, include_diagonal); break;
        case VIPRS_LD_I32: rc = launch_ld_dot<int32_t>(P, float_dtype, n_cols, dB, dY, dq_scale, include_diagonal); break;
        case VIPRS_LD_I64: rc = launch_ld_dot<int64_t>(P, float_dtype, n_cols, dB, dY, dq_scale, include_diagonal); break;
        case VIPRS_LD_F32: rc = launch_ld_dot<float>(P, float_dtype, n_cols, dB, dY, dq_scale, include_diagonal); break;
        case VIPRS_LD_F64: rc = launch_ld_dot<double>(P, float_dtype, n_cols, dB, dY, dq_scale, include_diagonal); break;
        default: return fail(VIPRS_EINVAL, "bad LD dtype code");
    }
    if (rc != VIPRS_OK) return rc;
    return P->time_dot.stop(P->stream);
}

extern "C" {

int viprs_plan_dot(viprs_plan* P, int float_dtype, int n_cols, const void* b_host, void* y_host, double dq_scale,
                   int include_diagonal) {
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    if (float_size(float_dtype) == 0) return fail(VIPRS_EINVAL, "bad float dtype code");
    if (n_cols < 1) return fail(VIPRS_EINVAL, "n_cols must be at least 1");
    if (!b_host || !y_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    const size_t bytes = (size_t)P->m * (size_t)n_cols * float_size(float_dtype);
    if (P->d_dot_b.n < bytes) HIP_TRY(P->d_dot_b.alloc(bytes));
    if (P->d_dot_y.n < bytes) HIP_TRY(P->d_dot_y.alloc(bytes));
    HIP_TRY(hipMemcpyAsync(P->d_dot_b.p, b_host, bytes, hipMemcpyHostToDevice, P->stream));
    int rc = enqueue_dot(P, float_dtype, n_cols, P->d_dot_b.p, P->d_dot_y.p, dq_scale, include_diagonal);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(P->stream));
    rc = check_device_error(P);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpy(y_host, P->d_dot_y.p, bytes, hipMemcpyDeviceToHost));
    return VIPRS_OK;
}

int viprs_state_dot(viprs_state* S, int field, double dq_scale, int include_diagonal, void* y_host) {
    if (!S || !S->plan) return fail(VIPRS_EINVAL, "null state");
    if (field != VIPRS_FIELD_ETA) return fail(VIPRS_EINVAL, "the LD product takes the posterior mean (VIPRS_FIELD_ETA) only");
    if (!y_host) return fail(VIPRS_EINVAL, "null host buffer");
    viprs_plan* P = S->plan;
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    const int n_cols = S->model_kind == VIPRS_MODEL_GRID ? S->width : 1;
    const size_t bytes = (size_t)P->m * (size_t)n_cols * float_size(S->float_dtype);
    if (P->d_dot_y.n < bytes) HIP_TRY(P->d_dot_y.alloc(bytes));
    int rc = enqueue_dot(P, S->float_dtype, n_cols, S->f[VIPRS_FIELD_ETA].p, P->d_dot_y.p, dq_scale, include_diagonal);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(P->stream));
    rc = check_device_error(P);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpy(y_host, P->d_dot_y.p, bytes, hipMemcpyDeviceToHost));
    return VIPRS_OK;
}

int viprs_plan_last_dot_ms(viprs_plan* P, double* ms) {
    if (!P || !ms) return fail(VIPRS_EINVAL, "null argument");
    return P->time_dot.elapsed(P->device, ms, "no timed product yet");
}

}  // extern "C"
