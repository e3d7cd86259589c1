// C ABI, greedy LD clumping (include/viprs_hip.h): index_of[k, g] = the index SNP that claimed k under the threshold of
// column g -- the primitive of clumping + thresholding and, with the natural order, of LD pruning.  Kernel: ld_clump.h;
// tables: those of the product (abi_dot.hip).
#include <cmath>

#include "internal.h"

using namespace viprs;

// the block of d_dot_blocks (the dense blocks as the schedule sorted them, then the windowed ones) of every SNP
static void build_block_of(viprs_plan* P) {
    if (P->clump_block_of.size() == (size_t)P->m) return;
    P->clump_block_of.assign((size_t)P->m, -1);
    int32_t k = 0;
    for (const auto* list : {&P->dense_all_h, &P->ragged_all_h})
        for (const BlockDesc& bd : *list) {
            std::fill_n(P->clump_block_of.begin() + bd.start, bd.size, k);
            ++k;
        }
}

extern "C" {

int viprs_plan_clump(viprs_plan* P, int64_t n_order, const int32_t* order_host, const uint8_t* member_host, int n_cols,
                     const double* r2_host, double dq_scale, int32_t* index_of_host) {
    if (n_cols < 1 || n_cols > 32) return fail(VIPRS_EINVAL, "n_cols must be in 1..32");
    if (!r2_host) return fail(VIPRS_EINVAL, "null r2");
    for (int g = 0; g < n_cols; ++g)
        if (!std::isfinite(r2_host[g]) || r2_host[g] < 0.0) return fail(VIPRS_EINVAL, "r2 thresholds must be finite and >= 0");
    if (!std::isfinite(dq_scale) || !(dq_scale > 0.0)) return fail(VIPRS_EINVAL, "dq_scale must be finite and > 0");
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    if (!index_of_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (n_order < 0 || (n_order > 0 && !order_host)) return fail(VIPRS_EINVAL, "null order");
    const size_t m = (size_t)P->m;
    std::vector<uint32_t> mask(m);
    const uint32_t beyond = n_cols == 32 ? 0u : ~0u << n_cols;          // the bits >= n_cols are never free
    for (size_t j = 0; j < m; ++j) mask[j] = (!member_host || member_host[j]) ? beyond : ~0u;
    {
        std::vector<uint8_t> seen(m, 0);
        for (int64_t t = 0; t < n_order; ++t) {
            const int64_t j = order_host[t];
            if (j < 0 || j >= (int64_t)m) return fail(VIPRS_EINVAL, "order entry out of range");
            if (seen[(size_t)j]) return fail(VIPRS_EINVAL, "order entry repeated");
            if (mask[(size_t)j] == ~0u) return fail(VIPRS_EINVAL, "order entry is not a member");
            seen[(size_t)j] = 1;
        }
    }
    if (m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    int rc = prepare_ld_rows(P);
    if (rc != VIPRS_OK) return rc;
    // the order, split stably by block (a counting sort over the blocks of d_dot_blocks)
    build_block_of(P);
    const size_t n_blocks = P->dense_all_h.size() + P->ragged_all_h.size();
    std::vector<int64_t> off(n_blocks + 1, 0);
    for (int64_t t = 0; t < n_order; ++t) {
        if (P->clump_block_of[(size_t)order_host[t]] < 0) return fail(VIPRS_EINVAL, "order entry outside every LD block");
        off[(size_t)P->clump_block_of[(size_t)order_host[t]] + 1]++;
    }
    for (size_t k = 0; k < n_blocks; ++k) off[k + 1] += off[k];
    std::vector<int32_t> pieces((size_t)n_order);
    {
        std::vector<int64_t> at(off.begin(), off.end() - 1);
        for (int64_t t = 0; t < n_order; ++t) pieces[(size_t)at[(size_t)P->clump_block_of[(size_t)order_host[t]]]++] = order_host[t];
    }
    // the pass test on the stored element: (double)x (double)x >= r2 / dq_scale^2
    double thr[32];
    const double s2 = dq_scale * dq_scale;
    for (int g = 0; g < 32; ++g) thr[g] = g < n_cols ? r2_host[g] / s2 : 0.0;
    const size_t n_out = m * (size_t)n_cols;
    HIP_TRY(P->d_clump_order.reserve(pieces.size()));
    HIP_TRY(P->d_clump_off.reserve(n_blocks + 1));
    HIP_TRY(P->d_clump_thr.reserve(32));
    HIP_TRY(P->d_clump_mask.reserve(m));
    HIP_TRY(P->d_clump_index.reserve(n_out));
    // uploads and kernels on the plan's stream
    auto enqueue = [&]() -> int {
        if (!pieces.empty())
            HIP_TRY(hipMemcpyAsync(P->d_clump_order.p, pieces.data(), sizeof(int32_t) * pieces.size(), hipMemcpyHostToDevice, P->stream));
        HIP_TRY(hipMemcpyAsync(P->d_clump_off.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, P->stream));
        HIP_TRY(hipMemcpyAsync(P->d_clump_thr.p, thr, sizeof(thr), hipMemcpyHostToDevice, P->stream));
        HIP_TRY(hipMemcpyAsync(P->d_clump_mask.p, mask.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, P->stream));
        HIP_TRY(hipMemsetAsync(P->d_clump_index.p, 0xff, sizeof(int32_t) * n_out, P->stream));           // -1 everywhere
        int rc = P->time_clump.start(P->stream);
        if (rc != VIPRS_OK) return rc;
        switch (P->ld_dtype) {
            case VIPRS_LD_I8: rc = launch_ld_clump<int8_t>(P, n_cols); break;
            case VIPRS_LD_I16: rc = launch_ld_clump<int16_t>(P, n_cols); break;
            case VIPRS_LD_I32: rc = launch_ld_clump<int32_t>(P, n_cols); break;
            case VIPRS_LD_I64: rc = launch_ld_clump<int64_t>(P, n_cols); break;
            case VIPRS_LD_F32: rc = launch_ld_clump<float>(P, n_cols); break;
            case VIPRS_LD_F64: rc = launch_ld_clump<double>(P, n_cols); break;
            default: rc = fail(VIPRS_EINVAL, "bad LD dtype code");
        }
        return rc == VIPRS_OK ? P->time_clump.stop(P->stream) : rc;
    };
    rc = enqueue();
    // (the uploads read this call's host vectors: they are not released before the stream has drained, whatever failed)
    const hipError_t drained = hipStreamSynchronize(P->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(drained);
    rc = check_device_error(P);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpy(index_of_host, P->d_clump_index.p, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost));
    return VIPRS_OK;
}

int viprs_plan_last_clump_ms(viprs_plan* P, double* ms) {
    if (!P || !ms) return fail(VIPRS_EINVAL, "null argument");
    return P->time_clump.elapsed(P->device, ms, "no timed clumping call yet");
}

}  // extern "C"
