// C ABI, ridge solve (include/viprs_hip.h): (R + diag(shift)) x = b by one MINRES per LD block, all blocks in lock step --
// what the reference's LDPredInf.fit() asks of scipy's minres over the assembled block-diagonal matrix
// (viprs/model/LDPredInf.py:43-114).  Kernels: ridge.h; the product of every iteration: abi_dot.hip.
#include "internal.h"
#include "ridge.h"

using namespace viprs;

int viprs::ensure_solver_blocks(viprs_plan* P) {
    const size_t nb = P->blocks.size();
    if (P->d_solver_blocks.p || nb == 0) return VIPRS_OK;
    std::vector<RidgeBlock> blocks(nb);
    for (size_t k = 0; k < nb; ++k) {
        blocks[k].start = P->blocks[k].start;
        blocks[k].size = (int32_t)(P->blocks[k].end - P->blocks[k].start);
        blocks[k].pad_ = 0;
    }
    HIP_TRY(P->d_solver_blocks.alloc(nb));
    HIP_TRY(hipMemcpy(P->d_solver_blocks.p, blocks.data(), nb * sizeof(RidgeBlock), hipMemcpyHostToDevice));
    return VIPRS_OK;
}

namespace {

int build_ridge_workspace(viprs_plan* P, size_t elem) {
    RidgeWork& W = P->ridge;
    const size_t nb = P->blocks.size();
    int rc = ensure_solver_blocks(P);
    if (rc != VIPRS_OK) return rc;
    if (!W.built) {
        HIP_TRY(W.d_rec.alloc(nb * sizeof(RidgeRec)));
        HIP_TRY(W.d_live.alloc(1));
        W.built = true;
    }
    const size_t bytes = (size_t)P->m * elem;
    if (W.vec_bytes < bytes) {
        W.vec_bytes = 0;
        for (auto& v : W.d_vec) HIP_TRY(v.alloc(bytes));
        HIP_TRY(W.d_shift.alloc(bytes));
        W.vec_bytes = bytes;
    }
    return VIPRS_OK;
}

template <typename T>
int solve_typed(viprs_plan* P, int float_dtype, const void* b_host, const double* shift_host, const void* x0_host,
                double dq_scale, double rtol, int max_iter, int check_every) {
    RidgeWork& W = P->ridge;
    const size_t m = (size_t)P->m, bytes = m * sizeof(T);
    const unsigned nb = (unsigned)P->blocks.size();
    T* vec[9];
    for (int i = 0; i < 9; ++i) vec[i] = reinterpret_cast<T*>(W.d_vec[i].p);
    T *v = vec[0], *Y = vec[1], *x = vec[8];
    T* r[3] = {vec[2], vec[3], vec[4]};             // r1, r2, the new r2
    T* w[3] = {vec[5], vec[6], vec[7]};             // w1, w2, the new w

    std::vector<T> shift(m);
    for (size_t j = 0; j < m; ++j) shift[j] = (T)shift_host[j];
    HIP_TRY(hipMemcpyAsync(W.d_shift.p, shift.data(), bytes, hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipMemcpyAsync(r[1], b_host, bytes, hipMemcpyHostToDevice, P->stream));
    if (x0_host) HIP_TRY(hipMemcpyAsync(x, x0_host, bytes, hipMemcpyHostToDevice, P->stream));
    else HIP_TRY(hipMemsetAsync(x, 0, bytes, P->stream));
    HIP_TRY(hipMemsetAsync(w[0], 0, bytes, P->stream));
    HIP_TRY(hipMemsetAsync(w[1], 0, bytes, P->stream));
    HIP_TRY(hipMemsetAsync(W.d_live.p, 0, sizeof(int32_t), P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));       // (the staging vector above goes out of use here)

    RidgeArgs<T> A;
    A.blocks = P->d_solver_blocks.p;
    A.rec = reinterpret_cast<RidgeRec*>(W.d_rec.p);
    A.live = W.d_live.p;
    A.Y = Y;
    A.shift = reinterpret_cast<const T*>(W.d_shift.p);
    A.v = v;
    A.x = x;
    A.rtol = rtol;
    A.max_iter = max_iter;
    A.has_x0 = x0_host ? 1 : 0;
    A.itn = 0;

    int rc = W.time.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    if (x0_host) {
        rc = enqueue_dot(P, float_dtype, 1, x, Y, dq_scale, 1);
        if (rc != VIPRS_OK) return rc;
    }
    A.r1 = r[0]; A.r2 = r[1]; A.y = r[1];
    A.w1 = w[0]; A.w2 = w[1]; A.w = w[2];
    ridge_init_kernel<T><<<nb, kRidgeThreads, 0, P->stream>>>(A, r[0]);
    HIP_TRY(hipGetLastError());

    W.iterations = 0;
    for (int itn = 1; itn <= max_iter; ++itn) {
        rc = enqueue_dot(P, float_dtype, 1, v, Y, dq_scale, 1);
        if (rc != VIPRS_OK) return rc;
        A.itn = itn;
        A.r1 = r[0]; A.r2 = r[1]; A.y = r[2];
        A.w1 = w[0]; A.w2 = w[1]; A.w = w[2];
        ridge_step_kernel<T><<<nb, kRidgeThreads, 0, P->stream>>>(A);
        HIP_TRY(hipGetLastError());
        W.iterations = itn;
        std::swap(r[0], r[1]); std::swap(r[1], r[2]);        // r1 <- r2 <- y
        std::swap(w[0], w[1]); std::swap(w[1], w[2]);        // w1 <- w2 <- w
        if (itn % check_every == 0 && itn < max_iter) {
            int32_t live = 0;
            HIP_TRY(hipMemcpyAsync(&live, W.d_live.p, sizeof(live), hipMemcpyDeviceToHost, P->stream));
            HIP_TRY(hipStreamSynchronize(P->stream));
            if (live == 0) break;
        }
    }
    rc = W.time.stop(P->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(P->stream));
    return check_device_error(P);
}

}  // namespace

extern "C" {

int viprs_plan_solve_ridge(viprs_plan* P, int float_dtype, const void* b_host, const double* shift_host, const void* x0_host,
                           void* x_host, double dq_scale, double rtol, int max_iter, int check_every, int32_t* block_iters,
                           double* block_relres, int32_t* block_status) {
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    const size_t elem = float_size(float_dtype);
    if (elem == 0) return fail(VIPRS_EINVAL, "bad float dtype code");
    if (!(rtol > 0.0)) return fail(VIPRS_EINVAL, "rtol must be positive");
    if (max_iter < 1) return fail(VIPRS_EINVAL, "max_iter must be at least 1");
    if (check_every < 1) return fail(VIPRS_EINVAL, "check_every must be at least 1");
    if (!b_host || !shift_host || !x_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    int rc = build_ridge_workspace(P, elem);
    if (rc != VIPRS_OK) return rc;
    if (float_dtype == VIPRS_F32)
        rc = solve_typed<float>(P, float_dtype, b_host, shift_host, x0_host, dq_scale, rtol, max_iter, check_every);
    else
        rc = solve_typed<double>(P, float_dtype, b_host, shift_host, x0_host, dq_scale, rtol, max_iter, check_every);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpy(x_host, P->ridge.d_vec[8].p, (size_t)P->m * elem, hipMemcpyDeviceToHost));
    const size_t nb = P->blocks.size();
    std::vector<RidgeRec> rec(nb);
    HIP_TRY(hipMemcpy(rec.data(), P->ridge.d_rec.p, nb * sizeof(RidgeRec), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nb; ++k) {
        if (block_iters) block_iters[k] = rec[k].iters;
        if (block_relres) block_relres[k] = rec[k].bnorm > 0.0 ? rec[k].phibar / rec[k].bnorm : 0.0;
        if (block_status) block_status[k] = rec[k].status;
    }
    return VIPRS_OK;
}

int viprs_plan_last_solve_ms(viprs_plan* P, double* total_ms, int* iterations) {
    if (!P || !total_ms) return fail(VIPRS_EINVAL, "null argument");
    const int rc = P->ridge.time.elapsed(P->device, total_ms, "no timed solve yet");
    if (rc == VIPRS_OK && iterations) *iterations = P->ridge.iterations;
    return rc;
}

}  // extern "C"
