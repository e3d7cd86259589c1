// Host-side launcher of the LD-score kernels (ld_score.h) for one LD element type: #define SCORE_U, then include.
// SCORE_DENSE (0 / 1): the element type has repacked dense blocks (the types the panel schedule accepts).
#include "internal.h"
#include "ld_score.h"

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

template <typename T, typename U, int NC, int MODE, bool UNIT>
int launch_kernel(viprs_plan* P, ScoreArgs<T> A) {
    constexpr int R = MODE == kDotDense ? score_rows_per_wave<T, U, NC, UNIT>() : 1;
    if constexpr (MODE == kDotDense) {              // the product's work list of R rows per item
        const auto& rows = P->d_dot_rows_dense[R == 4 ? 2 : (R == 2 ? 1 : 0)];
        A.rows = rows.p;
        A.n_rows = (int64_t)rows.n;
    }
    if (A.n_rows == 0) return VIPRS_OK;
    const unsigned grid = (unsigned)((A.n_rows + kDotWaves - 1) / kDotWaves);
    ld_score_kernel<T, U, NC, MODE, R, UNIT><<<grid, dim3(64 * kDotWaves), 0, P->stream>>>(A);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

template <typename T, typename U, int MODE>
int launch_mode(viprs_plan* P, ScoreArgs<T> A) {
    if (!A.A) return launch_kernel<T, U, 1, MODE, true>(P, A);         // unit weights: their own instantiation
    // columns per pass: two accumulators per column and element of a 16-byte load
    constexpr bool kWide = sizeof(U) >= 2;
    if constexpr (kWide) {
        if (A.n_cols >= 4) return launch_kernel<T, U, 4, MODE, false>(P, A);
    }
    if (A.n_cols >= 2) return launch_kernel<T, U, 2, MODE, false>(P, A);
    return launch_kernel<T, U, 1, MODE, false>(P, A);
}

template <typename T, typename U>
int launch_typed(viprs_plan* P, int n_cols, const void* dA, const double* dCorr, void* dY, double dq_scale) {
    ScoreArgs<T> A;
    A.blocks = P->d_dot_blocks.p;
    A.ip = P->d_ip.p;
    A.lb = P->d_lb.p;
    A.first = P->d_dot_first.p;
    A.m = P->m;
    A.A = static_cast<const T*>(dA);
    A.corr = dCorr;
    A.Y = static_cast<T*>(dY);
    A.n_cols = n_cols;
    A.scale = (T)dq_scale;
    int rc = VIPRS_OK;
#if SCORE_DENSE
    A.rows = P->d_dot_rows_dense[0].p;
    A.n_rows = (int64_t)P->d_dot_rows_dense[0].n;
    A.ld = P->d_ld_dense.p;
    // upper form: the mirrored squares hold whole rows; the zero-lower-triangle storage is read in place, as the product does
    if (!P->low_memory || P->mirror) rc = launch_mode<T, U, kDotDense>(P, A);
    else rc = launch_mode<T, U, kDotDenseGather>(P, A);
    if (rc != VIPRS_OK) return rc;
#endif
    A.rows = P->d_dot_rows_ragged.p;
    A.n_rows = (int64_t)P->d_dot_rows_ragged.n;
    A.ld = P->d_ld_raw.p;
    if (P->low_memory) rc = launch_mode<T, U, kDotWindowUpper>(P, A);
    else rc = launch_mode<T, U, kDotWindowSym>(P, A);
    return rc;
}
}  // namespace

template <>
int launch_ld_score<SCORE_U>(viprs_plan* P, int float_dtype, int n_cols, const void* dA, const double* dCorr, void* dY,
                             double dq_scale) {
    if (float_dtype == VIPRS_F32) return launch_typed<float, SCORE_U>(P, n_cols, dA, dCorr, dY, dq_scale);
    return launch_typed<double, SCORE_U>(P, n_cols, dA, dCorr, dY, dq_scale);
}

}  // namespace viprs
