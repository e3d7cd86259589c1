// Host-side launcher of the row-stream kernels (ld_rows.h) for one operation and one LD element type:
//     #define ROWS_U      the LD element type
//     #define ROWS_DENSE  0 / 1: the element type has repacked dense blocks (the types the panel schedule accepts)
//     #define ROWS_SCORE  0: the product (ld_dot.h), 1: the LD scores (ld_score.h)
// then include.
#include "internal.h"
#if ROWS_SCORE
#include "ld_score.h"
#else
#include "ld_dot.h"
#endif

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

template <typename Op, typename U, int NC, int MODE>
int launch_kernel(viprs_plan* P, typename Op::Args A) {
    constexpr int R = MODE == kDotDense ? rows_per_wave<typename Op::T, U>(Op::kSums * NC) : 1;
    if constexpr (MODE == kDotDense) {              // the work list of R rows per item
        const auto& rows = P->d_dot_rows_dense[R == 4 ? 2 : (R == 2 ? 1 : 0)];
        A.rows = rows.p;
        A.n_rows = (int64_t)rows.n;
    }
    if (A.n_rows == 0) return VIPRS_OK;
    const unsigned grid = (unsigned)((A.n_rows + kDotWaves - 1) / kDotWaves);
    ld_rows_kernel<Op, U, NC, MODE, R><<<grid, dim3(64 * kDotWaves), 0, P->stream>>>(A);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

// columns per pass: as many as leave room for the accumulators (columns x the operation's sums x elements of a 16-byte load)
template <typename Op, typename U, int MODE> constexpr int max_cols() {
    if (!Op::kOperand) return 1;
    if (Op::kSums == 1) return MODE == kDotDense && sizeof(U) >= 2 ? 8 : 4;
    return sizeof(U) >= 2 ? 4 : 2;
}

template <typename Op, typename U, int MODE>
int launch_mode(viprs_plan* P, const typename Op::Args& A) {
    constexpr int kMax = max_cols<Op, U, MODE>();
    if constexpr (kMax >= 8) if (A.n_cols >= 8) return launch_kernel<Op, U, 8, MODE>(P, A);
    if constexpr (kMax >= 4) if (A.n_cols >= 4) return launch_kernel<Op, U, 4, MODE>(P, A);
    if constexpr (kMax >= 2) if (A.n_cols >= 2) return launch_kernel<Op, U, 2, MODE>(P, A);
    return launch_kernel<Op, U, 1, MODE>(P, A);
}

// every block of the plan: the dense ones, then the windowed ones; `A` comes with the operation's own fields set
template <typename Op, typename U>
int launch_rows(viprs_plan* P, typename Op::Args A) {
    A.blocks = P->d_dot_blocks.p;
    A.ip = P->d_ip.p;
    A.lb = P->d_lb.p;
    A.first = P->d_dot_first.p;
    A.m = P->m;
    int rc = VIPRS_OK;
#if ROWS_DENSE
    A.rows = P->d_dot_rows_dense[0].p;
    A.n_rows = (int64_t)P->d_dot_rows_dense[0].n;
    A.ld = P->d_ld_dense.p;
    // upper form: the mirrored squares hold whole rows; the float64 sweeps' zero-lower-triangle storage is read as it is
    // (entries left of the diagonal from the column above it), so that a call between sweeps converts nothing
    if (!P->low_memory || P->mirror) rc = launch_mode<Op, U, kDotDense>(P, A);
    else rc = launch_mode<Op, U, kDotDenseGather>(P, A);
    if (rc != VIPRS_OK) return rc;
#endif
    A.rows = P->d_dot_rows_ragged.p;
    A.n_rows = (int64_t)P->d_dot_rows_ragged.n;
    A.ld = P->d_ld_raw.p;
    if (P->low_memory) rc = launch_mode<Op, U, kDotWindowUpper>(P, A);
    else rc = launch_mode<Op, U, kDotWindowSym>(P, A);
    return rc;
}

#if ROWS_SCORE
template <typename T>
int launch_typed(viprs_plan* P, int n_cols, const void* dA, const double* dCorr, void* dY, double dq_scale) {
    ScoreArgs<T> A;
    A.A = static_cast<const T*>(dA);
    A.corr = dCorr;
    A.Y = static_cast<T*>(dY);
    A.n_cols = n_cols;
    A.scale = (T)dq_scale;
    if (!dA) return launch_rows<ScoreOp<T, true>, ROWS_U>(P, A);            // unit weights: their own instantiation
    return launch_rows<ScoreOp<T, false>, ROWS_U>(P, A);
}
#else
template <typename T>
int launch_typed(viprs_plan* P, int n_cols, const void* dB, void* dY, double dq_scale, int include_diagonal) {
    DotArgs<T> A;
    A.B = static_cast<const T*>(dB);
    A.Y = static_cast<T*>(dY);
    A.n_cols = n_cols;
    A.scale = (T)dq_scale;
    A.include_diagonal = include_diagonal;
    return launch_rows<DotOp<T>, ROWS_U>(P, A);
}
#endif
}  // namespace

#if ROWS_SCORE
template <>
int launch_ld_score<ROWS_U>(viprs_plan* P, int float_dtype, int n_cols, const void* dA, const double* dCorr, void* dY,
                            double dq_scale) {
    if (float_dtype == VIPRS_F32) return launch_typed<float>(P, n_cols, dA, dCorr, dY, dq_scale);
    return launch_typed<double>(P, n_cols, dA, dCorr, dY, dq_scale);
}
#else
template <>
int launch_ld_dot<ROWS_U>(viprs_plan* P, int float_dtype, int n_cols, const void* dB, void* dY, double dq_scale,
                          int include_diagonal) {
    if (float_dtype == VIPRS_F32) return launch_typed<float>(P, n_cols, dB, dY, dq_scale, include_diagonal);
    return launch_typed<double>(P, n_cols, dB, dY, dq_scale, include_diagonal);
}
#endif

}  // namespace viprs
