// Host-side launcher of the LD product kernels (ld_dot.h) for one LD element type: #define DOT_U, then include.
// DOT_DENSE (0 / 1): the element type has repacked dense blocks (the types the panel schedule accepts).
#include "internal.h"
#include "ld_dot.h"

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

template <typename T, typename U, int NC, int MODE>
int launch_kernel(viprs_plan* P, DotArgs<T> A) {
    constexpr int R = MODE == kDotDense ? dot_rows_per_wave<T, U, NC>() : 1;
    if constexpr (MODE == kDotDense) {              // the work list of R rows per item
        const auto& rows = P->d_dot_rows_dense[R == 4 ? 2 : (R == 2 ? 1 : 0)];
        A.rows = rows.p;
        A.n_rows = (int64_t)rows.n;
    }
    if (A.n_rows == 0) return VIPRS_OK;
    const unsigned grid = (unsigned)((A.n_rows + kDotWaves - 1) / kDotWaves);
    ld_dot_kernel<T, U, NC, MODE, R><<<grid, dim3(64 * kDotWaves), 0, P->stream>>>(A);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

template <typename T, typename U, int MODE>
int launch_mode(viprs_plan* P, DotArgs<T> A) {
    // columns per pass: 8 where the element type leaves room for the accumulators (columns x elements of a 16-byte load)
    constexpr bool kWide = MODE == kDotDense && sizeof(U) >= 2;
    if constexpr (kWide) {
        if (A.n_cols >= 8) return launch_kernel<T, U, 8, MODE>(P, A);
    }
    if (A.n_cols >= 4) return launch_kernel<T, U, 4, MODE>(P, A);
    if (A.n_cols >= 2) return launch_kernel<T, U, 2, MODE>(P, A);
    return launch_kernel<T, U, 1, MODE>(P, A);
}

template <typename T, typename U>
int launch_typed(viprs_plan* P, int n_cols, const void* dB, void* dY, double dq_scale, int include_diagonal) {
    DotArgs<T> A;
    A.blocks = P->d_dot_blocks.p;
    A.ip = P->d_ip.p;
    A.lb = P->d_lb.p;
    A.first = P->d_dot_first.p;
    A.m = P->m;
    A.B = static_cast<const T*>(dB);
    A.Y = static_cast<T*>(dY);
    A.n_cols = n_cols;
    A.scale = (T)dq_scale;
    A.include_diagonal = include_diagonal;
    int rc = VIPRS_OK;
#if DOT_DENSE
    A.rows = P->d_dot_rows_dense[0].p;
    A.n_rows = (int64_t)P->d_dot_rows_dense[0].n;
    A.ld = P->d_ld_dense.p;
    // upper form: the mirrored squares hold whole rows; the float64 sweeps' zero-lower-triangle storage is read as it is
    // (entries left of the diagonal from the column above it), so that a product between sweeps converts nothing
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
int launch_ld_dot<DOT_U>(viprs_plan* P, int float_dtype, int n_cols, const void* dB, void* dY, double dq_scale,
                         int include_diagonal) {
    if (float_dtype == VIPRS_F32) return launch_typed<float, DOT_U>(P, n_cols, dB, dY, dq_scale, include_diagonal);
    return launch_typed<double, DOT_U>(P, n_cols, dB, dY, dq_scale, include_diagonal);
}

}  // namespace viprs
