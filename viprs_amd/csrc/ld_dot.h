// LD product Y = R B (include/viprs_hip.h, viprs_plan_dot) as an operation on the row stream: the traversal, the storage
// modes and THE ORDER are those of ld_rows.h.  An entry is ONE fused multiply-add fma(x, b, acc) in the state precision.
#pragma once
#include "ld_rows.h"

namespace viprs {

template <typename T> struct DotArgs : RowArgs {
    const T* B;                    // (m, n_cols) column-major
    T* Y;
    int n_cols;
    T scale;
    int include_diagonal;
};

template <typename T_> struct DotOp {
    using T = T_;
    using Args = DotArgs<T>;
    static constexpr int kSums = 1;
    static constexpr bool kOperand = true;
    static constexpr bool kMaskOperand = false;                 // x is zero wherever the row has no entry
    static constexpr int row_loads(int) { return kRowLoadsConverted; }
    static __device__ __forceinline__ const T* operand(const Args& A) { return A.B; }
    static __device__ __forceinline__ T element(T x) { return x; }
    template <int V> static __device__ __forceinline__ void add(T (&acc)[1][V], int v, T x, T b) {
        acc[0][v] = dot_fma<T>(x, b, acc[0][v]);
    }
    static __device__ __forceinline__ void store(const Args& A, int64_t, int64_t at, const T (&s)[1], int) {
        T y = A.scale * s[0];                                   // two separately rounded operations (no contraction)
        if (A.include_diagonal) y = y + A.B[at];
        A.Y[at] = y;
    }
};

}  // namespace viprs
