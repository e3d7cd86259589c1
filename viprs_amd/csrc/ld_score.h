// LD scores (include/viprs_hip.h, viprs_plan_ld_scores) as an operation on the row stream: per row j and column g of the
// weights A the two sums
//     S2[j, g] = sum p_ji A[i, g],  p = fl(x x), x = T(stored element)        S0[j, g] = sum A[i, g]
// over the off-diagonal entries (j, i) of the row, then the epilogue of the header on lane 0.  The traversal, the storage
// modes and THE ORDER are those of ld_rows.h: an entry adds to S2 by one fused multiply-add fma(p, a, acc) and to S0 by a
// plain addition.  The diagonal and the columns of the window that hold no entry add an exact zero to both sums (their
// weight is read as zero).
//
// UNIT (A == NULL: one column of ones) loads no weights: S2 = sum p in THE ORDER; S0 is the number of entries, counted in
// integers (the ordered sum of that many ones in T is the same number as long as it is below 2^24: a row of an LD block).
#pragma once
#include "ld_rows.h"

namespace viprs {

template <typename T> struct ScoreArgs : RowArgs {
    const T* A;                    // (m, n_cols) column-major; unused by the UNIT kernels
    const double* corr;            // (m,) or null
    T* Y;                          // (m, n_cols)
    int n_cols;
    T scale;                       // fl(dq_scale)
};

template <typename T_, bool UNIT> struct ScoreOp {
    using T = T_;
    using Args = ScoreArgs<T>;
    static constexpr int kSums = UNIT ? 1 : 2;                  // S2 and, with weights, S0
    static constexpr bool kOperand = !UNIT;
    static constexpr bool kMaskOperand = true;                  // S0 counts the weights of the entries only
    // 4-byte LD elements: without the barrier the scheduler waits for each row load before it issues the next and a
    // wavefront keeps one load in flight instead of R (measured on cfg3, unit weights, fp32 LD: 1.05-1.09 x the product's
    // time without it, 1.00 x with it; int8 LD, whose rows the compiler already overlaps with the conversions: 7 % slower
    // with it, so it stays out there)
    static constexpr int row_loads(int V) { return V <= 4 ? kRowLoadsFenced : kRowLoadsFirst; }
    static __device__ __forceinline__ const T* operand(const Args& A) { return A.A; }
    static __device__ __forceinline__ T element(T x) { return x * x; }
    template <int V> static __device__ __forceinline__ void add(T (&acc)[kSums][V], int v, T p) { acc[0][v] = acc[0][v] + p; }
    template <int V> static __device__ __forceinline__ void add(T (&acc)[kSums][V], int v, T p, T a) {
        static_assert(!UNIT && V > 0, "unit weights carry no operand and one sum");
        acc[0][v] = dot_fma<T>(p, a, acc[0][v]);
        acc[kSums - 1][v] = acc[kSums - 1][v] + a;
    }
    static __device__ __forceinline__ void store(const Args& A, int64_t j, int64_t at, const T (&s)[kSums], int n) {
        const T d2 = A.scale * A.scale;                         // every operation separately rounded (no contraction)
        const T self = UNIT ? (T)1 : A.A[at];                   // the diagonal: r_jj = 1, no correction
        const T s0 = UNIT ? (T)n : s[kSums - 1];
        T y = d2 * s[0];
        if (A.corr) {
            const T c = (T)A.corr[j];
            T t = y - s0;
            t = c * t;
            y = y + t;
        }
        A.Y[at] = y + self;
    }
};

}  // namespace viprs
