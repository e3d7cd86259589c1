// LD scores (include/viprs_hip.h, viprs_plan_ld_scores): per row j and column g of the weights A the two sums
//     S2[j, g] = sum p_ji A[i, g],  p = fl(x x), x = T(stored element)        S0[j, g] = sum A[i, g]
// over the off-diagonal entries (j, i) of the row, then the epilogue of the header on lane 0.  The work list, the block
// descriptors, the four storage modes and THE ORDER are those of the product (ld_dot.h): entry e of the row's window goes
// to accumulator e % V of lane (e / V) % 64 in ascending e -- S2 by one fused multiply-add fma(p, a, acc), S0 by a plain
// addition --, then the binary tree over V and the xor butterfly over the lanes.  The diagonal and the columns of the
// window that hold no entry add an exact zero to both sums (their weight is read as zero).
//
// UNIT (A == NULL: one column of ones) loads no weights: S2 = sum p in THE ORDER; S0 is the number of entries, counted in
// integers (the ordered sum of that many ones in T is the same number as long as it is below 2^24: a row of an LD block).
#pragma once
#include "ld_dot.h"

namespace viprs {

template <typename T> struct ScoreArgs {
    const BlockDesc* blocks;       // as DotArgs
    const int64_t* rows;
    int64_t n_rows;
    const void* ld;
    const int64_t* ip;
    const int32_t* lb;
    const int32_t* first;
    int64_t m;
    const T* A;                    // (m, n_cols) column-major; unused by the UNIT kernels
    const double* corr;            // (m,) or null
    T* Y;                          // (m, n_cols)
    int n_cols;
    T scale;                       // fl(dq_scale)
};

// rows a wavefront of the dense kernel carries at once: as dot_rows_per_wave with the accumulators counted twice (S2 and
// S0) when the weights are carried
template <typename T, typename U, int NC, bool UNIT> constexpr int score_rows_per_wave() {
    constexpr int V = 16 / (int)sizeof(U);
    constexpr int w = (int)sizeof(T) / 4;
    constexpr int n_acc = (UNIT ? 1 : 2) * NC * V * w;
    constexpr int by_acc = n_acc <= 32 ? 4 : (n_acc <= 64 ? 2 : 1);
    constexpr int by_elems = V * w <= 8 ? 4 : (V * w <= 16 ? 2 : 1);
    return by_acc < by_elems ? by_acc : by_elems;
}

template <typename T, int NC, int V>
__device__ __forceinline__ void score_reduce(T (&acc)[NC][V], T (&s)[NC]) {
#pragma unroll
    for (int g = 0; g < NC; ++g) {
#pragma unroll
        for (int w = V / 2; w >= 1; w >>= 1)
#pragma unroll
            for (int v = 0; v < w; ++v) acc[g][v] = acc[g][v] + acc[g][v + w];
        T t = acc[g][0];
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) t = t + __shfl_xor(t, w, 64);
        s[g] = t;
    }
}

// dense block whose square holds whole rows: columns [g0, g0 + NC) of the R rows r0 .. r0 + R - 1 (rows past the block's end
// repeat its last row and are not stored)
template <typename T, typename U, int NC, int R, bool UNIT>
__device__ __forceinline__ void score_rows_dense(const ScoreArgs<T>& A, const BlockDesc& bd, int r0, int g0,
                                                 T (&s2)[R][NC], T (&s0)[R][NC]) {
    constexpr int V = 16 / (int)sizeof(U);
    typedef U LV __attribute__((ext_vector_type(V)));
    const int lane = threadIdx.x & 63;
    const int64_t m = A.m;
    const int b = bd.size;
    T acc2[R][NC][V];
    T acc0[UNIT ? 1 : R][NC][V];
    int rr[R];
    const U* __restrict__ row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        rr[i] = min(r0 + i, b - 1);
        row[i] = static_cast<const U*>(A.ld) + bd.ld_off + (int64_t)rr[i] * bd.stride;
#pragma unroll
        for (int g = 0; g < NC; ++g)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                acc2[i][g][v] = (T)0;
                if constexpr (!UNIT) acc0[i][g][v] = (T)0;
            }
    }
    const T* __restrict__ Ab = UNIT ? nullptr : A.A + bd.start + (int64_t)g0 * m;
    for (int e0 = lane * V; e0 < b; e0 += 64 * V) {
        // (16-byte aligned and inside the padded row: ld_off and stride are multiples of 64 elements)
        // the R row loads go out together, then the arithmetic.  4-byte LD elements: without the barrier the scheduler waits
        // for each load before it issues the next and a wavefront keeps one load in flight instead of R (measured on cfg3,
        // unit weights, fp32 LD: 1.05-1.09 x the product's time without it, 1.00 x with it; int8 LD, whose rows the
        // compiler already overlaps with the conversions: 7 % slower with it, so it stays out there)
        LV lv[R];
#pragma unroll
        for (int i = 0; i < R; ++i) lv[i] = *reinterpret_cast<const LV*>(row[i] + e0);
        if constexpr (V <= 4) __builtin_amdgcn_sched_barrier(0);
        T p[R][V];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const T x = (e0 + v == rr[i] || e0 + v >= b) ? (T)0 : (T)lv[i][v];
                p[i][v] = x * x;
            }
        if constexpr (UNIT) {
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int v = 0; v < V; ++v) acc2[i][0][v] = acc2[i][0][v] + p[i][v];
        } else {
#pragma unroll
            for (int g = 0; g < NC; ++g) {
                DotVec<T, V> av;
                if (e0 + V <= b) {
                    __builtin_memcpy(&av, Ab + (int64_t)g * m + e0, sizeof(av));
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) av.x[v] = (e0 + v < b) ? Ab[(int64_t)g * m + e0 + v] : (T)0;
                }
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const T a = e0 + v == rr[i] ? (T)0 : av.x[v];        // the diagonal is no entry
                        acc2[i][g][v] = dot_fma<T>(p[i][v], a, acc2[i][g][v]);
                        acc0[i][g][v] = acc0[i][g][v] + a;
                    }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        score_reduce<T, NC, V>(acc2[i], s2[i]);
        if constexpr (UNIT) s0[i][0] = (T)(b - 1);
        else score_reduce<T, NC, V>(acc0[i], s0[i]);
    }
}

// columns [g0, g0 + NC) of one row read through the row's accessor; every lane returns with the row's sums
template <typename T, typename U, int NC, int MODE, bool UNIT>
__device__ __forceinline__ void score_row(const ScoreArgs<T>& A, const BlockDesc& bd, int r, int g0, T (&s2)[NC], T (&s0)[NC]) {
    constexpr int V = 16 / (int)sizeof(U);
    static_assert(MODE != kDotDense, "dense squares with whole rows: score_rows_dense");
    const int lane = threadIdx.x & 63;
    const int64_t m = A.m;
    T acc2[NC][V];
    T acc0[NC][V];
    int count = 0;
#pragma unroll
    for (int g = 0; g < NC; ++g)
#pragma unroll
        for (int v = 0; v < V; ++v) { acc2[g][v] = (T)0; acc0[g][v] = (T)0; }

    const U* __restrict__ ld = static_cast<const U*>(A.ld);
    const int64_t j = (int64_t)bd.start + r;
    int64_t c_lo;
    int W, dpos;                                    // window width, position of the diagonal inside it
    int64_t own = 0;                                // start of row j's own entries
    if constexpr (MODE == kDotDenseGather) {
        c_lo = bd.start; W = bd.size; dpos = r;
    } else if constexpr (MODE == kDotWindowSym) {
        own = A.ip[j];
        c_lo = A.lb[j]; W = (int)(A.ip[j + 1] - own); dpos = (int)(j - c_lo);
    } else {
        own = A.ip[j];
        c_lo = A.first[j]; dpos = (int)(j - c_lo); W = dpos + 1 + (int)(A.ip[j + 1] - own);
    }
    const T* __restrict__ Ab = UNIT ? nullptr : A.A + c_lo + (int64_t)g0 * m;
    for (int e0 = lane * V; e0 < W; e0 += 64 * V) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = e0 + v;
            T x = (T)0;
            bool entry = false;
            if (e < W && e != dpos) {
                if constexpr (MODE == kDotDenseGather) {
                    entry = true;
                    x = e < r ? (T)ld[bd.ld_off + (int64_t)e * bd.stride + r] : (T)ld[bd.ld_off + (int64_t)r * bd.stride + e];
                } else if constexpr (MODE == kDotWindowSym) {
                    entry = true;
                    x = (T)ld[own + e];
                } else {
                    if (e > dpos) {
                        entry = true;
                        x = (T)ld[own + (e - dpos - 1)];
                    } else {
                        const int64_t i = c_lo + e, s = A.ip[i];            // row i above j: does it reach j?
                        if (i + (A.ip[i + 1] - s) >= j) { entry = true; x = (T)ld[s + (j - i - 1)]; }
                    }
                }
            }
            const T p = x * x;
            if constexpr (UNIT) {
                acc2[0][v] = acc2[0][v] + p;
                count += entry ? 1 : 0;
            } else {
#pragma unroll
                for (int g = 0; g < NC; ++g) {
                    const T a = entry ? Ab[(int64_t)g * m + e] : (T)0;
                    acc2[g][v] = dot_fma<T>(p, a, acc2[g][v]);
                    acc0[g][v] = acc0[g][v] + a;
                }
            }
        }
    }
    score_reduce<T, NC, V>(acc2, s2);
    if constexpr (UNIT) {
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) count += __shfl_xor(count, w, 64);
        s0[0] = (T)count;
    } else {
        score_reduce<T, NC, V>(acc0, s0);
    }
}

template <typename T, typename U, int NC, int MODE, int R, bool UNIT>
__device__ __forceinline__ void score_row_store(const ScoreArgs<T>& A, const BlockDesc& bd, int r, int g0) {
    T s2[R][NC], s0[R][NC];
    if constexpr (MODE == kDotDense) score_rows_dense<T, U, NC, R, UNIT>(A, bd, r, g0, s2, s0);
    else score_row<T, U, NC, MODE, UNIT>(A, bd, r, g0, s2[0], s0[0]);
    if ((threadIdx.x & 63) == 0) {
        const T d2 = A.scale * A.scale;                     // every operation separately rounded (no contraction)
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (r + i >= bd.size) break;
            const int64_t j = (int64_t)bd.start + r + i;
#pragma unroll
            for (int g = 0; g < NC; ++g) {
                const int64_t at = j + (int64_t)(g0 + g) * A.m;
                const T self = UNIT ? (T)1 : A.A[at];       // the diagonal: r_jj = 1, no correction
                T y = d2 * s2[i][g];
                if (A.corr) {
                    const T c = (T)A.corr[j];
                    T t = y - s0[i][g];
                    t = c * t;
                    y = y + t;
                }
                A.Y[at] = y + self;
            }
        }
    }
}

// One work item (a row; the dense kernel: R consecutive rows of a block) per wavefront, as ld_dot_kernel.  UNIT: n_cols == 1.
template <typename T, typename U, int NCMAX, int MODE, int R, bool UNIT>
__global__ __launch_bounds__(64 * kDotWaves) void ld_score_kernel(ScoreArgs<T> A) {
    static_assert(R == 1 || MODE == kDotDense, "several rows per wavefront: the dense kernel only");
    static_assert(!UNIT || NCMAX == 1, "unit weights: one column");
    const int64_t item = (int64_t)blockIdx.x * kDotWaves + (threadIdx.x >> 6);
    if (item >= A.n_rows) return;
    const int64_t w = A.rows[item];
    const BlockDesc bd = A.blocks[(int)(w >> 32)];
    const int r = (int)(w & 0xffffffff);
    if constexpr (UNIT) {
        score_row_store<T, U, 1, MODE, R, true>(A, bd, r, 0);
    } else {
        int g0 = 0;
        for (; g0 + NCMAX <= A.n_cols; g0 += NCMAX) score_row_store<T, U, NCMAX, MODE, R, false>(A, bd, r, g0);
        if constexpr (NCMAX > 2) if (g0 + 2 <= A.n_cols) { score_row_store<T, U, 2, MODE, R, false>(A, bd, r, g0); g0 += 2; }
        if constexpr (NCMAX > 1) if (g0 + 1 <= A.n_cols) { score_row_store<T, U, 1, MODE, R, false>(A, bd, r, g0); g0 += 1; }
    }
}

}  // namespace viprs
