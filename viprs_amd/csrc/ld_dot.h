// LD product Y = R B (include/viprs_hip.h, viprs_plan_dot): one wavefront per row of the symmetric matrix the plan stands
// for, lane-strided partial sums, a tree across the lanes.  No serial chain, no atomics: a pure stream over the LD bytes.
//
// THE ORDER (the contract of the header).  A row's entries live in a window of W consecutive columns that starts at c_lo
// (dense block: the block, W = size; windowed row, symmetric form: the stored window; upper form: from the first row that
// reaches j to the end of row j's own entries).  Entry e = c - c_lo goes to lane (e / V) % 64 and to that lane's
// accumulator e % V, V = 16 / sizeof(LD element) (the elements of one 16-byte load); a lane adds its entries to an
// accumulator in ascending e, each by ONE fused multiply-add in the state precision (the product is not rounded; integer LD
// is converted exactly).  The diagonal and columns of the window that hold no entry contribute an exact zero.  Then the V
// accumulators of a lane are summed in a binary tree (log2 V levels), then the 64 lanes (6 levels, xor butterfly).
// Every kernel below follows this order, whatever storage it reads and however many columns of B it carries: a column's
// result depends on nothing but the row's entries and that column.
#pragma once
#include "kernels_common.h"

namespace viprs {

constexpr int kDotWaves = 4;                  // rows per workgroup (one wavefront each)

template <typename T> struct DotArgs {
    const BlockDesc* blocks;       // every block of the plan: the dense ones first, then the windowed ones
    const int64_t* rows;           // work list: (block of `blocks`) << 32 | (first) row inside the block
    int64_t n_rows;
    const void* ld;                // dense kernels: the repacked squares; window kernel: the caller's row-concatenated layout
    const int64_t* ip;             // window kernel: row starts, left bounds and (upper form) the first row that reaches j
    const int32_t* lb;
    const int32_t* first;
    int64_t m;
    const T* B;                    // (m, n_cols) column-major
    T* Y;
    int n_cols;
    T scale;
    int include_diagonal;
};

enum { kDotDense = 0,              // dense block whose square holds every entry of the row (symmetric form, mirrored upper form)
       kDotDenseGather = 1,        // dense block of the upper form with a zero lower triangle: entries left of the diagonal are
                                   // read from the column above it
       kDotWindowSym = 2, kDotWindowUpper = 3 };

template <typename T> __device__ __forceinline__ T dot_fma(T a, T b, T c);
template <> __device__ __forceinline__ float dot_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> __device__ __forceinline__ double dot_fma<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T, int V> struct DotVec { T x[V]; };

// rows a wavefront of the dense kernel carries at once: they share every load of B and keep R row loads in flight; as many
// as keep the accumulators (rows x columns x V) within 128 and the converted elements of one pass (rows x V) within 32
// 32-bit registers
template <typename T, typename U, int NC> constexpr int dot_rows_per_wave() {
    constexpr int V = 16 / (int)sizeof(U);
    constexpr int w = (int)sizeof(T) / 4;
    constexpr int by_acc = NC * V * w <= 32 ? 4 : (NC * V * w <= 64 ? 2 : 1);
    constexpr int by_elems = V * w <= 8 ? 4 : (V * w <= 16 ? 2 : 1);
    return by_acc < by_elems ? by_acc : by_elems;
}

// dense block whose square holds whole rows: columns [g0, g0 + NC) of the R rows r0 .. r0 + R - 1 (rows past the block's end
// repeat its last row and are not stored); every row in THE ORDER above, whatever R
template <typename T, typename U, int NC, int R>
__device__ __forceinline__ void dot_rows_dense(const DotArgs<T>& A, const BlockDesc& bd, int r0, int g0, T (&s)[R][NC]) {
    constexpr int V = 16 / (int)sizeof(U);
    typedef U LV __attribute__((ext_vector_type(V)));
    const int lane = threadIdx.x & 63;
    const int64_t m = A.m;
    const int b = bd.size;
    T acc[R][NC][V];
    int rr[R];
    const U* __restrict__ row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        rr[i] = min(r0 + i, b - 1);
        row[i] = static_cast<const U*>(A.ld) + bd.ld_off + (int64_t)rr[i] * bd.stride;
#pragma unroll
        for (int g = 0; g < NC; ++g)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[i][g][v] = (T)0;
    }
    const T* __restrict__ Bb = A.B + bd.start + (int64_t)g0 * m;
    for (int e0 = lane * V; e0 < b; e0 += 64 * V) {
        // (16-byte aligned and inside the padded row: ld_off and stride are multiples of 64 elements)
        T x[R][V];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const LV lv = *reinterpret_cast<const LV*>(row[i] + e0);
#pragma unroll
            for (int v = 0; v < V; ++v) x[i][v] = (e0 + v == rr[i] || e0 + v >= b) ? (T)0 : (T)lv[v];
        }
#pragma unroll
        for (int g = 0; g < NC; ++g) {
            DotVec<T, V> bv;
            if (e0 + V <= b) {
                __builtin_memcpy(&bv, Bb + (int64_t)g * m + e0, sizeof(bv));
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) bv.x[v] = (e0 + v < b) ? Bb[(int64_t)g * m + e0 + v] : (T)0;
            }
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int v = 0; v < V; ++v) acc[i][g][v] = dot_fma<T>(x[i][v], bv.x[v], acc[i][g][v]);
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int g = 0; g < NC; ++g) {
#pragma unroll
            for (int w = V / 2; w >= 1; w >>= 1)
#pragma unroll
                for (int v = 0; v < w; ++v) acc[i][g][v] = acc[i][g][v] + acc[i][g][v + w];
            T t = acc[i][g][0];
#pragma unroll
            for (int w = 1; w < 64; w <<= 1) t = t + __shfl_xor(t, w, 64);
            s[i][g] = t;
        }
}

// columns [g0, g0 + NC) of one row; every lane returns with the row's sums in s[]
template <typename T, typename U, int NC, int MODE>
__device__ __forceinline__ void dot_row(const DotArgs<T>& A, const BlockDesc& bd, int r, int g0, T (&s)[NC]) {
    constexpr int V = 16 / (int)sizeof(U);
    const int lane = threadIdx.x & 63;
    const int64_t m = A.m;
    T acc[NC][V];
#pragma unroll
    for (int g = 0; g < NC; ++g)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[g][v] = (T)0;

    static_assert(MODE != kDotDense, "dense squares with whole rows: dot_rows_dense");
    {
        // element loads through the row's accessor; the same (lane, accumulator) for every entry as above
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
        const T* __restrict__ Bb = A.B + c_lo + (int64_t)g0 * m;
        for (int e0 = lane * V; e0 < W; e0 += 64 * V) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int e = e0 + v;
                T x = (T)0;
                if (e < W && e != dpos) {
                    if constexpr (MODE == kDotDenseGather) {
                        x = e < r ? (T)ld[bd.ld_off + (int64_t)e * bd.stride + r] : (T)ld[bd.ld_off + (int64_t)r * bd.stride + e];
                    } else if constexpr (MODE == kDotWindowSym) {
                        x = (T)ld[own + e];
                    } else {
                        if (e > dpos) {
                            x = (T)ld[own + (e - dpos - 1)];
                        } else {
                            const int64_t i = c_lo + e, s0 = A.ip[i];            // row i above j: does it reach j?
                            if (i + (A.ip[i + 1] - s0) >= j) x = (T)ld[s0 + (j - i - 1)];
                        }
                    }
                }
#pragma unroll
                for (int g = 0; g < NC; ++g) {
                    const T bval = e < W ? Bb[(int64_t)g * m + e] : (T)0;
                    acc[g][v] = dot_fma<T>(x, bval, acc[g][v]);
                }
            }
        }
    }
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

template <typename T, typename U, int NC, int MODE, int R>
__device__ __forceinline__ void dot_row_store(const DotArgs<T>& A, const BlockDesc& bd, int r, int g0) {
    T s[R][NC];
    if constexpr (MODE == kDotDense) dot_rows_dense<T, U, NC, R>(A, bd, r, g0, s);
    else dot_row<T, U, NC, MODE>(A, bd, r, g0, s[0]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (r + i >= bd.size) break;
            const int64_t j = (int64_t)bd.start + r + i;
#pragma unroll
            for (int g = 0; g < NC; ++g) {
                const int64_t at = j + (int64_t)(g0 + g) * A.m;
                T y = A.scale * s[i][g];                    // two separately rounded operations (no contraction)
                if (A.include_diagonal) y = y + A.B[at];
                A.Y[at] = y;
            }
        }
    }
}

// One work item (a row; the dense kernel: R consecutive rows of a block) per wavefront.  NCMAX columns per pass over the
// row(s), the remainder in passes of NCMAX / 2, ..., 1 columns.  R = 1 for every mode but kDotDense.
template <typename T, typename U, int NCMAX, int MODE, int R>
__global__ __launch_bounds__(64 * kDotWaves) void ld_dot_kernel(DotArgs<T> A) {
    static_assert(R == 1 || MODE == kDotDense, "several rows per wavefront: the dense kernel only");
    const int64_t item = (int64_t)blockIdx.x * kDotWaves + (threadIdx.x >> 6);
    if (item >= A.n_rows) return;
    const int64_t w = A.rows[item];
    const BlockDesc bd = A.blocks[(int)(w >> 32)];
    const int r = (int)(w & 0xffffffff);
    int g0 = 0;
    for (; g0 + NCMAX <= A.n_cols; g0 += NCMAX) dot_row_store<T, U, NCMAX, MODE, R>(A, bd, r, g0);
    if constexpr (NCMAX > 4) if (g0 + 4 <= A.n_cols) { dot_row_store<T, U, 4, MODE, R>(A, bd, r, g0); g0 += 4; }
    if constexpr (NCMAX > 2) if (g0 + 2 <= A.n_cols) { dot_row_store<T, U, 2, MODE, R>(A, bd, r, g0); g0 += 2; }
    if constexpr (NCMAX > 1) if (g0 + 1 <= A.n_cols) { dot_row_store<T, U, 1, MODE, R>(A, bd, r, g0); g0 += 1; }
}

}  // namespace viprs
