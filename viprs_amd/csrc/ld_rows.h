// The row stream over a plan's LD: one wavefront per row of the symmetric matrix the plan stands for, lane-strided partial
// sums, a tree across the lanes.  No serial chain, no atomics: a pure stream over the LD bytes.  What is summed is the
// operation's business (ld_dot.h: the product R B; ld_score.h: the LD scores); how a row is found, read, masked, accumulated
// and reduced is written here, once.
//
// THE ORDER (the contract of include/viprs_hip.h).  A row's entries live in a window of W consecutive columns that starts at
// c_lo (dense block: the block, W = size; windowed row, symmetric form: the stored window; upper form: from the first row that
// reaches j to the end of row j's own entries).  Entry e = c - c_lo goes to lane (e / V) % 64 and to that lane's
// accumulator e % V, V = 16 / sizeof(LD element) (the elements of one 16-byte load); a lane adds its entries to an
// accumulator in ascending e, each by the operation's one step in the state precision (the product: ONE fused multiply-add,
// the element converted exactly and the product not rounded).  The diagonal and columns of the window that hold no entry
// contribute an exact zero.  Then the V accumulators of a lane are summed in a binary tree (log2 V levels), then the 64
// lanes (6 levels, xor butterfly).  Every kernel follows this order, whatever storage it reads, however many columns NC of
// the operand and however many rows R a wavefront carries: a column's result depends on nothing but the row's entries and
// that column.
//
// An operation Op gives
//     T, Args               the state precision; the kernel's arguments (RowArgs and its own)
//     kSums                 accumulators a column costs per element of a load (the rows-per-wave rule counts them)
//     kOperand              a column-major (m, n_cols) operand is carried; false: one column, nothing loaded, the entries of
//                           the row are counted instead
//     kMaskOperand          the operand is read as zero where the row has no entry (false: wherever the window reaches; the
//                           element is zero there anyway)
//     row_loads(V)          dense loop: the order of the R row loads and their conversions in the source (kRowLoads...)
//     operand(A)            the operand's base
//     element(x)            what enters the sums for the converted element x (zero where there is no entry)
//     add(acc, p, a)        one entry: the kSums accumulators, p = element(x), a = the operand (without it when !kOperand)
//     store(A, j, at, s, n) lane 0: the epilogue of row j at Y[at] from the kSums sums s (and the count n of entries)
#pragma once
#include "kernels_common.h"

namespace viprs {

constexpr int kDotWaves = 4;                  // rows (dense kernels: work items of R rows) per workgroup, one wavefront each

struct RowArgs {                   // filled from the plan by the launcher (launch_ld_rows.inc)
    const BlockDesc* blocks;       // every block of the plan: the dense ones first, then the windowed ones
    const int64_t* rows;           // work list: (block of `blocks`) << 32 | (first) row inside the block
    int64_t n_rows;
    const void* ld;                // dense kernels: the repacked squares; window kernel: the caller's row-concatenated layout
    const int64_t* ip;             // window kernel: row starts, left bounds and (upper form) the first row that reaches j
    const int32_t* lb;
    const int32_t* first;
    int64_t m;
};

enum { kDotDense = 0,              // dense block whose square holds every entry of the row (symmetric form, mirrored upper form)
       kDotDenseGather = 1,        // dense block of the upper form with a zero lower triangle: entries left of the diagonal are
                                   // read from the column above it
       kDotWindowSym = 2, kDotWindowUpper = 3 };

// The dense loop's R row loads of a pass and the conversions of their elements, in the order of the source.  What the
// scheduler makes of a pass depends on it, and each operation keeps the order it was measured with (EXPERIMENTS.md 6.16,
// 6.18): every row converted behind its load; all loads, then the conversions; or the same with a scheduling barrier
// between them, which keeps the R loads in flight together.
enum { kRowLoadsConverted = 0, kRowLoadsFirst = 1, kRowLoadsFenced = 2 };

template <typename T> __device__ __forceinline__ T dot_fma(T a, T b, T c);
template <> __device__ __forceinline__ float dot_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <> __device__ __forceinline__ double dot_fma<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }

// rows a wavefront of the dense kernel carries at once: they share every load of the operand and keep R row loads in
// flight; as many as keep the accumulators (rows x n_acc x V, n_acc = columns x the operation's kSums) within 128 and the
// converted elements of one pass (rows x V) within 32 32-bit registers
template <typename T, typename U> constexpr int rows_per_wave(int n_acc) {
    constexpr int V = 16 / (int)sizeof(U);
    constexpr int w = (int)sizeof(T) / 4;
    const int by_acc = n_acc * V * w <= 32 ? 4 : (n_acc * V * w <= 64 ? 2 : 1);
    const int by_elems = V * w <= 8 ? 4 : (V * w <= 16 ? 2 : 1);
    return by_acc < by_elems ? by_acc : by_elems;
}

// the window of row r of a block whose entries are read one by one (row_accessor)
struct RowWindow {
    int64_t c_lo;                  // first column
    int W, dpos;                   // width, position of the diagonal inside it
    int64_t own;                   // start of row j's own entries
};

template <int MODE>
__device__ __forceinline__ RowWindow row_window(const RowArgs& A, const BlockDesc& bd, int r) {
    static_assert(MODE != kDotDense, "dense squares with whole rows: rows_dense");
    const int64_t j = (int64_t)bd.start + r;
    RowWindow w;
    w.own = 0;
    if constexpr (MODE == kDotDenseGather) {
        w.c_lo = bd.start; w.W = bd.size; w.dpos = r;
    } else if constexpr (MODE == kDotWindowSym) {
        w.own = A.ip[j];
        w.c_lo = A.lb[j]; w.W = (int)(A.ip[j + 1] - w.own); w.dpos = (int)(j - w.c_lo);
    } else {
        w.own = A.ip[j];
        w.c_lo = A.first[j]; w.dpos = (int)(j - w.c_lo); w.W = w.dpos + 1 + (int)(A.ip[j + 1] - w.own);
    }
    return w;
}

// The lane reduction: the V accumulators acc[0..V) of a lane in a binary tree, then the 64 lanes (xor butterfly); every lane
// ends with the sum in `out`.  A macro -- and the operand load and the accessor sit inside their loops -- because the
// compiler schedules a helper function differently even when it inlines it.  With these three as __forceinline__ functions
// most of the product's kernels came out in another schedule than before the traversal was shared, some of them up to 3 %
// slower; written in place, all 112 are instruction for instruction what they were (EXPERIMENTS.md 6.18).
#define VIPRS_LANE_REDUCE(T, V, acc, out)                                                  \
    do {                                                                                   \
        _Pragma("unroll") for (int w_ = (V) / 2; w_ >= 1; w_ >>= 1)                        \
            _Pragma("unroll") for (int v_ = 0; v_ < w_; ++v_) (acc)[v_] = (acc)[v_] + (acc)[v_ + w_]; \
        T t_ = (acc)[0];                                                                   \
        _Pragma("unroll") for (int w_ = 1; w_ < 64; w_ <<= 1) t_ = t_ + __shfl_xor(t_, w_, 64); \
        (out) = t_;                                                                        \
    } while (0)

// V consecutive values of a column, the unit of the operand load
template <typename T, int V> struct RowVec { T x[V]; };

// dense block whose square holds whole rows: columns [g0, g0 + NC) of the R rows r0 .. r0 + R - 1 (rows past the block's end
// repeat its last row and are not stored); every row in THE ORDER, whatever R
template <typename Op, typename U, int NC, int R>
__device__ __forceinline__ void rows_dense(const typename Op::Args& A, const BlockDesc& bd, int r0, int g0,
                                           typename Op::T (&s)[R][NC][Op::kSums], int (&n)[R]) {
    using T = typename Op::T;
    constexpr int V = 16 / (int)sizeof(U);
    typedef U LV __attribute__((ext_vector_type(V)));
    const int lane = threadIdx.x & 63;
    const int64_t m = A.m;
    const int b = bd.size;
    T acc[R][NC][Op::kSums][V];
    int rr[R];
    const U* __restrict__ row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        rr[i] = min(r0 + i, b - 1);
        row[i] = static_cast<const U*>(A.ld) + bd.ld_off + (int64_t)rr[i] * bd.stride;
#pragma unroll
        for (int g = 0; g < NC; ++g)
#pragma unroll
            for (int k = 0; k < Op::kSums; ++k)
#pragma unroll
                for (int v = 0; v < V; ++v) acc[i][g][k][v] = (T)0;
    }
    const T* __restrict__ Ab = Op::kOperand ? Op::operand(A) + bd.start + (int64_t)g0 * m : nullptr;
    for (int e0 = lane * V; e0 < b; e0 += 64 * V) {
        // (16-byte aligned and inside the padded row: ld_off and stride are multiples of 64 elements)
        constexpr int kOrder = Op::row_loads(V);
        LV lv[R];
        T p[R][V];
#define VIPRS_CONVERT_ROW(i) \
    _Pragma("unroll") for (int v = 0; v < V; ++v) p[i][v] = Op::element((e0 + v == rr[i] || e0 + v >= b) ? (T)0 : (T)lv[i][v])
#pragma unroll
        for (int i = 0; i < R; ++i) {
            lv[i] = *reinterpret_cast<const LV*>(row[i] + e0);
            if constexpr (kOrder == kRowLoadsConverted) VIPRS_CONVERT_ROW(i);
        }
        if constexpr (kOrder == kRowLoadsFenced) __builtin_amdgcn_sched_barrier(0);
        if constexpr (kOrder != kRowLoadsConverted) {
#pragma unroll
            for (int i = 0; i < R; ++i) VIPRS_CONVERT_ROW(i);
        }
#undef VIPRS_CONVERT_ROW
        if constexpr (!Op::kOperand) {
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int v = 0; v < V; ++v) Op::add(acc[i][0], v, p[i][v]);
        } else {
#pragma unroll
            for (int g = 0; g < NC; ++g) {
                // the operand load: one 16-byte copy, or element by element with zeros beyond the block's end
                RowVec<T, V> av;
                if (e0 + V <= b) {
                    __builtin_memcpy(&av, Ab + (int64_t)g * m + e0, sizeof(av));
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) av.x[v] = (e0 + v < b) ? Ab[(int64_t)g * m + e0 + v] : (T)0;
                }
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int v = 0; v < V; ++v)         // (the diagonal is no entry)
                        Op::add(acc[i][g], v, p[i][v], (Op::kMaskOperand && e0 + v == rr[i]) ? (T)0 : av.x[v]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        n[i] = b - 1;
#pragma unroll
        for (int k = 0; k < Op::kSums; ++k)
#pragma unroll
            for (int g = 0; g < NC; ++g) VIPRS_LANE_REDUCE(T, V, acc[i][g][k], s[i][g][k]);
    }
}

// columns [g0, g0 + NC) of one row read through the row's accessor; every lane returns with the row's sums in s[] and, when
// no operand is carried, the number of its entries in n
template <typename Op, typename U, int NC, int MODE>
__device__ __forceinline__ void row_accessor(const typename Op::Args& A, const BlockDesc& bd, int r, int g0,
                                             typename Op::T (&s)[NC][Op::kSums], int& n) {
    using T = typename Op::T;
    constexpr int V = 16 / (int)sizeof(U);
    const int lane = threadIdx.x & 63;
    const int64_t m = A.m;
    T acc[NC][Op::kSums][V];
    int count = 0;
#pragma unroll
    for (int g = 0; g < NC; ++g)
#pragma unroll
        for (int k = 0; k < Op::kSums; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[g][k][v] = (T)0;
    const U* __restrict__ ld = static_cast<const U*>(A.ld);
    const int64_t j = (int64_t)bd.start + r;
    const RowWindow w = row_window<MODE>(A, bd, r);
    const T* __restrict__ Ab = Op::kOperand ? Op::operand(A) + w.c_lo + (int64_t)g0 * m : nullptr;
    for (int e0 = lane * V; e0 < w.W; e0 += 64 * V) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = e0 + v;
            // the accessor: is there an entry at position e, and x = T(stored) (zero when there is none).  (In place, see
            // VIPRS_LANE_REDUCE: as a function the two loads of the gather mode become one load from a selected address)
            T x = (T)0;
            bool entry = false;
            if (e < w.W && e != w.dpos) {
                if constexpr (MODE == kDotDenseGather) {
                    entry = true;
                    x = e < r ? (T)ld[bd.ld_off + (int64_t)e * bd.stride + r] : (T)ld[bd.ld_off + (int64_t)r * bd.stride + e];
                } else if constexpr (MODE == kDotWindowSym) {
                    entry = true;
                    x = (T)ld[w.own + e];
                } else if (e > w.dpos) {
                    entry = true;
                    x = (T)ld[w.own + (e - w.dpos - 1)];
                } else {
                    const int64_t i = w.c_lo + e, s0 = A.ip[i];            // row i above j: does it reach j?
                    if (i + (A.ip[i + 1] - s0) >= j) { entry = true; x = (T)ld[s0 + (j - i - 1)]; }
                }
            }
            const T p = Op::element(x);
            if constexpr (!Op::kOperand) {
                Op::add(acc[0], v, p);
                count += entry ? 1 : 0;
            } else {
#pragma unroll
                for (int g = 0; g < NC; ++g)
                    Op::add(acc[g], v, p, (Op::kMaskOperand ? entry : e < w.W) ? Ab[(int64_t)g * m + e] : (T)0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < Op::kSums; ++k)
#pragma unroll
        for (int g = 0; g < NC; ++g) VIPRS_LANE_REDUCE(T, V, acc[g][k], s[g][k]);
    if constexpr (!Op::kOperand) {
#pragma unroll
        for (int w2 = 1; w2 < 64; w2 <<= 1) count += __shfl_xor(count, w2, 64);
    }
    n = count;
}

template <typename Op, typename U, int NC, int MODE, int R>
__device__ __forceinline__ void rows_store(const typename Op::Args& A, const BlockDesc& bd, int r, int g0) {
    typename Op::T s[R][NC][Op::kSums];
    int n[R];
    if constexpr (MODE == kDotDense) rows_dense<Op, U, NC, R>(A, bd, r, g0, s, n);
    else row_accessor<Op, U, NC, MODE>(A, bd, r, g0, s[0], n[0]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (r + i >= bd.size) break;
            const int64_t j = (int64_t)bd.start + r + i;
#pragma unroll
            for (int g = 0; g < NC; ++g) Op::store(A, j, j + (int64_t)(g0 + g) * A.m, s[i][g], n[i]);
        }
    }
}

// One work item (a row; the dense kernel: R consecutive rows of a block) per wavefront.  NCMAX columns per pass over the
// row(s), the remainder in passes of NCMAX / 2, ..., 1 columns.  R = 1 for every mode but kDotDense.
template <typename Op, typename U, int NCMAX, int MODE, int R>
__global__ __launch_bounds__(64 * kDotWaves) void ld_rows_kernel(typename Op::Args A) {
    static_assert(R == 1 || MODE == kDotDense, "several rows per wavefront: the dense kernel only");
    static_assert(Op::kOperand || NCMAX == 1, "no operand: one column");
    const int64_t item = (int64_t)blockIdx.x * kDotWaves + (threadIdx.x >> 6);
    if (item >= A.n_rows) return;
    const int64_t w = A.rows[item];
    const BlockDesc bd = A.blocks[(int)(w >> 32)];
    const int r = (int)(w & 0xffffffff);
    if constexpr (!Op::kOperand) {
        rows_store<Op, U, 1, MODE, R>(A, bd, r, 0);
    } else {
        int g0 = 0;
        for (; g0 + NCMAX <= A.n_cols; g0 += NCMAX) rows_store<Op, U, NCMAX, MODE, R>(A, bd, r, g0);
        if constexpr (NCMAX > 4) if (g0 + 4 <= A.n_cols) { rows_store<Op, U, 4, MODE, R>(A, bd, r, g0); g0 += 4; }
        if constexpr (NCMAX > 2) if (g0 + 2 <= A.n_cols) { rows_store<Op, U, 2, MODE, R>(A, bd, r, g0); g0 += 2; }
        if constexpr (NCMAX > 1) if (g0 + 1 <= A.n_cols) { rows_store<Op, U, 1, MODE, R>(A, bd, r, g0); g0 += 1; }
    }
}

#undef VIPRS_LANE_REDUCE

}  // namespace viprs
