// Greedy LD clumping (include/viprs_hip.h, viprs_plan_clump): one workgroup per LD block walks the block's piece of the
// processing order; every SNP it finds available in some column becomes an index SNP of those columns and claims the
// available SNPs of its row whose stored element x passes (double)x (double)x >= thr[g].  LD blocks share no entry, so
// nothing crosses workgroups: __syncthreads() is the only synchronisation, no spin, no flag, no atomics.
//
// AVAILABILITY.  mask[k], one 32-bit word per SNP in global memory: bit g set = SNP k is NOT available in column g.  The
// host sets the bits >= n_cols and every bit of a non-member, so "nothing free" is ~0u whatever n_cols is.
//
// A STEP.  Every wavefront runs the same scan of the order from `pos`, 64 candidates at a time (mask word, ballot, first
// lane with a free bit): all of them find the same index SNP j with the same free columns, with no barrier between scan and
// row.  That holds because nothing a step writes can change what a scan of the SAME step reads at or before j's position:
// the candidates in front of j have no free bit (a step only sets bits), and j's own word is not written in its own step --
// its commit (mask[j] = ~0u, index_of[j, g] = j) is thread 0's first act of the NEXT step, and the row phase of that step
// takes k == previous j as unavailable instead of reading its word.  Then the workgroup streams row j once for all free
// columns: each thread owns the entries it loads, tests them, and writes their mask word and index_of values.  A barrier
// ends the step (workgroup-scope release / acquire: the next step's loads see this step's stores).
//
// ROWS.  kDotDense: 16-byte loads of V = 16 / sizeof(U) elements from the padded square (ld_off and stride are multiples of
// 64 elements: a load that starts inside the row ends inside its padding).  The other three storages read entry by entry
// through row_window and the accessor of ld_rows.h, written in place here.
#pragma once
#include "ld_rows.h"

namespace viprs {

// 4 wavefronts.  A step is a chain of dependent latencies (order -> mask -> ballot -> row -> mask -> barrier), not a stream:
// one pass of 256 threads x 16 bytes covers a row of 4 096 int8 / 1 024 fp32 elements, which is most blocks of a genome in
// one or two passes; more wavefronts would repeat the scan and lengthen the barrier without shortening the chain.
constexpr int kClumpThreads = 256;
constexpr int kClumpMaxCols = 32;

struct ClumpArgs : RowArgs {
    int block0;                    // the launch covers blocks[block0 + blockIdx.x]
    const int32_t* order;          // the order, split stably by block of `blocks`
    const int64_t* order_off;      // piece of block k: order[order_off[k] .. order_off[k + 1])
    const double* thr;             // n_cols thresholds on (double)x (double)x
    int n_cols;
    uint32_t* mask;                // (m,)
    int32_t* index_of;             // (m, n_cols) column-major
};

// entry (j, k) with stored element x: claim k for j in the columns of `free` where it passes and k is available
template <typename U>
__device__ __forceinline__ void clump_entry(const ClumpArgs& A, const double* thr, int32_t j, int64_t k, U x, uint32_t free,
                                            int32_t prev_j) {
    const double xd = (double)x;
    const double p = xd * xd;
    uint32_t pass = 0;
    for (int g = 0; g < A.n_cols; ++g) pass |= (p >= thr[g] ? 1u : 0u) << g;
    pass &= free;
    if (pass == 0 || k == (int64_t)prev_j) return;
    const uint32_t mk = A.mask[k];
    uint32_t claim = pass & ~mk;
    if (claim == 0) return;
    A.mask[k] = mk | claim;
    while (claim) {
        const int g = __builtin_ctz(claim);
        claim &= claim - 1;
        A.index_of[k + (int64_t)g * A.m] = j;
    }
}

template <typename U, int MODE>
__global__ __launch_bounds__(kClumpThreads) void ld_clump_kernel(ClumpArgs A) {
    constexpr int V = 16 / (int)sizeof(U);
    typedef U LV __attribute__((ext_vector_type(V)));
    __shared__ double thr[kClumpMaxCols];          // (LDS: no store of the kernel can alias it, every lane reads the same word)
    if ((int)threadIdx.x < A.n_cols) thr[threadIdx.x] = A.thr[threadIdx.x];
    __syncthreads();
    const int kb = A.block0 + (int)blockIdx.x;
    const BlockDesc bd = A.blocks[kb];
    const int32_t* __restrict__ order = A.order + A.order_off[kb];
    const int n = (int)(A.order_off[kb + 1] - A.order_off[kb]);
    const int lane = threadIdx.x & 63;
    const U* __restrict__ ld = static_cast<const U*>(A.ld);
    int pos = 0;
    int32_t prev_j = -1;
    uint32_t prev_free = 0;
    for (;;) {
        // the scan: the first candidate at or behind `pos` with a free column
        int32_t j = -1;
        uint32_t free = 0;
        for (; pos < n; pos += 64) {
            const int32_t cand = pos + lane < n ? order[pos + lane] : -1;
            const uint32_t w = cand >= 0 ? A.mask[cand] : ~0u;
            const unsigned long long open = __ballot(w != ~0u);
            if (open) {
                const int first = __builtin_ctzll(open);
                j = __shfl(cand, first, 64);
                free = ~(uint32_t)__shfl((int)w, first, 64);
                pos += first + 1;
                break;
            }
        }
        // the commit of the previous step's index SNP (see A STEP)
        if (threadIdx.x == 0 && prev_j >= 0) {
            A.mask[prev_j] = ~0u;
            for (uint32_t f = prev_free; f; f &= f - 1) A.index_of[prev_j + (int64_t)__builtin_ctz(f) * A.m] = prev_j;
        }
        if (j < 0) break;
        const int r = j - bd.start;
        if constexpr (MODE == kDotDense) {
            const int b = bd.size;
            const U* __restrict__ row = ld + bd.ld_off + (int64_t)r * bd.stride;
            for (int e0 = (int)threadIdx.x * V; e0 < b; e0 += kClumpThreads * V) {
                const LV lv = *reinterpret_cast<const LV*>(row + e0);
#pragma unroll
                for (int v = 0; v < V; ++v)
                    if (e0 + v < b && e0 + v != r) clump_entry<U>(A, thr, j, (int64_t)bd.start + e0 + v, lv[v], free, prev_j);
            }
        } else {
            const RowWindow w = row_window<MODE>(A, bd, r);
            for (int e = (int)threadIdx.x; e < w.W; e += kClumpThreads) {
                if (e == w.dpos) continue;
                // the accessor of ld_rows.h: is there an entry at position e of the window, and its stored element
                U x;
                if constexpr (MODE == kDotDenseGather) {
                    x = e < r ? ld[bd.ld_off + (int64_t)e * bd.stride + r] : ld[bd.ld_off + (int64_t)r * bd.stride + e];
                } else if constexpr (MODE == kDotWindowSym) {
                    x = ld[w.own + e];
                } else if (e > w.dpos) {
                    x = ld[w.own + (e - w.dpos - 1)];
                } else {
                    const int64_t i = w.c_lo + e, s0 = A.ip[i];            // row i above j: does it reach j?
                    if (i + (A.ip[i + 1] - s0) < (int64_t)j) continue;
                    x = ld[s0 + ((int64_t)j - i - 1)];
                }
                clump_entry<U>(A, thr, j, w.c_lo + e, x, free, prev_j);
            }
        }
        __syncthreads();
        prev_j = j;
        prev_free = free;
    }
}

}  // namespace viprs
