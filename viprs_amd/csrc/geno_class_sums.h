// Per-genotype-class column sums over packed PLINK .bed rows (include/viprs_hip.h, viprs_genotypes_class_sums): for SNP j,
// class k (code 0 / 2 / 3) and column c the sum of Y[i][c] over the samples of that class, in the order the header fixes.
//   geno_class_sums_kernel   one wavefront owns R consecutive rows and W columns.  Lane l is slot l of the definition: in
//                            round t it reads word l + 64 t of each of its rows (one coalesced dword load per row, the next
//                            round's words loaded before this round's are used) and the 16 x W values Y[c][t][q][l] -- 64
//                            consecutive doubles per instruction, from the call's device copy of Y in that layout -- each
//                            used for all R rows.  Per (sample, row): two bit tests of the code, three conditions shared by
//                            the W columns; per (sample, row, column): three selects of y or +0 and three double additions.
//                            3 x R x W double accumulators per lane.  After the last round: the xor butterfly over the 64
//                            lanes, d = 32 .. 1 (`__shfl_xor` moves the two halves of a double), and lane 0 stores.
// THE ORDER of the header: inside a lane the samples of its slot ascend (rounds ascending, q ascending inside a word), then the
// butterfly.  Neither depends on R, W, the row range or the launch.  No LDS, no atomics, vector stores, 64-bit offsets.
#pragma once
#include "internal.h"

namespace viprs {

constexpr int kClassSumSlots = VIPRS_CLASS_SUM_SLOTS;   // lanes of a wavefront = slots of the definition
constexpr int kClassSumRows = 4;                        // R: rows a wavefront carries (DESIGN.md 6.8 has the register figures)
constexpr int kClassSumCols = 4;                        // W: columns of the widest instantiation; the rest goes to 2 and 1
constexpr int kClassSumWaves = 4;                       // wavefronts (row groups) of a workgroup
static_assert(kClassSumSlots == 64, "a slot is a lane of a 64-wide wavefront");

struct GenoClassSumsArgs {
    const uint32_t* rows;          // m rows of n_words words
    const double* y;               // [n_cols][n_rounds][16][64]: sample i = 1024 t + 16 l + q; zeros at and beyond n
    double* out;                   // (row1 - row0, 3, n_cols) row-major
    int64_t n_words;               // row stride in 32-bit words (a multiple of 4)
    int64_t n_rounds;              // ceil(n_words / 64)
    int64_t row0, row1;
    int n_cols;
    int col0;                      // first column of this launch's groups (blockIdx.y counts groups of W from it)
};

template <int W>
__global__ __launch_bounds__(kClassSumWaves * 64) void geno_class_sums_kernel(GenoClassSumsArgs A) {
    constexpr int R = kClassSumRows;
    const int lane = threadIdx.x & 63;
    const int64_t j0 = A.row0 + ((int64_t)blockIdx.x * kClassSumWaves + (threadIdx.x >> 6)) * R;
    if (j0 >= A.row1) return;                                   // (wave-uniform: the butterfly below sees whole wavefronts)
    const int col = A.col0 + (int)blockIdx.y * W;               // col + W <= n_cols: the host launches whole groups only
    double acc[R][3][W];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < W; ++c) acc[r][k][c] = 0.0;
    // a row of the group at or beyond row1 is read as the group's first row and never stored
    const uint32_t* row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) row[r] = A.rows + (j0 + r < A.row1 ? j0 + r : j0) * A.n_words;
    constexpr uint32_t kMissing = 0x55555555u;                  // sixteen codes 1: a word the row does not have
    uint32_t next[R];
#pragma unroll
    for (int r = 0; r < R; ++r) next[r] = lane < A.n_words ? row[r][lane] : kMissing;
    for (int64_t t = 0; t < A.n_rounds; ++t) {
        uint32_t w[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = next[r];
        const int64_t ahead = (t + 1) * 64 + lane;
#pragma unroll
        for (int r = 0; r < R; ++r) next[r] = ahead < A.n_words ? row[r][ahead] : kMissing;
        const double* yt = A.y + ((int64_t)col * A.n_rounds + t) * (16 * 64) + lane;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            double y[W];
#pragma unroll
            for (int c = 0; c < W; ++c) y[c] = yt[((int64_t)c * A.n_rounds * 16 + q) * 64];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool b0 = (w[r] >> (2 * q)) & 1u, b1 = (w[r] >> (2 * q + 1)) & 1u;
                const bool is0 = !b0 && !b1, is1 = b1 && !b0, is2 = b1 && b0;   // codes 0, 2, 3
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    acc[r][0][c] = __dadd_rn(acc[r][0][c], is0 ? y[c] : 0.0);
                    acc[r][1][c] = __dadd_rn(acc[r][1][c], is1 ? y[c] : 0.0);
                    acc[r][2][c] = __dadd_rn(acc[r][2][c], is2 ? y[c] : 0.0);
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < W; ++c) acc[r][k][c] = __dadd_rn(acc[r][k][c], __shfl_xor(acc[r][k][c], d, 64));
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (j0 + r >= A.row1) break;
            double* o = A.out + (j0 + r - A.row0) * 3 * (int64_t)A.n_cols + col;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < W; ++c) o[(int64_t)k * A.n_cols + c] = acc[r][k][c];
        }
    }
}

// geno_class_sums.hip: the kernels of rows [A.row0, A.row1) and all A.n_cols columns on `stream`
int launch_geno_class_sums(hipStream_t stream, GenoClassSumsArgs A);

}  // namespace viprs
