// Polygenic scores from packed PLINK .bed rows (include/viprs_hip.h, viprs_genotypes_score).  Two kernels:
//   geno_score_kernel   grid (sample tile) x (SNP chunk) x (column group).  A lane owns the 16 samples of one 32-bit word of
//                       the row and carries W columns x 16 samples of partial sums in registers; the word loads are coalesced
//                       along the row, D[j][0..3] and B[j][c..c+W) have wave-uniform addresses (scalar loads).  Per sample: one
//                       bit-field extract, one dose select shared by the W columns, one multiply and one add per column.  The
//                       partial sums of the chunk go to the work buffer
//   geno_reduce_kernel  adds the partial sums of a range of chunks to the double sums, chunks ascending, and -- after the last
//                       range -- rounds them to T into the (n, n_cols) row-major result
// THE ORDER of the header: SNPs ascending inside a chunk in T, chunks ascending in double.  Neither depends on W, on the tile
// or on the ranges the host cuts the chunks into (the double sum continues where the previous range stopped).
// Work buffer and double sums share one layout: [chunk of the range][column][sample % 16][word], so that the 64 lanes of a
// wavefront store (and the reduction reads) 256 contiguous bytes per instruction.  No LDS, no atomics.
#pragma once
#include "internal.h"

namespace viprs {

constexpr int kScoreChunk = VIPRS_SCORE_CHUNK;     // L of the definition
constexpr int kScoreTileWords = 64;                // one wavefront per workgroup: a tile is 64 words = 1024 samples
constexpr int kScoreSnpsAhead = 4;                 // row words loaded before the first of them is used

template <typename T> struct GenoScoreArgs {
    const uint32_t* rows;          // m rows of n_words words
    const T* B;                    // (m, n_cols) row-major
    const T* dose;                 // (m, 4) or null: {2, 0, 1, 0}
    T* work;                       // [n_chunks of the range][n_cols][16][n_words]
    int64_t m;
    int64_t n_words;               // row stride in 32-bit words (a multiple of 4)
    int64_t chunk0;                // first chunk of the range (blockIdx.y counts from it)
    int n_cols;
    int col0;                      // first column of this launch's groups (blockIdx.z counts groups of W from it)
};

template <typename T> __device__ __forceinline__ T score_mul(T a, T b);
template <> __device__ __forceinline__ float score_mul<float>(float a, float b) { return __fmul_rn(a, b); }
template <> __device__ __forceinline__ double score_mul<double>(double a, double b) { return __dmul_rn(a, b); }
template <typename T> __device__ __forceinline__ T score_add(T a, T b);
template <> __device__ __forceinline__ float score_add<float>(float a, float b) { return __fadd_rn(a, b); }
template <> __device__ __forceinline__ double score_add<double>(double a, double b) { return __dadd_rn(a, b); }

// one SNP: the 16 samples of `w` into acc.  The four doses are scalars (wave-uniform values in SGPRs), chosen by two
// selects on the code's bits: nothing here is an indexed array
template <typename T, int W>
__device__ __forceinline__ void score_snp(T (&acc)[16][W], uint32_t w, T d0, T d1, T d2, T d3, const T (&b)[W]) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const bool bit0 = (w >> (2 * s)) & 1u, bit1 = (w >> (2 * s + 1)) & 1u;
        const T lo = bit0 ? d1 : d0;
        const T hi = bit0 ? d3 : d2;
        const T dose = bit1 ? hi : lo;
#pragma unroll
        for (int c = 0; c < W; ++c) acc[s][c] = score_add<T>(acc[s][c], score_mul<T>(b[c], dose));
    }
}

// SNP j of the launch's column group.  DOSE: the caller's table; otherwise the constants {2, 0, 1, 0} (no table is read)
template <typename T, int W, bool DOSE>
__device__ __forceinline__ void score_one(const GenoScoreArgs<T>& A, T (&acc)[16][W], int64_t j, int col, uint32_t w) {
    T b[W];
#pragma unroll
    for (int c = 0; c < W; ++c) b[c] = A.B[j * A.n_cols + col + c];
    if constexpr (DOSE) {
        const T* d = A.dose + j * 4;
        score_snp<T, W>(acc, w, d[0], d[1], d[2], d[3], b);
    } else {
        score_snp<T, W>(acc, w, (T)2, (T)0, (T)1, (T)0, b);
    }
}

template <typename T, int W, bool DOSE>
__global__ __launch_bounds__(64) void geno_score_kernel(GenoScoreArgs<T> A) {
    const int64_t word = (int64_t)blockIdx.x * kScoreTileWords + threadIdx.x;
    if (word >= A.n_words) return;                              // (no cross-lane operation below)
    const int64_t chunk = A.chunk0 + blockIdx.y;
    const int col = A.col0 + (int)blockIdx.z * W;               // col + W <= n_cols: the host launches whole groups only
    const int64_t j0 = chunk * kScoreChunk;
    const int64_t j1 = j0 + kScoreChunk < A.m ? j0 + kScoreChunk : A.m;
    T acc[16][W];
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int c = 0; c < W; ++c) acc[s][c] = (T)0;
    const uint32_t* row = A.rows + word;                        // + j * n_words: 64-bit
    int64_t j = j0;
    for (; j + kScoreSnpsAhead <= j1; j += kScoreSnpsAhead) {
        uint32_t w[kScoreSnpsAhead];
#pragma unroll
        for (int u = 0; u < kScoreSnpsAhead; ++u) w[u] = row[(j + u) * A.n_words];
#pragma unroll
        for (int u = 0; u < kScoreSnpsAhead; ++u) score_one<T, W, DOSE>(A, acc, j + u, col, w[u]);
    }
    for (; j < j1; ++j) score_one<T, W, DOSE>(A, acc, j, col, row[j * A.n_words]);
    T* out = A.work + (((int64_t)blockIdx.y * A.n_cols + col) * 16) * A.n_words + word;
#pragma unroll
    for (int c = 0; c < W; ++c)
#pragma unroll
        for (int s = 0; s < 16; ++s) out[((int64_t)c * 16 + s) * A.n_words] = acc[s][c];
}

template <typename T> struct GenoReduceArgs {
    const T* work;                 // [n_chunks][n_cols][16][n_words]
    double* sums;                  // [n_cols][16][n_words]
    T* scores;                     // (n, n_cols) row-major, written when `last`
    int64_t n;
    int64_t n_words;
    int64_t per_chunk;             // n_cols * 16 * n_words
    int n_chunks;                  // of this range
    int n_cols;
    int first, last;               // the first range starts the sums at 0; the last one writes the scores
};

template <typename T>
__global__ __launch_bounds__(256) void geno_reduce_kernel(GenoReduceArgs<T> A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (column, sample % 16, word)
    if (e >= A.per_chunk) return;
    double s = A.first ? 0.0 : A.sums[e];
    // (unrolled so that eight loads are in flight; the additions stay in chunk order)
#pragma unroll 8
    for (int k = 0; k < A.n_chunks; ++k) s = __dadd_rn(s, (double)A.work[(int64_t)k * A.per_chunk + e]);
    A.sums[e] = s;
    if (A.last) {
        const int64_t word = e % A.n_words;
        const int64_t cs = e / A.n_words;
        const int64_t i = word * 16 + (cs % 16);
        if (i < A.n) A.scores[i * A.n_cols + cs / 16] = (T)s;
    }
}

// geno_score_f32.hip / geno_score_f64.hip: the kernels of one range of chunks and its reduction on `stream`
template <typename T>
int launch_geno_score(hipStream_t stream, GenoScoreArgs<T> S, GenoReduceArgs<T> R);

// columns a lane carries: 16 samples x W accumulators of T in registers (DESIGN.md 6.6 has the register figures)
template <typename T> constexpr int score_group_width() { return sizeof(T) == 4 ? 8 : 4; }

// groups of W columns from S.col0 on, as many as fit below n_cols; the rest goes to the narrower instantiations
template <typename T, int W>
int launch_geno_groups(hipStream_t stream, GenoScoreArgs<T>& S, int n_chunks) {
    const int groups = (S.n_cols - S.col0) / W;
    if (groups > 0) {
        const dim3 grid((unsigned)((S.n_words + kScoreTileWords - 1) / kScoreTileWords), (unsigned)n_chunks, (unsigned)groups);
        if (S.dose) geno_score_kernel<T, W, true><<<grid, dim3(kScoreTileWords), 0, stream>>>(S);
        else geno_score_kernel<T, W, false><<<grid, dim3(kScoreTileWords), 0, stream>>>(S);
        HIP_TRY(hipGetLastError());
        S.col0 += groups * W;
    }
    if constexpr (W > 1) return launch_geno_groups<T, W / 2>(stream, S, n_chunks);
    return VIPRS_OK;
}

template <typename T>
int launch_geno_score_impl(hipStream_t stream, GenoScoreArgs<T> S, GenoReduceArgs<T> R) {
    S.col0 = 0;
    int rc = launch_geno_groups<T, score_group_width<T>()>(stream, S, R.n_chunks);
    if (rc != VIPRS_OK) return rc;
    geno_reduce_kernel<T><<<dim3((unsigned)((R.per_chunk + 255) / 256)), dim3(256), 0, stream>>>(R);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

}  // namespace viprs
