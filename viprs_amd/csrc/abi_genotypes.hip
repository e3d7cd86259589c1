// C ABI, genotype scoring (include/viprs_hip.h): packed PLINK .bed rows on the device, the per-SNP code counts and the
// polygenic scores.  Score kernels: geno_score.h; the counts kernel and the kernel that sets the slots beyond n are here.
#include "geno_score.h"

using namespace viprs;

struct viprs_genotypes {
    int64_t n = 0, m = 0;
    int device = 0;
    int64_t file_stride = 0;                       // ceil(n / 4): bytes of a row in the file
    int64_t stride = 0;                            // bytes of a row on the device, a multiple of 16
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> d_rows;                        // m * stride
    DevBuf<int64_t> d_counts;                      // m * 4
    DevBuf<char> d_b, d_dose, d_work, d_scores;
    DevBuf<double> d_sums;
    EventBracket time_score, time_counts;
    ~viprs_genotypes() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

constexpr size_t kWorkBudget = (size_t)64 << 20;   // bytes of partial sums in flight (at least one chunk)
// VIPRS_SCORE_WORK_BYTES: another budget, read at every call (the tests cut a three-chunk problem into three ranges with it)
size_t work_budget() {
    const char* e = std::getenv("VIPRS_SCORE_WORK_BYTES");
    if (!e || !*e) return kWorkBudget;
    const long long v = std::atoll(e);
    return v > 0 ? (size_t)v : kWorkBudget;
}
constexpr int kMaxRangeChunks = 4096;              // chunks of one launch (grid.y)

// Every slot at or beyond n of rows [row0, row0 + n_rows) becomes code 1 (missing): the spare bits of the byte that holds
// sample n - 1 and the padding bytes up to the stride.  One thread per row, at most 16 byte stores.
__global__ __launch_bounds__(256) void geno_tail_kernel(uint8_t* rows, int64_t row0, int64_t n_rows, int64_t n, int64_t stride) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    uint8_t* row = rows + (row0 + r) * stride;
    const int64_t full = n / 4;                    // bytes whose four slots are all samples
    const int rem = (int)(n % 4);
    int64_t at = full;
    if (rem) {
        const uint8_t keep = (uint8_t)((1u << (2 * rem)) - 1u);
        row[at] = (uint8_t)((row[at] & keep) | (0x55u & ~keep));
        ++at;
    }
    for (; at < stride; ++at) row[at] = 0x55u;
}

__device__ __forceinline__ void count_word(uint32_t w, int64_t first_sample, int64_t n, uint32_t (&c)[4]) {
    const int64_t left = n - first_sample;         // samples of this word below n
    if (left <= 0) return;
    const uint32_t valid = left >= 16 ? 0x55555555u : (0x55555555u & ((1u << (2 * (int)left)) - 1u));
    const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;        // the even / odd bit planes
    const uint32_t c1 = __popc(lo & ~hi & valid), c2 = __popc(hi & ~lo & valid), c3 = __popc(lo & hi & valid);
    c[1] += c1; c[2] += c2; c[3] += c3;
    c[0] += __popc(valid) - c1 - c2 - c3;
}

// One wavefront per SNP row, 16-byte loads, an integer xor butterfly over the 64 lanes; lane 0 stores the four counts.
__global__ __launch_bounds__(256) void geno_counts_kernel(const uint8_t* rows, int64_t m, int64_t n, int64_t stride,
                                                          int64_t* counts) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;                            // (wave-uniform)
    const uint4* row = reinterpret_cast<const uint4*>(rows + j * stride);
    const int64_t units = stride / 16;
    uint32_t c[4] = {0u, 0u, 0u, 0u};              // a lane sees n / 64 samples at most: below 2^32
    for (int64_t u = lane; u < units; u += 64) {
        const uint4 v = row[u];
        const int64_t s0 = u * 64;
        count_word(v.x, s0, n, c);
        count_word(v.y, s0 + 16, n, c);
        count_word(v.z, s0 + 32, n, c);
        count_word(v.w, s0 + 48, n, c);
    }
    long long t[4] = {(long long)c[0], (long long)c[1], (long long)c[2], (long long)c[3]};
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] += __shfl_xor(t[k], d, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) counts[j * 4 + k] = (int64_t)t[k];
    }
}

template <typename T>
int score_typed(viprs_genotypes* G, int n_cols, bool with_dose) {
    const int64_t n_words = G->stride / 4;
    const int64_t n_chunks = (G->m + kScoreChunk - 1) / kScoreChunk;
    const size_t per_chunk = (size_t)n_cols * 16 * (size_t)n_words;
    int64_t range = (int64_t)(work_budget() / (per_chunk * sizeof(T)));
    range = std::max<int64_t>(1, std::min<int64_t>({range, n_chunks, (int64_t)kMaxRangeChunks}));
    if (G->d_work.n < (size_t)range * per_chunk * sizeof(T)) HIP_TRY(G->d_work.alloc((size_t)range * per_chunk * sizeof(T)));
    if (G->d_sums.n < per_chunk) HIP_TRY(G->d_sums.alloc(per_chunk));
    GenoScoreArgs<T> S;
    S.rows = reinterpret_cast<const uint32_t*>(G->d_rows.p);
    S.B = reinterpret_cast<const T*>(G->d_b.p);
    S.dose = nullptr;
    S.work = reinterpret_cast<T*>(G->d_work.p);
    S.m = G->m;
    S.n_words = n_words;
    S.n_cols = n_cols;
    S.col0 = 0;
    GenoReduceArgs<T> R;
    R.work = S.work;
    R.sums = G->d_sums.p;
    R.scores = reinterpret_cast<T*>(G->d_scores.p);
    R.n = G->n;
    R.n_words = n_words;
    R.per_chunk = (int64_t)per_chunk;
    R.n_cols = n_cols;
    if (with_dose) S.dose = reinterpret_cast<const T*>(G->d_dose.p);
    int rc = G->time_score.start(G->stream);
    if (rc != VIPRS_OK) return rc;
    // ranges of chunks in turn: the work buffer holds one range, the double sums carry on from range to range
    for (int64_t k0 = 0; k0 < n_chunks; k0 += range) {
        S.chunk0 = k0;
        R.n_chunks = (int)std::min<int64_t>(range, n_chunks - k0);
        R.first = k0 == 0;
        R.last = k0 + range >= n_chunks;
        rc = launch_geno_score<T>(G->stream, S, R);
        if (rc != VIPRS_OK) return rc;
    }
    return G->time_score.stop(G->stream);
}

}  // namespace
}  // namespace viprs

extern "C" {

int viprs_genotypes_create(viprs_genotypes** out, int64_t n_samples, int64_t m, int device) {
    if (!out) return fail(VIPRS_EINVAL, "null handle pointer");
    if (n_samples < 0 || m < 0) return fail(VIPRS_EINVAL, "n_samples and m must not be negative");
    if (n_samples >= ((int64_t)1 << 31) - 16) return fail(VIPRS_EINVAL, "n_samples must be below 2^31 - 16");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(VIPRS_EINVAL, "no such device");
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<viprs_genotypes> G(new viprs_genotypes);
    G->n = n_samples;
    G->m = m;
    G->device = device;
    G->file_stride = (n_samples + 3) / 4;
    G->stride = (G->file_stride + 15) / 16 * 16;
    HIP_TRY(hipStreamCreateWithFlags(&G->stream, hipStreamNonBlocking));
    const size_t bytes = (size_t)m * (size_t)G->stride;
    if (bytes) {
        if (G->d_rows.alloc(bytes) != hipSuccess) return fail(VIPRS_ENOMEM, "no device memory for the genotype rows");
        HIP_TRY(hipMemsetAsync(G->d_rows.p, 0x55, bytes, G->stream));       // every sample missing until its row arrives
        HIP_TRY(hipStreamSynchronize(G->stream));
    }
    *out = G.release();
    return VIPRS_OK;
}

int viprs_genotypes_destroy(viprs_genotypes* G) {
    if (!G) return VIPRS_OK;
    (void)hipSetDevice(G->device);
    delete G;
    return VIPRS_OK;
}

int viprs_genotypes_upload_rows(viprs_genotypes* G, int64_t first_row, int64_t n_rows, const uint8_t* bed_rows) {
    if (!G) return fail(VIPRS_EINVAL, "null genotypes");
    if (first_row < 0 || n_rows < 0 || first_row > G->m || n_rows > G->m - first_row)
        return fail(VIPRS_EINVAL, "rows out of range");
    if (n_rows == 0 || G->n == 0) return VIPRS_OK;
    if (!bed_rows) return fail(VIPRS_EINVAL, "null host buffer");
    HIP_TRY(hipSetDevice(G->device));
    uint8_t* dst = G->d_rows.p + (size_t)first_row * (size_t)G->stride;
    if (G->stride == G->file_stride)
        HIP_TRY(hipMemcpyAsync(dst, bed_rows, (size_t)n_rows * (size_t)G->stride, hipMemcpyHostToDevice, G->stream));
    else
        HIP_TRY(hipMemcpy2DAsync(dst, (size_t)G->stride, bed_rows, (size_t)G->file_stride, (size_t)G->file_stride,
                                 (size_t)n_rows, hipMemcpyHostToDevice, G->stream));
    if (G->n % 4 != 0 || G->stride != G->file_stride) {
        geno_tail_kernel<<<dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, G->stream>>>(G->d_rows.p, first_row, n_rows,
                                                                                             G->n, G->stride);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(G->stream));
    return VIPRS_OK;
}

int viprs_genotypes_counts(viprs_genotypes* G, int64_t* counts) {
    if (!G) return fail(VIPRS_EINVAL, "null genotypes");
    if (!counts) return fail(VIPRS_EINVAL, "null host buffer");
    if (G->m == 0) return VIPRS_OK;
    const size_t bytes = (size_t)G->m * 4 * sizeof(int64_t);
    if (G->n == 0) {
        std::memset(counts, 0, bytes);
        return VIPRS_OK;
    }
    HIP_TRY(hipSetDevice(G->device));
    if (G->d_counts.n < (size_t)G->m * 4) HIP_TRY(G->d_counts.alloc((size_t)G->m * 4));
    int rc = G->time_counts.start(G->stream);
    if (rc != VIPRS_OK) return rc;
    geno_counts_kernel<<<dim3((unsigned)((G->m + 3) / 4)), dim3(256), 0, G->stream>>>(G->d_rows.p, G->m, G->n, G->stride,
                                                                                     G->d_counts.p);
    HIP_TRY(hipGetLastError());
    rc = G->time_counts.stop(G->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(counts, G->d_counts.p, bytes, hipMemcpyDeviceToHost, G->stream));
    HIP_TRY(hipStreamSynchronize(G->stream));
    return VIPRS_OK;
}

int viprs_genotypes_score(viprs_genotypes* G, int float_dtype, int n_cols, const void* b_host, const void* dose_host,
                          void* scores_host) {
    const size_t ts = float_size(float_dtype);
    if (ts == 0) return fail(VIPRS_EINVAL, "bad float dtype code");
    if (n_cols < 1) return fail(VIPRS_EINVAL, "n_cols must be at least 1");
    if (!G) return fail(VIPRS_EINVAL, "null genotypes");
    if (!b_host && G->m > 0) return fail(VIPRS_EINVAL, "null effect-size buffer");
    if (!scores_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (G->n == 0) return VIPRS_OK;
    const size_t out_bytes = (size_t)G->n * (size_t)n_cols * ts;
    if (G->m == 0) {
        std::memset(scores_host, 0, out_bytes);
        return VIPRS_OK;
    }
    HIP_TRY(hipSetDevice(G->device));
    const size_t b_bytes = (size_t)G->m * (size_t)n_cols * ts, d_bytes = (size_t)G->m * 4 * ts;
    if (G->d_b.n < b_bytes) HIP_TRY(G->d_b.alloc(b_bytes));
    if (dose_host && G->d_dose.n < d_bytes) HIP_TRY(G->d_dose.alloc(d_bytes));
    if (G->d_scores.n < out_bytes) HIP_TRY(G->d_scores.alloc(out_bytes));
    HIP_TRY(hipMemcpyAsync(G->d_b.p, b_host, b_bytes, hipMemcpyHostToDevice, G->stream));
    if (dose_host) HIP_TRY(hipMemcpyAsync(G->d_dose.p, dose_host, d_bytes, hipMemcpyHostToDevice, G->stream));
    int rc = float_dtype == VIPRS_F32 ? score_typed<float>(G, n_cols, dose_host != nullptr)
                                      : score_typed<double>(G, n_cols, dose_host != nullptr);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(scores_host, G->d_scores.p, out_bytes, hipMemcpyDeviceToHost, G->stream));
    HIP_TRY(hipStreamSynchronize(G->stream));
    return VIPRS_OK;
}

int viprs_genotypes_last_counts_ms(viprs_genotypes* G, double* ms) {
    if (!G || !ms) return fail(VIPRS_EINVAL, "null argument");
    return G->time_counts.elapsed(G->device, ms, "no timed counts call yet");
}

int viprs_genotypes_last_score_ms(viprs_genotypes* G, double* ms) {
    if (!G || !ms) return fail(VIPRS_EINVAL, "null argument");
    return G->time_score.elapsed(G->device, ms, "no timed score call yet");
}

}  // extern "C"
