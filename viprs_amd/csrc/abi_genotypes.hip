// C ABI, genotype scoring (include/viprs_hip.h): packed PLINK .bed rows on the device, the per-SNP code counts and the
// polygenic scores, and the LD matrix of the rows in the compact upper store.  Score kernels: geno_score.h; LD kernels:
// geno_ld.h; per-genotype-class column sums: geno_class_sums.h; the counts kernel and the kernel that sets the slots beyond n
// are here.
#include "geno_class_sums.h"
#include "geno_ld.h"
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
    bool counts_on_device = false;                 // d_counts holds the counts of the rows as they are now
    // LD (viprs_genotypes_ld): nn, a and the tiles free of missing codes follow from the counts, once per upload
    bool ld_tables_built = false;
    std::vector<uint8_t> tile_clean;               // per tile of kLdTile SNPs
    DevBuf<int64_t> d_nn, d_a, d_right_end, d_indptr, d_pairs;
    DevBuf<double> d_w;
    DevBuf<char> d_ld_out;
    EventBracket time_ld;
    DevBuf<double> d_class_y, d_class_out;         // class sums: the call's Y in the kernel's layout, the rows of its output
    EventBracket time_class_sums;
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

// nn_j, a_j and the clean tiles of the LD kernels, from the device counts: those of the caller's last counts call when the
// rows have not changed since, otherwise the counts kernel runs here (the caller's timing of it is not touched)
int ensure_ld_tables(viprs_genotypes* G) {
    if (G->ld_tables_built || G->m == 0) return VIPRS_OK;
    const size_t m = (size_t)G->m;
    std::vector<int64_t> c(m * 4, 0);
    if (G->n > 0) {
        if (!G->counts_on_device) {
            HIP_TRY(G->d_counts.reserve(m * 4));
            geno_counts_kernel<<<dim3((unsigned)((G->m + 3) / 4)), dim3(256), 0, G->stream>>>(G->d_rows.p, G->m, G->n,
                                                                                             G->stride, G->d_counts.p);
            HIP_TRY(hipGetLastError());
            G->counts_on_device = true;
        }
        HIP_TRY(hipMemcpyAsync(c.data(), G->d_counts.p, m * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, G->stream));
        HIP_TRY(hipStreamSynchronize(G->stream));
    }
    std::vector<int64_t> nn(m), a(m);
    std::vector<uint8_t> clean((m + kLdTile - 1) / kLdTile, 1);
    for (size_t j = 0; j < m; ++j) {
        nn[j] = c[j * 4] + c[j * 4 + 2] + c[j * 4 + 3];
        a[j] = 2 * c[j * 4] + c[j * 4 + 2];
        if (c[j * 4 + 1] != 0) clean[j / kLdTile] = 0;
    }
    HIP_TRY(G->d_nn.reserve(m));
    HIP_TRY(G->d_a.reserve(m));
    HIP_TRY(hipMemcpyAsync(G->d_nn.p, nn.data(), m * sizeof(int64_t), hipMemcpyHostToDevice, G->stream));
    HIP_TRY(hipMemcpyAsync(G->d_a.p, a.data(), m * sizeof(int64_t), hipMemcpyHostToDevice, G->stream));
    HIP_TRY(hipStreamSynchronize(G->stream));
    G->tile_clean.swap(clean);
    G->ld_tables_built = true;
    return VIPRS_OK;
}

// Everything `viprs_genotypes_ld` puts on the stream: the uploads of the call's tables, the kernels between the LD event pair,
// the download.  Nothing is synchronised here: the caller drains the stream whatever this returns, because the uploads read
// pageable host memory of the caller's frame
int enqueue_ld(viprs_genotypes* G, int64_t row0, int64_t row1, const int64_t* right_end, const double* w, int out_dtype,
               const std::vector<int64_t>& indptr, const std::vector<int64_t>& pairs, size_t n_clean, void* data_host) {
    const size_t m = (size_t)G->m;
    const size_t out_bytes = (size_t)(indptr[(size_t)row1] - indptr[(size_t)row0]) * ld_elem_size(out_dtype);
    HIP_TRY(hipMemcpyAsync(G->d_right_end.p, right_end, m * sizeof(int64_t), hipMemcpyHostToDevice, G->stream));
    HIP_TRY(hipMemcpyAsync(G->d_indptr.p, indptr.data(), (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, G->stream));
    HIP_TRY(hipMemcpyAsync(G->d_w.p, w, m * sizeof(double), hipMemcpyHostToDevice, G->stream));
    HIP_TRY(hipMemcpyAsync(G->d_pairs.p, pairs.data(), pairs.size() * sizeof(int64_t), hipMemcpyHostToDevice, G->stream));
    GenoLdArgs A;
    A.rows = G->d_rows.p;
    A.right_end = G->d_right_end.p;
    A.indptr = G->d_indptr.p;
    A.nn = G->d_nn.p;
    A.a = G->d_a.p;
    A.w = G->d_w.p;
    A.pairs = nullptr;
    A.out = G->d_ld_out.p;
    A.m = G->m;
    A.n = G->n;
    A.stride = G->stride;
    A.row0 = row0;
    A.row1 = row1;
    int rc = G->time_ld.start(G->stream);
    if (rc != VIPRS_OK) return rc;
    rc = launch_geno_ld(G->stream, out_dtype, A, G->d_pairs.p, (int64_t)n_clean, G->d_pairs.p + n_clean,
                        (int64_t)(pairs.size() - n_clean));
    if (rc != VIPRS_OK) return rc;
    rc = G->time_ld.stop(G->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(data_host, G->d_ld_out.p, out_bytes, hipMemcpyDeviceToHost, G->stream));
    return VIPRS_OK;
}

// Everything `viprs_genotypes_class_sums` puts on the stream: the upload of Y in the kernel's layout, the kernels between the
// event pair, the download.  Nothing is synchronised here: the caller drains the stream whatever this returns, because the
// upload reads `y_dev_layout` of the caller's frame
int enqueue_class_sums(viprs_genotypes* G, int64_t row0, int64_t row1, int n_cols, const std::vector<double>& y_dev_layout,
                       int64_t n_rounds, double* sums_host) {
    const size_t out_count = (size_t)(row1 - row0) * 3 * (size_t)n_cols;
    HIP_TRY(hipMemcpyAsync(G->d_class_y.p, y_dev_layout.data(), y_dev_layout.size() * sizeof(double), hipMemcpyHostToDevice,
                           G->stream));
    GenoClassSumsArgs A;
    A.rows = reinterpret_cast<const uint32_t*>(G->d_rows.p);
    A.y = G->d_class_y.p;
    A.out = G->d_class_out.p;
    A.n_words = G->stride / 4;
    A.n_rounds = n_rounds;
    A.row0 = row0;
    A.row1 = row1;
    A.n_cols = n_cols;
    A.col0 = 0;
    int rc = G->time_class_sums.start(G->stream);
    if (rc != VIPRS_OK) return rc;
    rc = launch_geno_class_sums(G->stream, A);
    if (rc != VIPRS_OK) return rc;
    rc = G->time_class_sums.stop(G->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(sums_host, G->d_class_out.p, out_count * sizeof(double), hipMemcpyDeviceToHost, G->stream));
    return VIPRS_OK;
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
    G->counts_on_device = false;                   // (counts and LD tables follow the rows: rebuilt by the next call)
    G->ld_tables_built = false;
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
    G->counts_on_device = true;
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

int viprs_genotypes_ld(viprs_genotypes* G, int64_t row0, int64_t row1, const int64_t* right_end, const double* w, int out_dtype,
                       void* data_host) {
    // every argument check comes before any device work
    if (out_dtype != VIPRS_LD_I8 && out_dtype != VIPRS_LD_I16 && out_dtype != VIPRS_LD_F32 && out_dtype != VIPRS_LD_F64)
        return fail(VIPRS_EINVAL, "bad LD output dtype code: int8, int16, float32 or float64");
    if (row0 > row1) return fail(VIPRS_EINVAL, "row0 must not exceed row1");
    if (!right_end) return fail(VIPRS_EINVAL, "null right_end");
    if (!w) return fail(VIPRS_EINVAL, "null w");
    if (!data_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (!G) return fail(VIPRS_EINVAL, "null genotypes");
    if (G->n > kLdMaxSamples)
        return fail(VIPRS_EINVAL, "n_samples must not exceed 2^19 = 524288: beyond it the numerator leaves int64");
    if (row0 < 0 || row1 > G->m) return fail(VIPRS_EINVAL, "rows out of range");
    for (int64_t j = 0; j < G->m; ++j) {
        if (right_end[j] < j + 1 || right_end[j] > G->m) return fail(VIPRS_EINVAL, "right_end[j] must lie in [j + 1, m]");
        if (j > 0 && right_end[j] < right_end[j - 1]) return fail(VIPRS_EINVAL, "right_end must be non-decreasing");
    }
    if (row0 == row1) return VIPRS_OK;
    const size_t m = (size_t)G->m;
    std::vector<int64_t> indptr(m + 1, 0);
    for (size_t j = 0; j < m; ++j) indptr[j + 1] = indptr[j] + (right_end[j] - (int64_t)j - 1);
    const int64_t n_out = indptr[(size_t)row1] - indptr[(size_t)row0];
    if (n_out == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(G->device));
    int rc = ensure_ld_tables(G);
    if (rc != VIPRS_OK) return rc;
    // tile pairs (I, J), J >= I, that meet the window of rows [row0, row1); right_end is monotone, so the last row of the
    // tile inside the range reaches furthest.  Clean pairs first, then the general ones
    std::vector<int64_t> pairs_clean, pairs_general;
    for (int64_t I = row0 / kLdTile; I * kLdTile < row1; ++I) {
        const int64_t last = std::min<int64_t>((I + 1) * kLdTile, row1) - 1;
        const int64_t J1 = (right_end[last] - 1) / kLdTile;
        for (int64_t J = I; J <= J1; ++J)
            (G->tile_clean[(size_t)I] && G->tile_clean[(size_t)J] ? pairs_clean : pairs_general).push_back((I << 32) | J);
    }
    const size_t n_clean = pairs_clean.size();
    pairs_clean.insert(pairs_clean.end(), pairs_general.begin(), pairs_general.end());
    const size_t out_bytes = (size_t)n_out * ld_elem_size(out_dtype);
    // (a failed allocation leaves its buffer empty, dev_buf.h: the next call allocates again)
    HIP_TRY(G->d_right_end.reserve(m));
    HIP_TRY(G->d_indptr.reserve(m + 1));
    HIP_TRY(G->d_w.reserve(m));
    HIP_TRY(G->d_pairs.reserve(pairs_clean.size()));
    if (G->d_ld_out.reserve(out_bytes) != hipSuccess)
        return fail(VIPRS_ENOMEM, "no device memory for the rows of the LD store: give a smaller row range");
    rc = enqueue_ld(G, row0, row1, right_end, w, out_dtype, indptr, pairs_clean, n_clean, data_host);
    // on the error paths too: the uploads read `indptr`, `pairs_clean` and the caller's arrays until the stream is drained
    const hipError_t drained = hipStreamSynchronize(G->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(drained);
    return VIPRS_OK;
}

int viprs_genotypes_class_sums(viprs_genotypes* G, int64_t row0, int64_t row1, int n_cols, const double* y_host,
                               double* sums_host) {
    // every argument check comes before the object is touched
    if (n_cols < 1) return fail(VIPRS_EINVAL, "n_cols must be at least 1");
    if (row0 > row1) return fail(VIPRS_EINVAL, "row0 must not exceed row1");
    if (!y_host) return fail(VIPRS_EINVAL, "null Y");
    if (!sums_host) return fail(VIPRS_EINVAL, "null host buffer");
    if (!G) return fail(VIPRS_EINVAL, "null genotypes");
    if (row0 < 0 || row1 > G->m) return fail(VIPRS_EINVAL, "rows out of range");
    if (row0 == row1) return VIPRS_OK;
    const size_t out_count = (size_t)(row1 - row0) * 3 * (size_t)n_cols;
    if (G->n == 0) {
        std::memset(sums_host, 0, out_count * sizeof(double));
        return VIPRS_OK;
    }
    // Y as the kernel reads it: [column][round t][sample-in-word q][lane l], sample i = 1024 t + 16 l + q; zeros beyond n
    const int64_t n_words = G->stride / 4;
    const int64_t n_rounds = (n_words + kClassSumSlots - 1) / kClassSumSlots;
    std::vector<double> y((size_t)n_cols * (size_t)n_rounds * 1024, 0.0);
    for (int64_t i = 0; i < G->n; ++i) {
        const size_t at = (size_t)(i >> 10) * 1024 + (size_t)(i & 15) * 64 + (size_t)((i >> 4) & 63);
        for (int c = 0; c < n_cols; ++c) y[(size_t)c * (size_t)n_rounds * 1024 + at] = y_host[(size_t)i * (size_t)n_cols + c];
    }
    HIP_TRY(hipSetDevice(G->device));
    // (a failed allocation leaves its buffer empty, dev_buf.h: the next call allocates again)
    if (G->d_class_y.reserve(y.size()) != hipSuccess) return fail(VIPRS_ENOMEM, "no device memory for Y");
    if (G->d_class_out.reserve(out_count) != hipSuccess)
        return fail(VIPRS_ENOMEM, "no device memory for the class sums: give a smaller row range");
    const int rc = enqueue_class_sums(G, row0, row1, n_cols, y, n_rounds, sums_host);
    // on the error paths too: the upload reads `y` until the stream is drained
    const hipError_t drained = hipStreamSynchronize(G->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(drained);
    return VIPRS_OK;
}

int viprs_genotypes_last_class_sums_ms(viprs_genotypes* G, double* ms) {
    if (!G || !ms) return fail(VIPRS_EINVAL, "null argument");
    return G->time_class_sums.elapsed(G->device, ms, "no timed class-sums call yet");
}

int viprs_genotypes_last_ld_ms(viprs_genotypes* G, double* ms) {
    if (!G || !ms) return fail(VIPRS_EINVAL, "null argument");
    return G->time_ld.elapsed(G->device, ms, "no timed LD call yet");
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
