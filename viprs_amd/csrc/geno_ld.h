// LD from packed PLINK .bed rows on the int8 matrix cores (include/viprs_hip.h, viprs_genotypes_ld).
//
// A work item is a pair (I, J), J >= I, of tiles of kLdTile = 64 SNPs that meets the window of the call's rows; the host
// builds the list from right_end.  The K loop runs over the samples.  A 32-bit word of a row is the 16 consecutive samples
// of one SNP, which is one lane's 16-element int8 fragment of v_mfma_i32_32x32x32_i8: lane l takes its words from SNP
// (tile start + (l & 31)) and from the 16-byte unit (l >> 5) of every 32 bytes of the row, so one 16-byte load feeds four
// k-steps.  The A fragment (tile I) and the B fragment (tile J) are built by the same code from the same words, hence every
// sample meets itself whatever k the hardware gives an element: integer sums do not depend on the order.
//   decode   2-bit codes -> the int8 planes x (dose 2 / 0 / 1 / 0 for the codes 0 / 1 / 2 / 3) and p (1 / 0 / 1 / 1) with
//            shifts, masks and one byte-wise add.  No table, no array indexed by the code, no LDS: each wave decodes its own
//   general  geno_ld_kernel<O, false>: four waves, each a 32 x 32 quarter of the tile pair with the four sums
//            S = x x', U_ij = x p', U_ji = p x', N = p p' (4 x 16 accumulator registers)
//   clean    geno_ld_kernel<O, true>: both tiles free of missing codes.  Only S is accumulated; U_ij = a_i, U_ji = a_j, N = n.
//            One wave carries the whole 64 x 64 pair (again 4 x 16 accumulator registers), so that a decoded fragment is
//            used by two products
// TAIL SAMPLES: every slot at or beyond n of a device row reads as code 1 (geno_tail_kernel: the spare bits of the last byte
// and the padding up to the 16-byte stride), and the unit beyond an odd number of units is replaced by 0x55 bytes here.  Code 1
// has x = 0 and p = 0 and adds nothing to any of the four sums: there is no mask at n.
// Epilogue: int32 sums -> num in int64 -> double -> O, one division, stored straight to the row's place in the compact upper
// store.  C/D map of the 32 x 32 forms: column = lane & 31 (the B fragment's SNP), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
// (the A fragment's SNP), so the 32 lanes of a half store 32 consecutive elements of one row.  The diagonal, the sub-diagonal
// half, entries at or beyond right_end and rows outside [row0, row1) are not written.  No atomics; every offset is 64-bit.
#pragma once
#include "internal.h"

namespace viprs {

constexpr int kLdTile = 64;                        // SNPs of a tile: two fragments of 32
constexpr int64_t kLdMaxSamples = (int64_t)1 << 19; // 4 n^3 4 < 2^63

struct GenoLdArgs {
    const uint8_t* rows;           // m rows of `stride` bytes
    const int64_t* right_end;      // m
    const int64_t* indptr;         // m + 1: indptr[j + 1] - indptr[j] = right_end[j] - j - 1
    const int64_t* nn;             // m: non-missing samples
    const int64_t* a;              // m: sum of the doses
    const double* w;               // m: sqrt(nn d), built on the host
    const int64_t* pairs;          // work list: I << 32 | J
    void* out;                     // rows [row0, row1) of the store: element indptr[row0] is element 0
    int64_t m, n, stride;
    int64_t row0, row1;
};

typedef int ld_frag __attribute__((ext_vector_type(4)));
typedef int ld_acc __attribute__((ext_vector_type(16)));

// the four 2-bit codes of byte q of `w`, one per byte
__device__ __forceinline__ uint32_t ld_spread(uint32_t w, int q) {
    const uint32_t b = (w >> (8 * q)) & 0xffu;
    const uint32_t t = (b | (b << 12)) & 0x000f000fu;
    return (t | (t << 6)) & 0x03030303u;
}

// code (hi, lo) = 00 -> x 2, p 1;  01 (missing) -> 0, 0;  10 -> 1, 1;  11 -> 0, 1
template <bool WITH_P>
__device__ __forceinline__ void ld_decode(uint32_t w, ld_frag& x, ld_frag& p) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t c = ld_spread(w, q);
        const uint32_t hi = (c >> 1) & 0x01010101u, nlo = ~c & 0x01010101u;
        x[q] = (int)(nlo + (nlo & ~hi));           // byte-wise: at most 2, no carry
        if constexpr (WITH_P) p[q] = (int)(hi | nlo);
    }
}

__device__ __forceinline__ uint32_t ld_word(const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// 16-byte unit u of the lane's row; beyond the row: every code missing
__device__ __forceinline__ uint4 ld_unit(const uint4* row, int64_t u, int64_t units) {
    return u < units ? row[u] : make_uint4(0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u);
}

template <typename O> __device__ __forceinline__ O ld_round(double r);
template <> __device__ __forceinline__ double ld_round<double>(double r) { return r; }
template <> __device__ __forceinline__ float ld_round<float>(double r) { return (float)r; }
template <> __device__ __forceinline__ int8_t ld_round<int8_t>(double r) {
    const double v = rint(__dmul_rn(r, 127.0));
    return (int8_t)(v > 127.0 ? 127.0 : (v < -127.0 ? -127.0 : v));
}
template <> __device__ __forceinline__ int16_t ld_round<int16_t>(double r) {
    const double v = rint(__dmul_rn(r, 32767.0));
    return (int16_t)(v > 32767.0 ? 32767.0 : (v < -32767.0 ? -32767.0 : v));
}

// the 32 x 32 quarter whose A fragment starts at SNP i0 and whose B fragment starts at SNP j0
template <typename O, bool CLEAN>
__device__ __forceinline__ void ld_store_quarter(const GenoLdArgs& A, int64_t i0, int64_t j0, int lane, const ld_acc& S,
                                                 const ld_acc& Uij, const ld_acc& Uji, const ld_acc& N) {
    const int64_t j = j0 + (lane & 31);
    if (j >= A.m) return;                          // (no cross-lane operation below)
    const int64_t nn_j = A.nn[j], a_j = A.a[j];
    const double w_j = A.w[j];
    O* out = reinterpret_cast<O*>(A.out);
    const int64_t base = A.indptr[A.row0];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int64_t i = i0 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        if (i < A.row0 || i >= A.row1 || j <= i) continue;
        if (j >= A.right_end[i]) continue;
        const int64_t nn_i = A.nn[i], a_i = A.a[i];
        const double w_i = A.w[i];
        const int64_t s = (int64_t)S[reg];
        const int64_t u_ij = CLEAN ? a_i : (int64_t)Uij[reg];
        const int64_t u_ji = CLEAN ? a_j : (int64_t)Uji[reg];
        const int64_t nb = CLEAN ? A.n : (int64_t)N[reg];
        const int64_t num = nn_i * nn_j * s - nn_i * a_j * u_ij - nn_j * a_i * u_ji + a_i * a_j * nb;
        const double r = (w_i == 0.0 || w_j == 0.0) ? 0.0 : __ddiv_rn((double)num, __dmul_rn(w_i, w_j));
        out[(A.indptr[i] - base) + (j - i - 1)] = ld_round<O>(r);
    }
}

// does the quarter (i0, j0) hold an entry of the call?  Wave-uniform.  right_end is non-decreasing: the last row decides
__device__ __forceinline__ bool ld_quarter_live(const GenoLdArgs& A, int64_t i0, int64_t j0) {
    const int64_t first = i0 > A.row0 ? i0 : A.row0;
    const int64_t last = (i0 + 32 < A.row1 ? i0 + 32 : A.row1) - 1;
    if (last < first) return false;
    if (j0 + 31 <= first) return false;            // diagonal and below only
    return j0 < A.right_end[last];
}

template <typename O, bool CLEAN>
__global__ __launch_bounds__(CLEAN ? 64 : 256) void geno_ld_kernel(GenoLdArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = A.pairs[blockIdx.x];
    const int64_t I = pair >> 32, J = pair & 0xffffffffll;
    const int64_t units = A.stride / 16;
    const int h = lane >> 5;
    const ld_acc zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (CLEAN) {
        const int64_t i0 = I * kLdTile, j0 = J * kLdTile;
        const uint4* ra[2];
        const uint4* rb[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {              // (rows beyond m: the last row's words, never stored)
            const int64_t ia = i0 + 32 * f + (lane & 31), jb = j0 + 32 * f + (lane & 31);
            ra[f] = reinterpret_cast<const uint4*>(A.rows + (ia < A.m ? ia : A.m - 1) * A.stride);
            rb[f] = reinterpret_cast<const uint4*>(A.rows + (jb < A.m ? jb : A.m - 1) * A.stride);
        }
        ld_acc acc[2][2] = {{zero, zero}, {zero, zero}};
        uint4 va[2], vb[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) { va[f] = ld_unit(ra[f], h, units); vb[f] = ld_unit(rb[f], h, units); }
        for (int64_t t = 0; t < units; t += 2) {
            uint4 ca[2] = {va[0], va[1]}, cb[2] = {vb[0], vb[1]};
            if (t + 2 < units) {
#pragma unroll
                for (int f = 0; f < 2; ++f) { va[f] = ld_unit(ra[f], t + 2 + h, units); vb[f] = ld_unit(rb[f], t + 2 + h, units); }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ld_frag xa[2], xb[2], none;
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    ld_decode<false>(ld_word(ca[f], k), xa[f], none);
                    ld_decode<false>(ld_word(cb[f], k), xb[f], none);
                }
#pragma unroll
                for (int fa = 0; fa < 2; ++fa)
#pragma unroll
                    for (int fb = 0; fb < 2; ++fb)
                        acc[fa][fb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa[fa], xb[fb], acc[fa][fb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int fa = 0; fa < 2; ++fa)
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
                if (ld_quarter_live(A, i0 + 32 * fa, j0 + 32 * fb))
                    ld_store_quarter<O, true>(A, i0 + 32 * fa, j0 + 32 * fb, lane, acc[fa][fb], zero, zero, zero);
    } else {
        const int wave = threadIdx.x >> 6;
        const int64_t i0 = I * kLdTile + 32 * (wave >> 1), j0 = J * kLdTile + 32 * (wave & 1);
        if (!ld_quarter_live(A, i0, j0)) return;   // (wave-uniform; the waves of a workgroup share nothing)
        const int64_t ia = i0 + (lane & 31), jb = j0 + (lane & 31);
        const uint4* ra = reinterpret_cast<const uint4*>(A.rows + (ia < A.m ? ia : A.m - 1) * A.stride);
        const uint4* rb = reinterpret_cast<const uint4*>(A.rows + (jb < A.m ? jb : A.m - 1) * A.stride);
        ld_acc S = zero, Uij = zero, Uji = zero, N = zero;
        uint4 va = ld_unit(ra, h, units), vb = ld_unit(rb, h, units);
        for (int64_t t = 0; t < units; t += 2) {
            const uint4 ca = va, cb = vb;
            if (t + 2 < units) { va = ld_unit(ra, t + 2 + h, units); vb = ld_unit(rb, t + 2 + h, units); }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ld_frag xa, pa, xb, pb;
                ld_decode<true>(ld_word(ca, k), xa, pa);
                ld_decode<true>(ld_word(cb, k), xb, pb);
                S = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, xb, S, 0, 0, 0);
                Uij = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, pb, Uij, 0, 0, 0);
                Uji = __builtin_amdgcn_mfma_i32_32x32x32_i8(pa, xb, Uji, 0, 0, 0);
                N = __builtin_amdgcn_mfma_i32_32x32x32_i8(pa, pb, N, 0, 0, 0);
            }
        }
        ld_store_quarter<O, false>(A, i0, j0, lane, S, Uij, Uji, N);
    }
}

// geno_ld.hip: the kernels of one call on `stream`: the clean pairs, then the general ones (either list may be empty)
int launch_geno_ld(hipStream_t stream, int out_dtype, GenoLdArgs A, const int64_t* d_pairs_clean, int64_t n_clean,
                   const int64_t* d_pairs_general, int64_t n_general);

}  // namespace viprs
