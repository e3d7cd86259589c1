// Row loads, lane-crossing helpers and the strip updates of the panel scheme (estep_panel.h), shared with the band, tile
// and batched grid kernels.
#pragma once
#include "kernels_common.h"

namespace viprs {

// ---- 4-element row loads, converted with static_cast<float> as e_step.hpp:173 does ----------
template <typename U> __device__ __forceinline__ float4 load4(const U* p);
template <> __device__ __forceinline__ float4 load4<float>(const float* p) {
    return *reinterpret_cast<const float4*>(p);
}
template <> __device__ __forceinline__ float4 load4<int8_t>(const int8_t* p) {
    const int w = *reinterpret_cast<const int*>(p);
    return make_float4((float)(int8_t)(w), (float)(int8_t)(w >> 8), (float)(int8_t)(w >> 16),
                       (float)(int8_t)(w >> 24));
}
template <> __device__ __forceinline__ float4 load4<int16_t>(const int16_t* p) {
    const int2 w = *reinterpret_cast<const int2*>(p);
    return make_float4((float)(int16_t)(w.x), (float)(int16_t)(w.x >> 16), (float)(int16_t)(w.y),
                       (float)(int16_t)(w.y >> 16));
}

// Keeps N wave-uniform values (v_readlane results) in SGPRs at this point of the program: the reads are issued together and
// the scalar chain that consumes them follows without the two wait states a VALU read of a just-written SGPR costs per term.
template <int N> __device__ __forceinline__ void pin_sgprs(int (&v)[N]) {
    static_assert(N == 4 || N == 5 || N == 8 || N == 9, "chain lengths of the K <= 8 mixture step");
    if constexpr (N == 4) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]));
    if constexpr (N == 5) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]));
    if constexpr (N == 8) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]));
    if constexpr (N == 9) asm volatile("" : "+s"(v[0]), "+s"(v[1]), "+s"(v[2]), "+s"(v[3]), "+s"(v[4]), "+s"(v[5]), "+s"(v[6]), "+s"(v[7]),
                                       "+s"(v[8]));
}
// max(x[lane - N], x[lane]) within a row of 16 lanes, lanes without a source keep x (no NaN canonicalisation:
// the operands are finite); the two wait states a DPP read of a fresh VALU result needs are in the asm
template <int N> __device__ __forceinline__ float dpp_max_shr(float x) {
    float r;
    if (N == 1) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "0"(x));
    if (N == 2) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "0"(x));
    if (N == 4) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "0"(x));
    if (N == 8) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "0"(x));
    return r;
}

// r = mask[lane] ? b : a with the lane mask in an SGPR pair (one v_cndmask, no per-step v_cmp)
__device__ __forceinline__ float sel_mask(float a, float b, unsigned long long m) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}

// staged outputs of a team block: another member -- possibly on another XCD, behind another L2 -- copies them into place
// when the block is done, so they are written past the caches (agent scope)
__device__ __forceinline__ void stage_store(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float rl(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// CPL consecutive columns of one LD row exactly as stored (float / int8 / int16), converted with
// static_cast<float> (e_step.hpp:173) only when consumed: the prefetch buffer of an updater lane holds
// raw bytes, so a 16-byte load brings 4 fp32, 8 int16 or 16 int8 columns.
template <typename U, int CPL> struct RawRow {
    static constexpr int kWords = CPL * (int)sizeof(U) / 4;
    static_assert(CPL * sizeof(U) % 4 == 0 && (kWords == 1 || kWords == 2 || kWords == 4), "1, 2 or 4 dwords per lane and row");
    unsigned w[kWords];
    __device__ __forceinline__ float get(int i) const {
        if constexpr (sizeof(U) == 4) return __uint_as_float(w[i]);
        else if constexpr (sizeof(U) == 1) return static_cast<float>(static_cast<int8_t>(w[i >> 2] >> (8 * (i & 3))));
        else return static_cast<float>(static_cast<int16_t>(w[i >> 1] >> (16 * (i & 1))));
    }
};
template <typename U, int CPL> __device__ __forceinline__ RawRow<U, CPL> load_raw(const U* p) {
    RawRow<U, CPL> r;
    if constexpr (RawRow<U, CPL>::kWords == 1) {
        r.w[0] = *reinterpret_cast<const unsigned*>(p);
    } else if constexpr (RawRow<U, CPL>::kWords == 2) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        r.w[0] = t.x; r.w[1] = t.y;
    } else {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        r.w[0] = t.x; r.w[1] = t.y; r.w[2] = t.z; r.w[3] = t.w;
    }
    return r;
}

constexpr int kChainPrefetch = 16;   // diagonal-tile rows in flight ahead of the serial chain
#ifndef PANEL_STRIP_DEPTH
#define PANEL_STRIP_DEPTH 16
#endif
constexpr int kStripRowsInFlight = PANEL_STRIP_DEPTH;   // row loads in flight per updater lane (x 16 B for every LD type)


// Trailing update of one strip (64 * CPL columns) by one wave: q[c..c+CPL-1] = fma(R[row][c..], a_row, .)
// for the 64 rows of a panel, in row order, with DEPTH row loads in flight per lane (DEPTH * CPL = 64
// floats of row data per lane whatever the strip width).  The row loop is rolled in groups of DEPTH
// so that every load is consumed exactly one group later (a fully unrolled loop lets hipcc sink the
// loads next to their uses, leaving two in flight), and there is no runtime guard around any load
// (a guard makes hipcc wait vmcnt(0) per row).  FULL = false (partial last panel of a block): rows
// past its end are clamped to its last row; their a is 0, so fma(R, 0, q) == q leaves q untouched.
// MIXED (mirrored upper form, a strip with columns on both sides of the chain): the multiplier of row j is per lane,
// fvec * avec[j] -- avec = eta_diff of the panel, fvec = 1 for a column left of the chain (a term of its second-pass sum),
// dq right of it (dq * eta_diff[j] IS a_j, the same product the chain formed): one v_mul per row more.
template <typename U, int CPL, bool FULL, int DEPTH = kStripRowsInFlight, bool MIXED = false>
__device__ __forceinline__ void strip_update(const U* __restrict__ rowp, int stride, int last_row, float avec,
                                             float* __restrict__ lq_c, float fvec = 1.0f) {
    static_assert(kPanel % DEPTH == 0, "panel must be a whole number of prefetch groups");
    float qv[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) qv[i] = lq_c[i];
    RawRow<U, CPL> buf[DEPTH];
#pragma unroll
    for (int k = 0; k < DEPTH; ++k)
        buf[k] = load_raw<U, CPL>(rowp + (int64_t)(FULL ? k : min(k, last_row)) * stride);
#pragma unroll 1
    for (int g = 0; g < kPanel / DEPTH - 1; ++g) {
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const RawRow<U, CPL> v = buf[k];
            const int rn = DEPTH * (g + 1) + k;
            buf[k] = load_raw<U, CPL>(rowp + (int64_t)(FULL ? rn : min(rn, last_row)) * stride);
            const float a = MIXED ? fvec * rl(avec, DEPTH * g + k) : rl(avec, DEPTH * g + k);
#pragma unroll
            for (int i = 0; i < CPL; ++i) qv[i] = __builtin_fmaf(v.get(i), a, qv[i]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) {
        const RawRow<U, CPL> v = buf[k];
        const float a = MIXED ? fvec * rl(avec, kPanel - DEPTH + k) : rl(avec, kPanel - DEPTH + k);
#pragma unroll
        for (int i = 0; i < CPL; ++i) qv[i] = __builtin_fmaf(v.get(i), a, qv[i]);
    }
#pragma unroll
    for (int i = 0; i < CPL; ++i) lq_c[i] = qv[i];
}

// Mirrored upper form: the terms of the second-pass sums that lie INSIDE a diagonal tile -- s[i] += R[i, j] ed[j] for the
// SNPs i < j of one panel, read as R[j, i] from row j (lane = column i), rows in ascending order.  The tile is the one the
// chain has just swept, still in LDS (fp32, staged rows past a partial last panel clamped; their eta_diff is 0).
__device__ __forceinline__ float diag_lower_update(const float* __restrict__ tile, float edvec, float sv, int lane) {
#pragma unroll 16
    for (int jr = 0; jr < kPanel; ++jr) {
        const float t = __builtin_fmaf(tile[jr * kPanel + lane], rl(edvec, jr), sv);
        sv = lane < jr ? t : sv;
    }
    return sv;
}

}  // namespace viprs
