// Row loads, lane-crossing helpers and the strip updates of the panel scheme (estep_panel.h), shared with the band, tile
// and batched grid kernels.
#pragma once
#include <type_traits>

#include "kernels_common.h"

namespace viprs {

// ---- cache policy of an LD load ------------------------------------------------------------------
// kCached: a plain load, the default policy.  kStream: a non-temporal load (global_load ... nt) for bytes that are read
// once per sweep by one workgroup: they pass L1 without allocating a line and leave L2 / Infinity Cache to the data that
// is re-used (per-SNP arrays, hand-off granules, team tiles).  Never for bytes several workgroups re-read.  The panel
// sweep picks a policy per load site (estep_panel.h, PanelLdPolicy); every other kernel family loads kCached.
// A streamed row is loaded dword by dword from a pointer of known alignment: hipcc merges the adjacent non-temporal loads
// into one global_load_dwordx2 / dwordx4 ... nt and allocates registers as for the plain load of a uint2 / uint4.  (One
// __builtin_nontemporal_load of a 16-byte ext-vector gives the same instruction, but the prefetch ring of strip_update is
// then copied register by register at the end of every row group: 8 VGPRs more in the symmetric-form kernels.)
constexpr int kCached = 0, kStream = 1;
template <int WORDS, typename W> __device__ __forceinline__ void load_stream(const void* p, W (&w)[WORDS]) {
    static_assert(sizeof(W) == 4 && (WORDS == 1 || WORDS == 2 || WORDS == 4), "1, 2 or 4 dwords");
    const W* q = static_cast<const W*>(__builtin_assume_aligned(p, 4 * WORDS));
#pragma unroll
    for (int i = 0; i < WORDS; ++i) w[i] = __builtin_nontemporal_load(q + i);
}

// ---- 4-element row loads, converted with static_cast<float> as e_step.hpp:173 does ----------
template <typename U, int POLICY = kCached> __device__ __forceinline__ float4 load4(const U* p) {
    static_assert(std::is_same<U, float>::value || std::is_same<U, int8_t>::value || std::is_same<U, int16_t>::value,
                  "float, int8 or int16 LD");
    if constexpr (std::is_same<U, float>::value) {
        if constexpr (POLICY == kStream) {
            float t[4];
            load_stream(p, t);
            return make_float4(t[0], t[1], t[2], t[3]);
        } else {
            return *reinterpret_cast<const float4*>(p);
        }
    } else if constexpr (std::is_same<U, int8_t>::value) {
        int w;
        if constexpr (POLICY == kStream) {
            int t[1];
            load_stream(p, t);
            w = t[0];
        } else {
            w = *reinterpret_cast<const int*>(p);
        }
        return make_float4((float)(int8_t)(w), (float)(int8_t)(w >> 8), (float)(int8_t)(w >> 16),
                           (float)(int8_t)(w >> 24));
    } else {
        int wx, wy;
        if constexpr (POLICY == kStream) {
            int t[2];
            load_stream(p, t);
            wx = t[0]; wy = t[1];
        } else {
            const int2 w = *reinterpret_cast<const int2*>(p);
            wx = w.x; wy = w.y;
        }
        return make_float4((float)(int16_t)(wx), (float)(int16_t)(wx >> 16), (float)(int16_t)(wy),
                           (float)(int16_t)(wy >> 16));
    }
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
template <typename U, int CPL, int POLICY = kCached> __device__ __forceinline__ RawRow<U, CPL> load_raw(const U* p) {
    RawRow<U, CPL> r;
    if constexpr (POLICY == kStream) {
        load_stream(p, r.w);
    } else if constexpr (RawRow<U, CPL>::kWords == 1) {
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
// Cache policy of the panel sweep's LD loads (estep_panel.h, PanelLdPolicy).  -DVIPRS_LD_STREAM=0: every load kCached, the
// device code of the sweep before the policy existed (the A side of tools/ab_bench.py).  The two experiments of
// EXPERIMENTS.md 6.27, each on top of VIPRS_LD_STREAM=1 and neither kept: -DVIPRS_LD_STREAM_PARTIAL=1 streams the
// FULL = false strips too (partial last panel of a block, clamped rows re-read), -DVIPRS_LD_STREAM_NARROW=1 the strips of
// 8 and 4 bytes per lane.  (Through tools/build_variant.sh; none of the three changes a result.)
#ifndef VIPRS_LD_STREAM
#define VIPRS_LD_STREAM 1
#endif
#ifndef VIPRS_LD_STREAM_PARTIAL
#define VIPRS_LD_STREAM_PARTIAL 0
#endif
#ifndef VIPRS_LD_STREAM_NARROW
#define VIPRS_LD_STREAM_NARROW 0
#endif


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
// POLICY: the cache policy of the row loads (kCached / kStream).
template <typename U, int CPL, bool FULL, int DEPTH = kStripRowsInFlight, bool MIXED = false, int POLICY = kCached>
__device__ __forceinline__ void strip_update(const U* __restrict__ rowp, int stride, int last_row, float avec,
                                             float* __restrict__ lq_c, float fvec = 1.0f) {
    static_assert(kPanel % DEPTH == 0, "panel must be a whole number of prefetch groups");
    float qv[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) qv[i] = lq_c[i];
    RawRow<U, CPL> buf[DEPTH];
#pragma unroll
    for (int k = 0; k < DEPTH; ++k)
        buf[k] = load_raw<U, CPL, POLICY>(rowp + (int64_t)(FULL ? k : min(k, last_row)) * stride);
#pragma unroll 1
    for (int g = 0; g < kPanel / DEPTH - 1; ++g) {
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const RawRow<U, CPL> v = buf[k];
            const int rn = DEPTH * (g + 1) + k;
            buf[k] = load_raw<U, CPL, POLICY>(rowp + (int64_t)(FULL ? rn : min(rn, last_row)) * stride);
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
