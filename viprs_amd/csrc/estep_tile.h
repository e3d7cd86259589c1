// float64 state (float_precision='float64', VIPRS.py:72): the E-step walked in 64-SNP panels by one workgroup per LD
// block -- the panel scheme of estep_panel.h in its plainest form (no teams, no hand-off), for the state type the panel
// kernels do not specialise.  Per panel p:
//   1. its 64 x 64 diagonal tile and the off-diagonal tile (rows of panel p - 1, columns of panel p) go into LDS, 0
//      outside a row's window (fetched one panel ahead by waves 1 .. NW - 1);
//   2. wave 0 applies the rows of panel p - 1 to its 64 columns (64 fma per lane), then runs the 64 sequential updates
//      (e_step.hpp:401-431) with q of the panel in its lanes' registers -- the in-panel part of every row's axpy
//      (e_step.hpp:421) is one fma per step, the skip branch a select -- and leaves a_j = dq * eta_diff_j in LDS;
//   3. meanwhile waves 1 .. NW - 1 apply the rows of panel p - 1 to the columns outside panels p - 1 and p,
//      q[c] = fma(R[j,c], a_j, q[c]) for j in panel order: every q[c] sees its rows in the order the reference applies
//      them (symmetric form: the same fma sequence per element).
// The second pass of the upper-triangular form (update_q_factor, e_step.hpp:331-337) is its own launch over the rows of
// all blocks, one wave per group of 8 rows with the lanes across the columns (coalesced); the dot is summed in
// lane-partial order there, NOT in the reference's index order.  A float64 state is compared to the reference within
// 1e-10, never bit for bit (the chain's exp is not glibc's, see below).  Models: spike-and-slab, the columns of a grid, the
// sparse mixture with up to 4 components.  The row-by-row kernels of estep_generic.h remain for what this file does not
// cover: mixtures of more than 4 components with a float64 state, blocks whose q does not fit the LDS.
#pragma once
#include "device_math.h"
#include "estep_generic.h"
#include "kernels_common.h"
#include "panel_loads.h"         // RawRow / load_raw

namespace viprs {

constexpr int kTileThreads = 256;
// step 3: a thread owns CPT adjacent columns (16 bytes of a row: one vector load; at least 4 columns), and the loads
// of RIF rows are in flight at a time (64 VGPRs of row data)
template <typename U> constexpr int tile_cpt() { return sizeof(U) >= 4 ? 4 : 16 / (int)sizeof(U); }
template <typename U> constexpr int tile_rif() { return 256 / (tile_cpt<U>() * (int)sizeof(U)); }

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------------------------------------------------------
// The chain's sigmoid: BIT-IDENTICAL to the reference's on the host (round 5) -- glibc's double exp (device_math.h:
// exp_glibc_f64_*, the library's own constants) and an IEEE divide.  The chain evaluates wave-uniform scalars (every lane
// the same numbers from the step's SNP), so the lookup in the table of 2^(k/128) = scale (1 + tail) is ONE broadcast
// 16-byte LDS read per exp (the table, 2 KB, is copied to LDS when the kernel starts); the special ranges (|x| < 2^-54,
// x <= -512: subnormal results, 0, nan) are one uniform branch behind the common path.
// (Rounds 2-4 ran a shorter chain here -- a 64-entry table, a degree-6 polynomial, v_rcp_f64 + Newton + correction:
//  < 2 ulp from the reference, compared at 1e-10.)
// ---------------------------------------------------------------------------------------------------------------
struct ExpTab64 {
    const unsigned long long* t;                             // the 2 x 128-entry table in LDS (2 KB)
    // every thread of the workgroup takes part (the workgroups have 256 or 512 threads)
    __device__ __forceinline__ void init(unsigned long long* lds) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) lds[i] = kExp64Tab[i];
        __syncthreads();
        t = lds;
    }
};

__device__ __forceinline__ double exp_nonpos_f64_uniform(double t, const ExpTab64& tab) {
    const Exp64Reduced q = exp_glibc_f64_reduce(t);
    // wave-uniform k: ONE 16-byte LDS read (a broadcast) brings tail and scale of entry k % 128; it is issued as soon as
    // kd is known and lands while r and the polynomial's first terms are computed
    const int k = __builtin_amdgcn_readfirstlane((int)(unsigned)q.ki);
    const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(tab.t + 2 * (k & 127));
    return exp_glibc_f64_core<true>(t, q, __longlong_as_double((long long)e.x), e.y);
}

__device__ __forceinline__ double sigmoid_f64_uniform(double x, const ExpTab64& tab) {
    const double e = exp_nonpos_f64_uniform(-fabs(x), tab);
    const double num = (x < 0.0) ? e : 1.0;
    return div_unit_range_f64(num, 1.0 + e);                  // e_step.hpp:254-260: IEEE add and divide (device_math.h)
}

// spike-and-slab (e_step.hpp:401-413) / one model of the grid (e_step.hpp:613-620: no skip branch, half_var_tau, no fma)
constexpr int kTileMixK = 4;       // sparse mixture on this kernel: up to 4 components with the inputs prefetched a panel ahead,
constexpr int kTileMixWideK = 10;  // up to 10 (the reference's own test, tests/test_basic.py:60) loading them at the panel's start
                                   // (more: estep_generic.h)

struct TileSpikeSlab {
    static constexpr bool kSkip = true;
    static constexpr bool kMixture = false;
    static constexpr int kSlots = 1;
    __device__ static __forceinline__ void update(double mm, double beta, double s, double ulog, double eta_old, double qj,
                                                  const ExpTab64& tab, double& mu, double& gamma, double& d) {
        const double p = mm * qj;
        mu = __builtin_fma(mm, beta, -p);
        const double u = s * mu;
        gamma = sigmoid_f64_uniform(__builtin_fma(u, u, ulog), tab);
        d = __builtin_fma(gamma, mu, -eta_old);
    }
};
struct TileGridColumn {
    static constexpr bool kSkip = false;
    static constexpr bool kMixture = false;
    static constexpr int kSlots = 1;
    __device__ static __forceinline__ void update(double mm, double beta, double hvt, double ulog, double eta_old, double qj,
                                                  const ExpTab64& tab, double& mu, double& gamma, double& d) {
        mu = mm * (beta - qj);
        const double uj = ulog + hvt * mu * mu;
        gamma = sigmoid_f64_uniform(uj, tab);
        d = gamma * mu - eta_old;
    }
};

// e_step_mixture (e_step.hpp:447-551) with K <= kTileMixK components: the chain wave evaluates the K components of the
// step's SNP as wave-uniform scalars (every lane the same numbers -- no cross-lane reduction; the K exponentials and the
// K divides are independent of each other and overlap), lane l keeps the K inputs / outputs of SNP l of the panel.
// KMAX = kTileMixWideK: 3 x 10 + 3 doubles of inputs per lane -- a second set in flight for the next panel would not fit the
// registers next to the K outputs and the step's K exponentials, so the chain wave loads its inputs when the panel starts
// (one exposed round trip per 64 steps of ~1 us each).
template <int KMAX>
struct TileMixture {
    static constexpr bool kSkip = false;
    static constexpr bool kMixture = true;
    static constexpr int kSlots = KMAX;
};

template <typename U, int N> struct alignas(sizeof(U) * N) UVec { U v[N]; };

// LDS: q[qcap] (doubles) | diagonal tile [64][64] | off-diagonal tile [64][64] (LD elements, 0 outside a row's window) |
// per panel parity: a[64] (doubles), rowbase[64] (int64), ws[64], we[64] (ints)
__host__ __device__ constexpr size_t tile_lds_bytes(int qcap, size_t ld_elem) {
    return (size_t)qcap * 8 + 2 * kPanel * kPanel * ld_elem + 2 * (kPanel * 8 + kPanel * 8 + 2 * kPanel * 4);
}

// window of one LD row, block-local columns [ws, we), and the element offset of (row, block column 0)
struct TileWindow { int ws, we; int64_t base; };

// Panel p's chain (wave 0) runs side by side with the rows of panel p - 1 going onto the columns outside panels
// p - 1 and p (waves 1..3): before its chain, wave 0 itself applies those rows to ITS 64 columns from the off-diagonal
// tile in LDS (64 fma per lane).  Everything a panel needs from global memory -- its inputs, its two tiles, the windows
// of its rows (those two panels ahead: the tiles' addresses come from them) -- is fetched one panel ahead into
// registers while the chain of the panel before runs.
#ifdef VIPRS_TILE_PROFILE
#define TPROF(i) do { if (wave == 0 && lane == 0 && blockIdx.x == 0 && (p0 >> 6) < 24) s_tp[p0 >> 6][i] = wall_clock64(); } while (0)
#else
#define TPROF(i) do { } while (0)
#endif

template <typename U, typename MODEL, bool DENSE, int NW>
__global__ __launch_bounds__(NW * 64) void estep_tile_f64_kernel(EStepArgs<double> A0, int qcap) {
    using T = double;
    constexpr int NT = NW * 64;                                // 1 chain wave + NW - 1 waves for the tiles and the row pass
#ifdef VIPRS_TILE_PROFILE
    __shared__ unsigned long long s_tp[24][8];
#endif
    // Waves 1 .. NW - 1 fetch and stage the tiles (rows w - 1, w - 1 + (NW - 1), ...): the chain wave issues no vector-memory
    // instruction but the loads of its own per-SNP inputs, one panel ahead -- under the row pass's load its issue stalls for
    // microseconds (measured: 16 tile-row loads 1.6 us in a quiet workgroup, 4 us next to a 3 648-column row pass).
    constexpr int kWaves = NW;
    constexpr int kRowsPerWave = (kPanel + kWaves - 2) / (kWaves - 1);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* const qv = reinterpret_cast<T*>(smem_raw);
    U* const tile_d = reinterpret_cast<U*>(qv + qcap);         // rows of panel p, columns of panel p
    U* const tile_o = tile_d + kPanel * kPanel;                // rows of panel p - 1, columns of panel p
    T* const s_a = reinterpret_cast<T*>(tile_o + kPanel * kPanel);         // [2][64]: a_j = dq * eta_diff_j
    int64_t* const s_base = reinterpret_cast<int64_t*>(s_a + 2 * kPanel);  // [2][64]
    int* const s_ws = reinterpret_cast<int*>(s_base + 2 * kPanel);         // [2][64]
    int* const s_we = s_ws + 2 * kPanel;                                   // [2][64]
    __shared__ int s_item;
    __shared__ int s_cmin[2], s_cmax[2];                                   // union of the panel's row windows
    __shared__ unsigned long long s_applied[2];                            // rows of the panel that were not skipped

    __shared__ __attribute__((aligned(16))) unsigned long long s_exp64[256];   // glibc's exp table (device_math.h)
    ExpTab64 tab;
    tab.init(s_exp64);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n_models = max(1, A0.n_active);
    const int64_t n_items = (int64_t)A0.n_blocks * n_models;
    const U* __restrict__ ld = static_cast<const U*>(DENSE ? A0.ld_dense : A0.ld_rows);
    const T eps = Eps<T>::value;
    unsigned long long my_skipped = 0;

    for (;;) {
        if (tid == 0) s_item = atomicAdd(A0.counter, 1);
        __syncthreads();
        const int item = s_item;
        __syncthreads();
        if (item >= n_items) break;
        const BlockDesc bd = A0.blocks[item / n_models];
        const EStepArgs<T> A = select_model(A0, item % n_models);
        const int64_t s0 = bd.start;
        const int n = bd.size;

        // window of row `row` of a dense block: no index loads (symmetric form: the whole block; upper form: right of the
        // diagonal; rows beyond the block: empty)
        auto dense_row = [&](int row) {
            TileWindow w;
            w.ws = A.low_memory ? row + 1 : 0;
            w.we = row < n ? n : w.ws;
            w.base = bd.ld_off + (int64_t)row * bd.stride;
            return w;
        };
        auto load_window = [&](int p0) {                       // lane l: row p0 + l
            if (DENSE) return dense_row(p0 + lane);
            TileWindow w{0, 0, 0};
            if (p0 + lane < n) {
                const int64_t j = s0 + p0 + lane;
                w.ws = A.lb[j] - (int)s0;
                w.we = w.ws + A.rowlen[j];
                w.base = A.rowstart[j] - w.ws;
            }
            return w;
        };
        // window of row r0 + jj (jj uniform): arithmetic for dense blocks, out of the lanes' registers otherwise
        auto row_window = [&](const TileWindow& w, int r0, int jj) {
            if (DENSE) return dense_row(r0 + jj);
            TileWindow r;
            r.ws = __builtin_amdgcn_readlane(w.ws, jj);
            r.we = __builtin_amdgcn_readlane(w.we, jj);
            const int lo = __builtin_amdgcn_readlane((int)(uint32_t)w.base, jj);
            const int hi = __builtin_amdgcn_readlane((int)(w.base >> 32), jj);
            r.base = ((int64_t)hi << 32) | (uint32_t)lo;
            return r;
        };
        // a 64 x 64 tile: rows r0 .. r0 + 63 (windows `w`), columns c0 + lane; this wave's rows of it
        // Entries outside a row's window are staged as 0: the chain applies every row to all its 64 lanes without a
        // window test (fma(0, a, q) == q).
        constexpr int n_stagers = kWaves - 1;
        const int stager = wave - 1;                                   // -1: the chain wave sits out
        auto load_tile = [&](U (&t)[kRowsPerWave], const TileWindow& w, int r0, int c0) {
            if (stager < 0) return;
            const int c = c0 + lane;
#pragma unroll
            for (int k = 0; k < kRowsPerWave; ++k) {
                const int jj = stager + n_stagers * k;
                if (jj >= kPanel) break;
                const TileWindow r = row_window(w, r0, jj);
                t[k] = (c >= r.ws && c < r.we) ? ld[r.base + c] : (U)0;          // (rows beyond the block: ws == we)
            }
        };
        auto store_tile = [&](const U (&t)[kRowsPerWave], U* tile) {
            if (stager < 0) return;
#pragma unroll
            for (int k = 0; k < kRowsPerWave; ++k) {
                const int jj = stager + n_stagers * k;
                if (jj < kPanel) tile[jj * kPanel + lane] = t[k];
            }
        };
        constexpr int KM = MODEL::kSlots;                      // per-SNP input slots (mixture: one per component)
        constexpr bool kPrefetchInputs = KM <= kTileMixK;
        const int K = MODEL::kMixture ? A.width : 1;
        T in_mm[KM], in_sh[KM], in_ul[KM], in_sb = 0, in_eta = 0, in_lnp = 0;
#pragma unroll
        for (int k = 0; k < KM; ++k) in_mm[k] = in_sh[k] = in_ul[k] = 0;
        auto load_inputs = [&](int p0) {
            if (wave == 0 && p0 < n) {
                const int64_t jl = s0 + min(p0 + lane, n - 1);
                if constexpr (MODEL::kMixture) {
#pragma unroll
                    for (int k = 0; k < KM; ++k) {
                        if (k < K) { in_mm[k] = A.mu_mult[jl * K + k]; in_sh[k] = A.shvt[jl * K + k]; in_ul[k] = A.u_logs[jl * K + k]; }
                    }
                    in_lnp = A.log_null_pi[jl];
                } else {
                    in_mm[0] = A.mu_mult[jl]; in_sh[0] = A.shvt[jl]; in_ul[0] = A.u_logs[jl];
                }
                in_sb = A.std_beta[jl]; in_eta = A.eta[jl];
            }
        };
        // rows of the panel at r0 (parity `par`) onto the columns outside [x0, x1), by threads u of nu: a thread owns 4
        // adjacent columns; the loads of RIF rows are in flight at a time.  Dense blocks: every row of the panel reaches
        // every column outside it (symmetric form) / to the right of it (upper form) -- no per-element window test;
        // windowed rows: element loads and tests.
        auto rows_onto_columns = [&](int par, int x0, int x1, int u, int nu) {
            constexpr int CPT = 4;
            constexpr int RIF = DENSE ? 64 / (int)sizeof(U) : 8;        // 64 VGPRs of row data in flight per lane
            const unsigned long long applied = s_applied[par];
            if (applied == 0) return;
            const T* const pa = s_a + par * kPanel;
            const int64_t* const pbase = s_base + par * kPanel;
            const int* const pws = s_ws + par * kPanel;
            const int* const pwe = s_we + par * kPanel;
            const int cmin = s_cmin[par] & ~(CPT - 1), cmax = s_cmax[par];
            if constexpr (DENSE) {
                for (int cb = cmin + CPT * u; cb < cmax; cb += CPT * nu) {
                    if (cb >= x0 && cb < x1) continue;                           // (panels start at multiples of 64)
                    T v[CPT];
#pragma unroll
                    for (int x = 0; x < CPT; ++x) v[x] = cb + x < n ? qv[cb + x] : (T)0;
                    for (int j0 = 0; j0 < kPanel; j0 += RIF) {
                        UVec<U, CPT> r[RIF];
#pragma unroll
                        for (int k = 0; k < RIF; ++k) r[k] = *reinterpret_cast<const UVec<U, CPT>*>(ld + pbase[j0 + k] + cb);   // (rows are padded to 64)
#pragma unroll
                        for (int k = 0; k < RIF; ++k) {
                            if (!((applied >> (j0 + k)) & 1ull)) continue;
                            const T a = pa[j0 + k];
#pragma unroll
                            for (int x = 0; x < CPT; ++x) v[x] = __builtin_fma(static_cast<T>(r[k].v[x]), a, v[x]);
                        }
                    }
#pragma unroll
                    for (int x = 0; x < CPT; ++x)
                        if (cb + x < n) qv[cb + x] = v[x];
                }
            } else {
                for (int cb = cmin + CPT * u; cb < cmax; cb += CPT * nu) {
                    if (cb >= x0 && cb < x1) continue;                           // (panels start at multiples of 64)
                    T v[CPT];
#pragma unroll
                    for (int x = 0; x < CPT; ++x) v[x] = cb + x < n ? qv[cb + x] : (T)0;
                    for (int j0 = 0; j0 < kPanel; j0 += RIF) {
                        U r[RIF][CPT];
#pragma unroll
                        for (int k = 0; k < RIF; ++k) {
#pragma unroll
                            for (int x = 0; x < CPT; ++x) {
                                const int c = cb + x;
                                r[k][x] = (c >= pws[j0 + k] && c < pwe[j0 + k]) ? ld[pbase[j0 + k] + c] : (U)0;
                            }
                        }
#pragma unroll
                        for (int k = 0; k < RIF; ++k) {
                            const int jj = j0 + k;
                            if (!((applied >> jj) & 1ull)) continue;
                            const T a = pa[jj];
                            const int ws = pws[jj], we = pwe[jj];
#pragma unroll
                            for (int x = 0; x < CPT; ++x) {
                                const int c = cb + x;
                                const T w = __builtin_fma(static_cast<T>(r[k][x]), a, v[x]);
                                v[x] = (c >= ws && c < we) ? w : v[x];
                            }
                        }
                    }
#pragma unroll
                    for (int x = 0; x < CPT; ++x)
                        if (cb + x < n) qv[cb + x] = v[x];
                }
            }
        };

        for (int i = tid; i < n; i += NT) qv[i] = A.q[s0 + i];
        TileWindow w_cur = load_window(0), w_nxt = load_window(kPanel);
        U t_d[kRowsPerWave], t_o[kRowsPerWave];
        load_tile(t_d, w_cur, 0, 0);
#pragma unroll
        for (int k = 0; k < kRowsPerWave; ++k) t_o[k] = (U)0;
        if (kPrefetchInputs) load_inputs(0);
        T prev_a = 0;                                          // wave 0, lane jj: a_jj of the panel before (0: skipped)

        for (int p0 = 0; p0 < n; p0 += kPanel) {
            const int np = min(kPanel, n - p0);
            const int par = (p0 >> 6) & 1;
            TPROF(0);
            // ---- 1. the prefetched panel into LDS (the chain before is done with the tiles: barrier at the loop's end) --
            if (wave == 0) {
                s_ws[par * kPanel + lane] = w_cur.ws;
                s_we[par * kPanel + lane] = w_cur.we;
                s_base[par * kPanel + lane] = w_cur.base;
                int cmin, cmax;
                if (DENSE) {
                    cmin = A.low_memory ? p0 + 1 : 0;
                    cmax = n;
                } else {
                    cmin = w_cur.we > w_cur.ws ? w_cur.ws : n;
                    cmax = w_cur.we > w_cur.ws ? w_cur.we : 0;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        cmin = min(cmin, __shfl_xor(cmin, off));
                        cmax = max(cmax, __shfl_xor(cmax, off));
                    }
                }
                if (lane == 0) { s_cmin[par] = cmin; s_cmax[par] = cmax; }
            }
            store_tile(t_d, tile_d);
            if (p0 > 0) store_tile(t_o, tile_o);
            if (!kPrefetchInputs) load_inputs(p0);
            T c_mm[KM], c_sh[KM], c_ul[KM];
#pragma unroll
            for (int k = 0; k < KM; ++k) { c_mm[k] = in_mm[k]; c_sh[k] = in_sh[k]; c_ul[k] = in_ul[k]; }
            const T c_sb = in_sb, c_eta = in_eta, c_lnp = in_lnp;
            TPROF(1);
            __syncthreads();
            TPROF(2);
            // ---- prefetch for the panel after this one (in flight during the chain) ----------------------------------
            const TileWindow w_nn = load_window(p0 + 2 * kPanel);
            load_tile(t_d, w_nxt, p0 + kPanel, p0 + kPanel);
            load_tile(t_o, w_cur, p0, p0 + kPanel);
            if (kPrefetchInputs) load_inputs(p0 + kPanel);
            TPROF(3);

            if (wave == 0) {
                // ---- 2. the chain: lane l carries q of SNP p0 + l ---------------------------------------------------
                T ql = qv[p0 + min(lane, np - 1)];
                // the rows of the panel before onto these 64 columns first (e_step.hpp:421 for j in that panel; a skipped
                // row carries a = 0: fma(r, 0, q) == q); 8 rows' LDS reads in flight at a time
                // (Entries outside a row's window are staged as 0, and fma(0, a, q) == q only for a FINITE a: the reference does
                //  not touch q outside the window whatever a is, so a column outside the window keeps its q by a select --
                //  dense blocks: every column of this panel is inside the windows of the panel before, no test.)
                if (p0 > 0) {
                    const int* const ows = s_ws + (par ^ 1) * kPanel;
                    const int* const owe = s_we + (par ^ 1) * kPanel;
                    for (int j0 = 0; j0 < kPanel; j0 += 8) {
                        T rr[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) rr[k] = static_cast<T>(tile_o[(j0 + k) * kPanel + lane]);
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const T v = __builtin_fma(rr[k], readlane_f64(prev_a, j0 + k), ql);
                            if constexpr (DENSE) ql = v;
                            else ql = (p0 + lane >= ows[j0 + k] && p0 + lane < owe[j0 + k]) ? v : ql;
                        }
                    }
                }
                TPROF(4);
                T o_mu[KM], o_gam[KM], o_eta = 0, o_ed = 0, o_a = 0;
#pragma unroll
                for (int k = 0; k < KM; ++k) o_mu[k] = o_gam[k] = 0;
                unsigned long long applied_v = 0;              // (the same value in every lane)
                // The step has no branch and no memory operation between q_j and the new q: the tile row of step jj + 1 is
                // read from LDS while step jj computes, the skip branch (e_step.hpp:410-413) is a select -- a skipped SNP
                // applies a = 0 (fma(r, 0, q) == q) and keeps its outputs.
                T r_nxt = static_cast<T>(tile_d[lane]);
                // Columns outside the window of row jj keep their q (see above).
                //   windowed rows: the row's own bounds, read one step ahead like the tile row, and a select on the step;
                //   dense blocks, upper form: a column c is outside the windows of the rows jj >= c only, so its final value is
                //     the q its OWN step consumed -- captured beside the chain (`q_keep`: nothing depends on it), no select on
                //     the serial path; symmetric form: every column of the panel is inside every window.
                const int* const dws = s_ws + par * kPanel;
                const int* const dwe = s_we + par * kPanel;
                bool in_nxt = DENSE ? true : (p0 + lane >= dws[0] && p0 + lane < dwe[0]);
                T q_keep = ql;
                for (int jj = 0; jj < np; ++jj) {
                    const T r = r_nxt;
                    const bool in_win = in_nxt;
                    r_nxt = static_cast<T>(tile_d[min(jj + 1, kPanel - 1) * kPanel + lane]);
                    if constexpr (!DENSE) {
                        const int jn = min(jj + 1, kPanel - 1);
                        in_nxt = p0 + lane >= dws[jn] && p0 + lane < dwe[jn];
                    }
                    if constexpr (DENSE) q_keep = (lane == jj) ? ql : q_keep;
                    const T qj = readlane_f64(ql, jj);
                    const T eta_old = readlane_f64(c_eta, jj);
                    T mu[KM], gam[KM], d;
                    // (all lanes compute the same numbers from lane jj's inputs: wave-uniform)
                    if constexpr (MODEL::kMixture) {
                        const T rq = readlane_f64(c_sb, jj) - qj;                             // e_step.hpp:505
                        const T lnp = readlane_f64(c_lnp, jj);
                        T u[KM], mx = lnp;
#pragma unroll
                        for (int k = 0; k < KM; ++k) {
                            mu[k] = readlane_f64(c_mm[k], jj) * rq;                           // :509
                            const T t = readlane_f64(c_sh[k], jj) * mu[k];
                            u[k] = __builtin_fma(t, t, readlane_f64(c_ul[k], jj));            // :511
                            if (k < K) mx = fmax(mx, u[k]);                                   // c_max, :58-71
                        }
                        T ssum = 0;                                                           // softmax, :231-240: k = 0 .. K in order
#pragma unroll
                        for (int k = 0; k < KM; ++k) {
                            if (k < K) {
                                u[k] = exp_nonpos_f64_uniform(u[k] - mx, tab);
                                ssum += u[k];
                            }
                        }
                        ssum += exp_nonpos_f64_uniform(lnp - mx, tab);
                        d = -eta_old;                                                         // :519
#pragma unroll
                        for (int k = 0; k < KM; ++k) {
                            gam[k] = 0;
                            if (k < K) {
                                gam[k] = u[k] / ssum;                                         // :239
                                d = __builtin_fma(gam[k], mu[k], d);                          // :523
                            }
                        }
                    } else {
                        MODEL::update(readlane_f64(c_mm[0], jj), readlane_f64(c_sb, jj), readlane_f64(c_sh[0], jj),
                                      readlane_f64(c_ul[0], jj), eta_old, qj, tab, mu[0], gam[0], d);
                    }
                    const bool skip = MODEL::kSkip && fabs(d) < eps;                          // e_step.hpp:410
                    const T de = skip ? (T)0 : d;                                             // :412
                    const T a = A.dq * de;
                    const T v = (DENSE || in_win) ? __builtin_fma(r, a, ql) : ql;             // :421, in-panel columns of the row's window
                    const bool own = lane == jj;
                    ql = (own && !A.low_memory) ? v - de : v;                                 // :427
                    const bool take = own && !skip;                                           // :416-418, :431
#pragma unroll
                    for (int k = 0; k < KM; ++k) {
                        o_mu[k] = take ? mu[k] : o_mu[k];
                        o_gam[k] = take ? gam[k] : o_gam[k];
                    }
                    o_eta = take ? eta_old + d : o_eta;
                    o_ed = take ? d : o_ed;
                    o_a = take ? a : o_a;
                    applied_v |= skip ? 0ull : (1ull << jj);
                }
                TPROF(5);
                const unsigned long long applied = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(applied_v >> 32)) << 32) |
                                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)applied_v);
                if (DENSE && A.low_memory) ql = q_keep;
                if (lane < np) {
                    const int64_t j = s0 + p0 + lane;
                    qv[p0 + lane] = ql;
                    A.eta_diff[j] = o_ed;
                    if ((applied >> lane) & 1ull) {
#pragma unroll
                        for (int k = 0; k < KM; ++k) {
                            if (k < K) {
                                A.var_mu[j * K + k] = o_mu[k];
                                A.var_gamma[j * K + k] = o_gam[k];
                            }
                        }
                        A.eta[j] = o_eta;
                    }
                }
                s_a[par * kPanel + lane] = o_a;
                if (lane == 0) {
                    s_applied[par] = applied;
                    my_skipped += (unsigned long long)(np - __popcll(applied));
                }
                prev_a = o_a;
                TPROF(6);
            } else if (p0 > 0) {
                // ---- 3. meanwhile: the rows of the panel before onto the columns outside that panel and this one -------
                rows_onto_columns(par ^ 1, p0 - kPanel, p0 + kPanel, tid - 64, NT - 64);
            }
            __syncthreads();
            TPROF(7);
            w_cur = w_nxt;
            w_nxt = w_nn;
        }
#ifdef VIPRS_TILE_PROFILE
        if (tid == 0 && blockIdx.x == 0 && n >= 640) {
            for (int p = 0; p < min(24, (n + 63) / 64); ++p) {
                const unsigned long long t = s_tp[p][0];
                printf("panel %2d @%7llu: staged %4d barrier %4d prefetch-issued %4d priority %4d chain %5d stores %5d end %5d (x10ns)\n", p,
                       t - s_tp[0][0], (int)(s_tp[p][1] - t), (int)(s_tp[p][2] - t), (int)(s_tp[p][3] - t), (int)(s_tp[p][4] - t),
                       (int)(s_tp[p][5] - t), (int)(s_tp[p][6] - t), (int)(s_tp[p][7] - t));
            }
        }
#endif
        // the rows of the last panel onto the columns outside it (a partial last panel has no skipped-row bits beyond np)
        {
            const int last = (n - 1) / kPanel * kPanel;
            rows_onto_columns((last >> 6) & 1, last, last + kPanel, tid, NT);
        }
        __syncthreads();
        for (int i = tid; i < n; i += NT) A.q[s0 + i] = qv[i];
        __syncthreads();
    }
    if (tid == 0 && my_skipped) atomicAdd(A0.skipped, my_skipped);
}

constexpr int kTileGroupRows = 8;       // second pass: rows per record of the plan's row lists (a 64-row group starts at every 8th)

// A half tile (64 rows x 32 columns) for a lane-per-ROW chain: COALESCED loads -- instruction i covers rows i * 64 / N .. of
// the row panel, N lanes per row (one 16-byte piece each): 8 .. 32 cache lines per instruction instead of 64 -- and
// `to_rows`, which hands every lane the N pieces of its own row through a 32-row LDS buffer of the wave (two rounds; pieces
// rotated by the row so that both the 16-byte writes and the 16-byte reads are conflict-free).  (Half a tile per unit, so
// that the next unit's loads can be in flight while the current one is accumulated without a second tile's worth of registers.)
template <typename U> struct HalfTileRows {
    static constexpr int C = 16 / (int)sizeof(U);      // columns per 16-byte load
    static constexpr int N = (kPanel / 2) / C;         // loads per lane and half tile
    RawRow<U, C> v[N];
    static constexpr int kRowBytes = N * 16;
    static constexpr int kRowsPerLoad = kPanel / N;
    static constexpr int kBufBytes = 32 * kRowBytes;
    static __device__ __forceinline__ int rot(int row) { return (row / (8 / N)) % N; }
    __device__ __forceinline__ void load_co(const U* __restrict__ col0, int64_t stride, int row0, int b, int lane) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int row = min(row0 + i * kRowsPerLoad + lane / N, b - 1);      // rows past the block: clamped, never used
            v[i] = load_raw<U, C>(col0 + (int64_t)row * stride + (lane % N) * C);
        }
    }
    __device__ __forceinline__ void to_rows(char* __restrict__ buf, int lane) {
        static_assert(N == 2 || N == 4 || N == 8, "pieces per row");
        RawRow<U, C> out[N];
#pragma unroll
        for (int round = 0; round < 2; ++round) {
#pragma unroll
            for (int k = 0; k < N / 2; ++k) {
                const int i = round * (N / 2) + k;
                const int row = k * kRowsPerLoad + lane / N;                      // 0 .. 31 within the round
                const int slot = (lane % N + rot(row)) % N;
                *reinterpret_cast<uint4*>(buf + row * kRowBytes + slot * 16) = uint4{v[i].w[0], v[i].w[1], v[i].w[2], v[i].w[3]};
            }
            __builtin_amdgcn_wave_barrier();
            if ((lane >> 5) == round) {
                const int row = lane & 31;
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    const uint4 t = *reinterpret_cast<const uint4*>(buf + row * kRowBytes + ((c + rot(row)) % N) * 16);
                    out[c].w[0] = t.x; out[c].w[1] = t.y; out[c].w[2] = t.z; out[c].w[3] = t.w;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int c = 0; c < N; ++c) v[c] = out[c];
    }
};

// ---------------------------------------------------------------------------------------------------------------
// Second pass of the upper-triangular form, update_q_factor (e_step.hpp:331-337): q[j] += dq * dot(eta_diff[win(j)],
// row(j)), in the REFERENCE'S ORDER: dot() of e_step.hpp:82-104 is a serial fma chain over a row's columns in index order,
// so a LANE owns a ROW and walks its columns in ascending order -- q of the upper-triangular form equals the reference's
// bit for bit.  (Rounds 3-5 also carried two shorter passes that summed per lane and across lanes, 1e-10 from the reference,
// for math_mode = fast; a float64 state now always takes this one: every float64 result is `==`.)  One wave per group of 64
// consecutive rows (the records of `groups` whose first row is a multiple of 64).
//   The terms on and left of the diagonal do not exist in the reference's dot (its row starts at column j + 1): the stored
//   zeros there are SKIPPED, not multiplied -- fma(0, eta_diff, s) would turn a non-finite eta_diff[c], c <= j, into a NaN in
//   q[j] that the reference does not produce.
//   dense blocks, LD elements of 1 / 2 / 4 bytes: a tile of 64 rows x 32 columns is loaded coalesced and handed to the
//     rows through the wave's LDS buffer (HalfTileRows above), eta_diff of the
//     tile's 64 columns sits in LDS as doubles (broadcast reads); the next half tile's loads are in flight while the
//     current one is accumulated; a tile whose eta_diff are all zero (skipped SNPs) is not read: fma(R, 0, s) == s.
//   everything else (windowed components, 8-byte LD elements): element by element along the row.
// ---------------------------------------------------------------------------------------------------------------
template <typename U, int C>
__device__ __forceinline__ double raw_elem_f64(const RawRow<U, C>& v, int e) {
    if constexpr (std::is_same<U, float>::value) return (double)__uint_as_float(v.w[e]);
    else if constexpr (sizeof(U) == 4) return (double)(int)v.w[e];
    else if constexpr (sizeof(U) == 1) return (double)static_cast<int8_t>(v.w[e >> 2] >> (8 * (e & 3)));
    else return (double)static_cast<int16_t>(v.w[e >> 1] >> (16 * (e & 1)));
}

template <typename U, bool DENSE>
__global__ __launch_bounds__(kTileThreads, 2) void tile_f64_second_pass_exact_kernel(EStepArgs<double> A0,
                                                                                    const int64_t* __restrict__ groups,
                                                                                    int64_t n_groups) {
    using T = double;
    constexpr bool kTiled = DENSE && sizeof(U) <= 4;
    constexpr int kWavesPerWg = kTileThreads / 64;
    using H = HalfTileRows<typename std::conditional<kTiled, U, float>::type>;
    __shared__ __attribute__((aligned(16))) char s_tbuf[kWavesPerWg][H::kBufBytes];
    __shared__ __attribute__((aligned(16))) double s_ed[kWavesPerWg][kPanel];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerWg + wib;
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerWg;
    const int n_models = max(1, A0.n_active);
    const int64_t n_items = n_groups * n_models;
    const U* __restrict__ ld = static_cast<const U*>(DENSE ? A0.ld_dense : A0.ld_rows);
    char* __restrict__ tbuf = s_tbuf[wib];
    double* __restrict__ edl = s_ed[wib];
    for (int64_t item = wave; item < n_items; item += n_waves) {
        const int64_t g = groups[item % n_groups];
        const int r0 = (int)(uint32_t)g;
        if (r0 & (kPanel - 1)) continue;                          // (records are per 8 rows: a 64-row group starts at every 8th)
        const BlockDesc bd = A0.blocks[(int)(g >> 32)];
        const EStepArgs<T> A = select_model(A0, (int)(item / n_groups));
        const int b = bd.size;
        const int64_t s0 = bd.start;
        const T* __restrict__ ed = A.eta_diff + s0;
        const bool live = r0 + lane < b;
        T s = 0;
        if constexpr (kTiled) {
            const U* __restrict__ base = ld + bd.ld_off;
            const int np = (b + kPanel - 1) / kPanel;
            for (int ct = r0 / kPanel; ct < np; ++ct) {
                const int c = ct * kPanel + lane;
                const T e = c < b ? ed[c] : (T)0;
                if (__ballot(e != (T)0) == 0) continue;            // all-zero eta_diff: every term is fma(R, 0, s) == s
                __builtin_amdgcn_wave_barrier();
                edl[lane] = e;
                __builtin_amdgcn_wave_barrier();
                H h0, h1;
                const U* __restrict__ col0 = base + ct * kPanel;
                h0.load_co(col0, bd.stride, r0, b, lane);
                h1.load_co(col0 + kPanel / 2, bd.stride, r0, b, lane);
                const bool diag = ct == r0 / kPanel;              // the tile that holds the rows' own diagonal (wave-uniform)
                auto accumulate = [&](const H& h, int c0, auto masked) {
                    constexpr bool MASK = decltype(masked)::value;
#pragma unroll
                    for (int i = 0; i < H::N; ++i) {
                        const double2* __restrict__ ep = reinterpret_cast<const double2*>(edl + c0 + H::C * i);
#pragma unroll
                        for (int x = 0; x < H::C; x += 2) {
                            const double2 ee = ep[x >> 1];
                            const int cc = c0 + H::C * i + x;     // column inside the tile; this lane's row sits at `lane`
                            const T t0 = __builtin_fma(raw_elem_f64<U, H::C>(h.v[i], x), ee.x, s);
                            s = (MASK && cc <= lane) ? s : t0;
                            const T t1 = __builtin_fma(raw_elem_f64<U, H::C>(h.v[i], x + 1), ee.y, s);
                            s = (MASK && cc + 1 <= lane) ? s : t1;
                        }
                    }
                };
                // (one tile in np carries the mask: a uniform branch, the other tiles keep the plain fma chain)
                h0.to_rows(tbuf, lane);
                if (diag) accumulate(h0, 0, std::true_type{}); else accumulate(h0, 0, std::false_type{});
                h1.to_rows(tbuf, lane);
                if (diag) accumulate(h1, kPanel / 2, std::true_type{}); else accumulate(h1, kPanel / 2, std::false_type{});
            }
        } else {
            // row r0 + lane: columns [ws, we) at ld[base + c]
            int ws = 0, we = 0;
            int64_t base = 0;
            if (live) {
                const int jj = r0 + lane;
                if (DENSE) {
                    ws = jj + 1; we = b; base = bd.ld_off + (int64_t)jj * bd.stride;
                } else {
                    const int64_t j = s0 + jj;
                    ws = A.lb[j] - (int)s0; we = ws + A.rowlen[j]; base = A.rowstart[j] - ws;
                }
            }
            // (wave-uniform column loop over the union of the rows' windows: eta_diff is one scalar load per column)
            int cmin = we > ws ? ws : b, cmax = we > ws ? we : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { cmin = min(cmin, __shfl_xor(cmin, o)); cmax = max(cmax, __shfl_xor(cmax, o)); }
            for (int c = cmin; c < cmax; ++c) {
                const T e = ed[c];
                if (c >= ws && c < we) s = __builtin_fma(static_cast<T>(ld[base + c]), e, s);
            }
        }
        if (live) A.q[s0 + r0 + lane] += A.dq * s;                 // e_step.hpp:335
    }
}

}  // namespace viprs
