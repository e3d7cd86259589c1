// Internal host-side declarations shared by the translation units of libviprs_hip.so:
// plan / state objects, error reporting, launcher entry points of the kernel families.
// (The C ABI itself is include/viprs_hip.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/viprs_hip.h"
#include "dev_buf.h"
#include "kernels_common.h"
#include "planner.h"
#include "sweep_route.h"

namespace viprs {

int fail(int code, const std::string& msg);      // records the thread's error message, returns `code`

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return ::viprs::fail(VIPRS_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

inline size_t ld_elem_size(int ld_dtype) {
    switch (ld_dtype) {
        case VIPRS_LD_I8: return 1;
        case VIPRS_LD_I16: return 2;
        case VIPRS_LD_I32: return 4;
        case VIPRS_LD_I64: return 8;
        case VIPRS_LD_F32: return 4;
        case VIPRS_LD_F64: return 8;
        default: return 0;
    }
}
inline size_t float_size(int t) { return t == VIPRS_F32 ? 4 : (t == VIPRS_F64 ? 8 : 0); }

// workgroup-size classes of the panel kernel (waves per workgroup; wave 0 is the chain)
// Every class uses 4-wave workgroups (1 chain + 3 updaters) so that a team member needs exactly
// the same CU resources as a small-block workgroup; larger blocks get more CUs, not bigger groups.
struct SchedConfig {
    int large_block = 2304, medium_block = 1600;   // VIPRS_LARGE_BLOCK / VIPRS_MEDIUM_BLOCK
    int class_team[3] = {8, 4, 1};                 // workgroups (CUs) sharing one block of the class (0/1: teams)
    // mixture: the same team sizes (rounds 1-2 ran teams of 4 / single workgroups -- every member replicates the chain,
    // whose step is ~2.5x the spike-and-slab one; re-measured at the end of round 3, cfg3: K = 4 1.273 -> 1.230 ms
    // symmetric, 1.40 -> 1.36 upper; K = 10 2.11 -> 2.08, K = 20 2.91 -> 2.88)
    int class_team_mix[3] = {8, 4, 1};
    bool team_env = false;                         // VIPRS_TEAM0/1 given: they apply to every model
    // small-block queue: every `bottom_mod`-th workgroup pulls from the SMALL end of the size-sorted queue (0 = off)
    int bottom_mod = 0;                            // VIPRS_BOTTOM_MOD
};
SchedConfig& sched_config();                       // process-wide, read from the environment at plan creation
constexpr int kClassWaves[3] = {4, 4, 4};
constexpr int kPlanCounters = 32;                  // work-queue heads of a plan (d_counters), zeroed by every sweep's prologue

struct DevEvent {
    hipEvent_t e = nullptr;
    ~DevEvent() { if (e) (void)hipEventDestroy(e); }
};

// The event pair that brackets a feature's kernels on a stream (the sweeps' timing ring never sees them).
struct EventBracket {
    DevEvent ev[2];                                // created by the first start()
    bool timed = false;
    int start(hipStream_t s) {
        for (auto& e : ev)
            if (!e.e) HIP_TRY(hipEventCreate(&e.e));
        HIP_TRY(hipEventRecord(ev[0].e, s));
        return VIPRS_OK;
    }
    int stop(hipStream_t s) {
        HIP_TRY(hipEventRecord(ev[1].e, s));
        timed = true;
        return VIPRS_OK;
    }
    // ms between the last start() and stop(); `nothing`: the error message when nothing has been timed yet
    int elapsed(int device, double* ms, const char* nothing) {
        if (!timed) return fail(VIPRS_EINVAL, nothing);
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipEventSynchronize(ev[1].e));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[0].e, ev[1].e));
        *ms = (double)t;
        return VIPRS_OK;
    }
};

double host_clock_ms();                            // abi_plan.hip

// The timing record of a plan's sweeps (viprs_plan_last_kernel_ms, viprs_plan_timing_history): a ring of the last kRing
// sweeps.  Per sweep four HIP events {sweep start, sweep end, dense start, dense end}, recorded on the stream the kernels
// are launched on, and the host clock (ms) at the record of the dense start event and behind the dense end event's
// (which = 2).  The route of the sweep (sweep_route.h) says which of the events it records and who records the start.
struct SweepTiming {
    static constexpr int kRing = 256;
    struct Slot {
        DevEvent ev[4];
        bool whole = false;                        // ev[0] .. ev[1] were recorded; otherwise ev[2] .. ev[3] bracket the whole sweep
        bool dense = false;                        // ev[2] .. ev[3] were recorded
        double t0 = 0.0, t1 = 0.0;
    };
    Slot ring[kRing];
    hipStream_t stream = nullptr;
    int64_t sweeps = 0;                            // sweeps recorded since the last reset
    // The start event of the sweep being enqueued is recorded by the panel / grid launcher IMMEDIATELY in front of its first
    // kernel launch (launcher_start): with an empty stream the event is reached at once, and whatever the host does between
    // the record and the launch -- occupancy query, team split, launch gate, a scheduler hiccup -- would count as kernel time
    bool armed = false;

    Slot& slot(int64_t sweep) { return ring[sweep % kRing]; }
    int create(hipStream_t s) {                    // every event up front: the launch path creates none
        stream = s;
        for (Slot& sl : ring)
            for (DevEvent& e : sl.ev) HIP_TRY(hipEventCreate(&e.e));
        return VIPRS_OK;
    }
    // the slot of the sweep being enqueued.  Its host stamps start at zero: a sweep that brackets nothing reports 0 for
    // which = 2, not what an earlier sweep left in the slot
    int open(bool whole_sweep_events, bool dense_bracketed) {
        Slot& s = slot(sweeps);
        s.whole = whole_sweep_events;
        s.dense = dense_bracketed;
        s.t0 = s.t1 = 0.0;
        armed = false;
        if (s.whole) HIP_TRY(hipEventRecord(s.ev[0].e, stream));
        return VIPRS_OK;
    }
    void arm() { armed = true; }                   // the launcher records the start event
    int start() {                                  // the caller records it, in front of the dense launcher
        armed = false;
        slot(sweeps).t0 = host_clock_ms();
        HIP_TRY(hipEventRecord(slot(sweeps).ev[2].e, stream));
        return VIPRS_OK;
    }
    int launcher_start() { return armed ? start() : VIPRS_OK; }      // (first launch of the sweep only: disarmed after)
    int stop() {
        HIP_TRY(hipEventRecord(slot(sweeps).ev[3].e, stream));
        slot(sweeps).t1 = host_clock_ms();
        return VIPRS_OK;
    }
    // behind the dense launcher: the end of its own bracket, where the sweep has one beside the whole sweep's
    int dense_done() { return slot(sweeps).whole && slot(sweeps).dense ? stop() : VIPRS_OK; }
    // behind the last launcher: ev[2] .. ev[3] close here when they stand for the whole sweep
    int close() {
        if (slot(sweeps).whole) HIP_TRY(hipEventRecord(slot(sweeps).ev[1].e, stream));
        else { const int rc = stop(); if (rc != VIPRS_OK) return rc; }
        sweeps++;
        return VIPRS_OK;
    }
    void abandon() { armed = false; }              // a launcher failed: the sweep is not counted
    void reset() { sweeps = 0; armed = false; }
    // which: 0 = all kernels of the sweep, 1 = the dense bracket, 2 = host time inside the dense bracket
    int elapsed(int64_t sweep, int which, double* ms) {
        Slot& s = slot(sweep);
        *ms = 0.0;
        if (which == 2) { *ms = std::max(0.0, s.t1 - s.t0); return VIPRS_OK; }
        const bool bracket = which == 1 || !s.whole;
        if (bracket && !s.dense) return VIPRS_OK;
        float t = 0.f;
        HIP_TRY(hipEventSynchronize(s.ev[bracket ? 3 : 1].e));
        HIP_TRY(hipEventElapsedTime(&t, s.ev[bracket ? 2 : 0].e, s.ev[bracket ? 3 : 1].e));
        *ms = t;
        return VIPRS_OK;
    }
};

struct RidgeBlock;                                 // ridge.h: start and size of an LD block

// ridge solve (abi_ridge.hip, ridge.h): the workspace of a plan, allocated by its first solve and reused by the later ones
struct RidgeWork {
    bool built = false;
    DevBuf<char> d_rec;                            // RidgeRec per LD block, SNP order
    DevBuf<int32_t> d_live;                        // blocks still running
    size_t vec_bytes = 0;                          // capacity of each vector below
    DevBuf<char> d_vec[9];                         // v, R v, three residual and three direction vectors in rotation, x
    DevBuf<char> d_shift;
    EventBracket time;
    int iterations = 0;                            // iterations the last solve launched
};

// extremal eigenvalues (abi_spectrum.hip, lanczos.h): the workspace of a plan, allocated by its first call and reused
struct SpectrumWork {
    bool built = false;
    DevBuf<double> d_beta;                         // beta_k of the iteration to come, per block
    DevBuf<int32_t> d_status, d_iters;             // per block
    DevBuf<int32_t> d_live;                        // blocks still running
    size_t vec_bytes = 0;                          // capacity of each vector below
    DevBuf<char> d_vec[3];                         // v, v_prev (w while a step runs), A v
    size_t coef_cap = 0;                           // capacity of each array below (doubles)
    DevBuf<double> d_alpha, d_betas;               // alpha_k / beta_{k+1} at [block * max_iter + k - 1]
    EventBracket time;
    int iterations = 0;                            // iterations the last call launched
    double host_ms = 0.0;                          // host time of its checks (downloads + tridiagonal eigenproblems)
};

// SuSiE fine-mapping (abi_susie.hip, susie.h): the workspace of a plan, allocated by its first call and reused
struct SusieWork {
    DevBuf<char> d_rec;                            // SusieRec per LD block, SNP order
    DevBuf<int32_t> d_live;                        // blocks still running
    DevBuf<char> d_alpha, d_mu, d_rb;              // (m, L) each, state precision
    DevBuf<char> d_bbar, d_y;                      // (m,): the product's input and result
    DevBuf<double> d_w, d_z, d_log_pi;             // (m,)
    DevBuf<double> d_v, d_v0, d_post_var;          // (n_blocks, L)
    EventBracket time, time_step;                  // the whole call; the step kernel of effect L - 1 of iteration 1
    int steps = 0;                                 // step kernels the last call launched
};

}  // namespace viprs

struct viprs_state;
struct viprs_comm;                                  // comm.hip
struct viprs_plan {
    int64_t m = 0;
    int64_t nnz = 0;
    int low_memory = 0;
    int mirror = 0;                  // upper-triangular form: the dense blocks currently hold the upper triangle mirrored into the lower one
                                     // (what the panel and grid kernels sweep; the float64 kernels read it with a zero lower triangle)
    int ld_dtype = 0;
    int device = 0;
    int n_cu = 0;
    int math_mode = VIPRS_MATH_EXACT;
    int math_used = 0;                      // kernels of the last sweep: bit 0 = exact arithmetic ran, bit 1 = fast arithmetic ran
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;             // float64 state: the big-block class of estep_tile.h runs beside the rest
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<viprs::Block> blocks;              // SNP order
    std::vector<viprs::BlockDesc> dense_h, ragged_h;  // schedule order (descending cost)
    // dense blocks are served by panel kernels of three workgroup sizes (more updater waves =
    // more row loads in flight = a larger share of HBM bandwidth for the larger blocks); class c
    // covers dense_h[class_begin[c] .. class_begin[c+1])
    int class_begin[4] = {0, 0, 0, 0};
    int team0 = 0;                          // team size of the largest class for this plan's largest block (0: the configured one)
    viprs::DevBuf<viprs::BlockDesc> d_dense, d_ragged;
    // viprs_plan_set_active_blocks: the lists above are what a sweep visits -- all blocks, or the active subset (the
    // lock-step fit of one model per chromosome drops the blocks of the chromosomes that have converged); the full lists:
    std::vector<viprs::BlockDesc> dense_all_h, ragged_all_h;
    int class_begin_all[4] = {0, 0, 0, 0};
    viprs::DevBuf<viprs::BlockDesc> d_dense_all;   // what ensure_upper_storage converts (every block, active or not)
    bool filtered = false;
    uint64_t dense_gen = 0;                        // changes of the dense list (viprs_plan_set_active_blocks): maps indexed like it follow
    viprs::DevBuf<unsigned long long> d_granules;  // team hand-off granules (one row of 64 per panel of a team block)
    int64_t n_granule_rows = 0;
    viprs::DevBuf<int32_t> d_error;
    int grid_mfma = -1;                     // batched grid E-step on the matrix cores: 1 always, 0 never (per-(block,
                                            // model) items), -1 when the plan has enough blocks to fill the CUs (VIPRS_GRID_MFMA)
    viprs::DevBuf<int32_t> d_lb;
    viprs::DevBuf<int64_t> d_ip;
    viprs::DevBuf<int32_t> d_rowlen;               // indptr[j+1] - indptr[j]
    viprs::DevBuf<int64_t> d_rowlist_dense, d_rowlist_ragged;   // float64 second pass (estep_tile.h): (block of the list) << 32 | first row, per group of 8 rows
    viprs::DevBuf<int64_t> d_rowstart_dense;       // row starts inside the repacked dense buffer (generic kernels)
    viprs::DevBuf<char> d_ld_raw;                  // kept only when ragged blocks exist
    viprs::DevBuf<char> d_ld_dense;
    int64_t dense_elems = 0;
    int max_dense = 0, max_ragged = 0;
    int max_band_panels = 0;                // ragged blocks: widest (band_left + band_right + 2), sizes the band kernel's q ring
    viprs::DevBuf<int32_t> d_counters;             // [0] dense queue head, [1] ragged queue head
    viprs::DevBuf<unsigned long long> d_skipped;   // [0] running count of the sweep in flight, [1] of the sweep kernel(s) that are done
    bool skip_count_in_place = false;              // the last sweep ran kernels that leave their count in [0] (no panel-sweep epilogue moved it)
    viprs::DevBuf<int32_t> d_arrive;               // panel sweep: arrival counters of the team (block, model) items; [last]: workgroups done
    uint32_t granule_gen = 0;                      // panel sweep launches so far (mod 2^20): generation of the hand-off tags
    // batched grid kernel, teams for the blocks beyond its resident form (launch_grid.inc): per team workgroup (block of the
    // size-sorted list, member, team size), per team block the offset of its a-vector granules
    // the split of the team budget between the two team classes (launch_panel.inc) depends on the plan and on these only
    struct TeamSplit { int64_t key[6] = {-1, -1, -1, -1, -1, -1}; int best[2] = {0, 0}; } team_split;
    bool grid_teams_built = false;
    int grid_team_blocks = 0, grid_team_wgs = 0;
    std::vector<int> grid_team_ts;                 // team size per team block (largest block first)
    viprs::DevBuf<int32_t> d_grid_team_block, d_grid_team_member, d_grid_team_size;
    viprs::DevBuf<int64_t> d_grid_team_goff;
    viprs::DevBuf<unsigned long long> d_grid_gran;
    uint32_t grid_gen = 0;
    viprs::SweepTiming timing;                     // of the E-step sweeps
    viprs_state* scratch = nullptr;         // state used by the one-shot host-buffer calls
    // LD product (abi_dot.hip, ld_dot.h): its own tables over EVERY block of the plan (the product is not filtered by
    // viprs_plan_set_active_blocks), built by the first product; its own event pair
    bool dot_built = false;
    viprs::DevBuf<viprs::BlockDesc> d_dot_blocks;  // dense_all_h, then ragged_all_h
    // work lists in the order of the plan's full block lists: (block of d_dot_blocks) << 32 | (first) row of the block; dense [k]: 1 << k rows per item
    viprs::DevBuf<int64_t> d_dot_rows_dense[3], d_dot_rows_ragged;
    viprs::DevBuf<int32_t> d_dot_first;            // upper form with windowed blocks: the first row whose entries reach row j
    viprs::DevBuf<char> d_dot_b, d_dot_y;          // staging of the host-buffer call / the results
    viprs::EventBracket time_dot;
    bool unmirrored_wanted = false;                // the last launch that asked for a storage of the upper form wanted the zero lower triangle
    // LD scores (abi_ld_score.hip, ld_score.h): the product's tables; its own staging and event pair
    viprs::DevBuf<char> d_score_a, d_score_y;
    viprs::DevBuf<double> d_score_corr;
    viprs::EventBracket time_score;
    // LD clumping (abi_clump.hip, ld_clump.h): the product's tables; its own buffers and event pair
    std::vector<int32_t> clump_block_of;           // the block of d_dot_blocks of every SNP (built by the first call)
    viprs::DevBuf<int32_t> d_clump_order;          // the order, split stably by block of d_dot_blocks
    viprs::DevBuf<int64_t> d_clump_off;            // blocks + 1 offsets of the pieces
    viprs::DevBuf<double> d_clump_thr;             // 32 thresholds on the squared stored element
    viprs::DevBuf<uint32_t> d_clump_mask;          // (m,) bit g set: the SNP is not available in column g
    viprs::DevBuf<int32_t> d_clump_index;          // (m, n_cols) results
    viprs::EventBracket time_clump;
    viprs::DevBuf<viprs::RidgeBlock> d_solver_blocks;   // start and size of every LD block, SNP order (ensure_solver_blocks)
    viprs::RidgeWork ridge;                        // viprs_plan_solve_ridge
    viprs::EventBracket time_gibbs_draws;          // the draws kernel of the Gibbs sweeps (abi_gibbs.hip)
    viprs::EventBracket time_cs_variates, time_cs_update;   // the two PRS-CS kernels (abi_cs.hip)
    viprs::EventBracket time_bayesr_draws;         // the draws kernel of the SBayesR sweeps (abi_bayesr.hip)
    viprs::SpectrumWork spectrum;                  // viprs_plan_extremal_eigenvalues
    viprs::SusieWork susie;                        // viprs_plan_susie

    ~viprs_plan();
};

struct viprs_state {
    viprs_plan* plan = nullptr;
    int device = 0;                         // (own copy: viprs_state_destroy must not read the plan -- a garbage collector may have destroyed it first)
    int float_dtype = VIPRS_F32;
    int model_kind = VIPRS_MODEL_SPIKE_SLAB;
    int width = 1;
    viprs::DevBuf<char> f[VIPRS_FIELD_COUNT];
    viprs::DevBuf<int32_t> d_active;               // grid: active model indices of the current call
    viprs::DevBuf<char> eta_out, q_out;            // team kernels' in-out staging (see kernels_common.h)
    viprs::DevBuf<double> d_n, d_var_tau, d_partials, d_sums;   // device-resident EM iteration
    viprs::DevBuf<double> d_weight;                // optional per-SNP weight of sum [0] (several chromosomes in one plan)
    viprs::DevBuf<double> d_log_var_tau0;          // mixture: the log var_tau of the initial state (the reference's ELBO never refreshes it)
    std::vector<double> col_prep;                  // grid: (one_plus_lambda, sigma_eps, tau_beta) of every column's last prep (3 x width; NaN: none yet)
    // viprs_state_set_groups: contiguous SNP ranges with their own hyper-parameters and their own sums (one model per chromosome)
    int n_groups = 0;
    std::vector<int64_t> group_start;              // n_groups + 1 entries
    // grid state with groups: one set of hyper-parameters per (group, column) pair
    std::vector<double> pair_prep;                 // (one_plus_lambda, sigma_eps, tau_beta) of every pair's last prep (3 x n_groups x width; NaN: none yet)
    std::vector<uint8_t> group_cols_h;             // viprs_state_set_group_columns: n_groups x width mask (empty: none)
    viprs::DevBuf<uint8_t> d_group_cols;
    viprs::DevBuf<int32_t> d_blk_group;            // group of every block of the plan's dense list (indexed as d_dense)
    uint64_t blk_group_gen = ~0ull;                // the plan's dense_gen d_blk_group was built for
    viprs::DevBuf<int32_t> d_group_lists;          // per launch of 32 active columns and group: its columns under the mask (kGroupListStride ints)
    // row tables of the batched prep / sums calls (abi_state.hip): room for rows_cap rows each, staged through h_rows
    // (pinned: rows_cap prep rows, then rows_cap sums rows)
    viprs::DevBuf<char> d_prep_rows;
    viprs::DevBuf<char> d_sum_rows;
    char* h_rows = nullptr;
    size_t rows_cap = 0;
    hipEvent_t ev_prep = nullptr;                  // the last batched prep launch (it reads d_prep_rows)
    size_t h_sums_cap = 0;
    double* h_sums = nullptr;               // pinned landing buffer of the device sums
    size_t sums_total = 0;                  // doubles of the reduction in flight (or of the zeros `end` returns: sums_empty)
    bool sums_pending = false, sums_empty = false;
    viprs_comm* comm = nullptr;             // viprs_state_set_comm: the sums are all-rank sums (one all-gather per reduction)
    // LDpred2 Gibbs sweeps (abi_gibbs.hip), allocated by the first Gibbs call: 2 x (m, G) float32 -- U, then noise -- and the
    // (m, G) float64 sum of the Rao-Blackwellised means
    viprs::DevBuf<float> d_gibbs_draws;
    viprs::DevBuf<double> d_gibbs_mean;
    // PRS-CS (abi_cs.hip), allocated by the first cs call: the VIPRS_CS_BUFFER_COUNT (m, G) float32 buffers of
    // viprs_cs_buffer in ONE allocation, in the order of the enum; the (column, sigma2, phi) rows of the call in flight
    viprs::DevBuf<float> d_cs;
    viprs::DevBuf<double> d_cs_rows;
    // SBayesR (abi_bayesr.hip), allocated by the first SBayesR call: 3 m four-byte words in ONE allocation -- U, z (float32),
    // then k* (int32); the two (m,) float64 accumulators, mean_sum then pip_sum, created on first use; partials and results of
    // viprs_state_bayesr_sums
    viprs::DevBuf<float> d_bayesr;
    viprs::DevBuf<double> d_bayesr_acc;
    viprs::DevBuf<double> d_bayesr_sums;
    ~viprs_state() {
        if (h_sums) (void)hipHostFree(h_sums);
        if (h_rows) (void)hipHostFree(h_rows);
        if (ev_prep) (void)hipEventDestroy(ev_prep);
    }
    size_t field_elems(int field) const {
        const size_t m = (size_t)plan->m;
        switch (field) {
            case VIPRS_FIELD_STD_BETA: return m;
            case VIPRS_FIELD_LOG_NULL_PI: return model_kind == VIPRS_MODEL_MIXTURE ? m : 0;
            case VIPRS_FIELD_ETA: case VIPRS_FIELD_Q: case VIPRS_FIELD_ETA_DIFF:
                return model_kind == VIPRS_MODEL_GRID ? m * width : m;
            default: return m * width;
        }
    }
};

namespace viprs {

// abi_plan.hip: a plan whose LD rows (the caller's row-concatenated layout, `ip64[m]` elements) are written by `fill`
// into device memory instead of being uploaded from the host (synth.hip)
int plan_create_generated(viprs_plan** out, int64_t m, const int32_t* lb, const std::vector<int64_t>& ip64, int ld_dtype,
                          int low_memory, int device, const std::function<int(void*)>& fill);

// Launches whose workgroups wait for each other (team hand-offs: the panel sweep, the batched grid kernel) size their grid to
// the workgroups the WHOLE device can hold at once.  Two such launches in flight on one device (several plans of one
// process on their own streams: unmerged chromosomes, VIPRSGrid's per-plan sweeps) would each find only part of the device
// and could leave a team member undispatched while its peers spin.  `team_launch_gate` orders them: the stream of the plan
// waits for the previous gated launch on this device, `team_launch_done` records this one.  (Other PROCESSES on the
// same device cannot be ordered from here: the bounded spins report VIPRS_EDEVICE instead of hanging.)
int ensure_upper_storage(viprs_plan* P, bool mirrored);
int team_launch_gate(viprs_plan* P);
int team_launch_done(viprs_plan* P);

// after a synchronisation point: did a team hand-off give up (bounded spin)?
int check_device_error(viprs_plan* P);

// abi_dot.hip: what every call over the plan's LD rows does first.  The tables of the product (every block of the plan, one
// work item per row) are built once per plan; an upper-form plan nobody has swept yet is mirrored once
int prepare_ld_rows(viprs_plan* P);
// abi_ridge.hip: the block table of the lock-step solvers (P->d_solver_blocks), built once per plan
int ensure_solver_blocks(viprs_plan* P);
// abi_dot.hip: the kernels of one LD product on the plan's stream (device pointers, (m, n_cols) column-major), between the
// product's own two events; nothing is synchronised
int enqueue_dot(viprs_plan* P, int float_dtype, int n_cols, const void* dB, void* dY, double dq_scale, int include_diagonal);

// comm.hip: all-gather + rank-ordered reduction of the device vector (n doubles, in place) on `stream`; the last
// element of every `group` is a maximum, the others are sums
int comm_reduce_on_stream(viprs_comm* C, double* d_vec, int n, int group, hipStream_t stream);

// ---- kernel families (one translation unit per family and LD element type) ------------------------
// (the families and their model constants: sweep_route.h)

// generic kernels over one block list: `dense` = the repacked dense blocks, otherwise the ragged blocks
template <typename T, typename U> int launch_generic(viprs_plan* P, EStepArgs<T> A, int model, bool dense);
// float64 state: the panel-walking kernels (estep_tile.h) over one block list; falls back to launch_generic for the
// mixture and for blocks whose q does not fit the LDS
template <typename U> int launch_tile_f64(viprs_plan* P, EStepArgs<double> A, int model, bool dense);
// panel kernels of the three size classes on their own streams, joined into the plan's stream
template <typename U> int launch_panel(viprs_plan* P, EStepArgs<float> A, int model);
// band kernel for the windowed components
template <typename U> int launch_band(viprs_plan* P, EStepArgs<float> A, int model);
int band_ring_panels(const viprs_plan* P);
// The two launchers behind their kernel selection (launch_panel.inc, launch_band.inc): everything but the choice of the
// instantiation, which the caller hands in.  The elastic-net policy (panel_enet.h) is instantiated in translation units of
// its own -- panel_enet_*.hip, band_enet_*.hip -- and launched through them: launch_panel_enet / launch_band_enet.
#ifdef PANEL_NW
constexpr int kPanelWaves = PANEL_NW;              // (experiments: kernels_common.h)
#else
constexpr int kPanelWaves = kClassWaves[0];
#endif
using BandKernelFn = void (*)(EStepArgs<float>, int);
template <typename U> int launch_panel_kernel(viprs_plan* P, EStepArgs<float> A, int model, const void* kfn, int nw, int math_bit);
template <typename U> int launch_band_kernel(viprs_plan* P, EStepArgs<float> A, BandKernelFn kfn, int math_bit);
template <typename U> int launch_panel_enet(viprs_plan* P, EStepArgs<float> A);
template <typename U> int launch_band_enet(viprs_plan* P, EStepArgs<float> A);
// the LDpred2 Gibbs policy (panel_gibbs.h) likewise: panel_gibbs_*.hip, band_gibbs_*.hip
template <typename U> int launch_panel_gibbs(viprs_plan* P, EStepArgs<float> A);
template <typename U> int launch_band_gibbs(viprs_plan* P, EStepArgs<float> A);
// abi_gibbs.hip: the state's draw buffers (U, then noise: the two halves of ONE allocation, created by the first Gibbs call),
// the draws kernel on the plan's stream between the plan's own two events (device list of columns; nothing is synchronised),
// and what a Gibbs sweep hands the policy in the log_null_pi slot of its arguments (panel_gibbs.h): the distance in bytes
// from the state's mu_mult buffer to U
int gibbs_ensure_draws(viprs_state* S);
int gibbs_enqueue_draws(viprs_state* S, uint64_t seed, uint64_t draw_index, const int32_t* d_active, int n_active);
const float* gibbs_draws_slot(const viprs_state* S);
// the SBayesR policy (panel_bayesr.h): panel_bayesr_*.hip, band_bayesr_*.hip
template <typename U> int launch_panel_bayesr(viprs_plan* P, EStepArgs<float> A);
template <typename U> int launch_band_bayesr(viprs_plan* P, EStepArgs<float> A);
// abi_bayesr.hip: what every SBayesR entry point refuses (`what` names the call in the message), the state's draw allocation
// (U | z | k*, zeroed, created by the first SBayesR call) and the draws kernel on the plan's stream between the plan's own two
// events (nothing is synchronised).  A sweep hands the policy the allocation in the `active` slot of its arguments.
int bayesr_state_check(const viprs_state* S, const char* what);
int bayesr_ensure_draws(viprs_state* S);
int bayesr_enqueue_draws(viprs_state* S, uint64_t seed, uint64_t draw_index);
// abi_cs.hip: what every PRS-CS entry point refuses (`what` names the call in the message), and the state's cs buffers
// (psi = 1, the rest zero), created by the first call that needs them
int cs_state_check(const viprs_state* S, const char* what);
int cs_ensure_buffers(viprs_state* S);
// batched grid E-step on the matrix cores
template <typename U> int launch_grid_mfma(viprs_plan* P, EStepArgs<float> A);
// LD product Y = dq_scale (R - diag) B (+ B) over every block of the plan (ld_dot.h); device pointers, (m, n_cols) column-major
template <typename U> int launch_ld_dot(viprs_plan* P, int float_dtype, int n_cols, const void* dB, void* dY, double dq_scale,
                                        int include_diagonal);
// LD scores over every block of the plan (ld_score.h); device pointers, dA null: unit weights, dCorr null: no correction
template <typename U> int launch_ld_score(viprs_plan* P, int float_dtype, int n_cols, const void* dA, const double* dCorr,
                                          void* dY, double dq_scale);
// greedy clumping over every block of the plan (ld_clump.h): one workgroup per block of d_dot_blocks; the order pieces, the
// thresholds, the masks and the results are the plan's d_clump_* buffers
template <typename U> int launch_ld_clump(viprs_plan* P, int n_cols);

}  // namespace viprs
