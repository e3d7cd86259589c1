// Panel kernels (estep_panel.h) for one LD element type: included by panel_f32.hip / panel_i8.hip /
// panel_i16.hip with PANEL_U defined.
#include "internal.h"
#include "estep_panel.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

// The dense blocks of a plan are swept by ONE launch of estep_sweep_kernel: team workgroups for the two classes of
// large blocks first, small-block workers behind them (estep_panel.h); the second pass of the upper-triangular form
// (update_q_factor, e_step.hpp:331-337) runs inside the sweep, over the mirrored blocks (kFormMirror), and so does the
// bookkeeping that used to be two more launches (the prologue's zeroing, the commit of the team blocks' staged outputs).
// `kfn`: the estep_sweep_kernel instantiation of the model's policy for this form, built for `nw` waves per workgroup and
// panel_cols<U>() columns per updater lane (the caller selects it: launch_panel below; launch_panel_enet.inc for the
// policies that live in translation units of their own); `math_bit`: what it adds to viprs_plan_last_math_modes.
template <typename U>
int launch_panel_kernel(viprs_plan* P, EStepArgs<float> A, int model, const void* kfn, int nw, int math_bit) {
    constexpr int CPL = panel_cols<U>();
    const bool upper = P->low_memory != 0;
    // the arithmetic of the upper form runs over mirrored storage (kFormMirror): strips as in the symmetric form
    const bool mirror = upper;
    if (upper) { const int rc = ensure_upper_storage(P, true); if (rc != VIPRS_OK) return rc; }
    const int n_models = std::max(1, A.n_active);
    const int* team_of = ((model == kPanelMixture || model == kPanelMixtureWide) && !sched_config().team_env) ? sched_config().class_team_mix
                                                                             : sched_config().class_team;
    P->math_used |= math_bit;

    // hand-off granules (one set per model of a grid launch) and arrival counters of the team items; a launch generation
    // in the granule tags replaces their zeroing (20 bits: the buffer is cleared once every 2^20 launches)
    const int n_team_blocks = P->class_begin[2];
    const int64_t ng = P->n_granule_rows * kPanel * (int64_t)n_models;
    if (P->d_granules.n < (size_t)ng) {
        HIP_TRY(hipStreamSynchronize(P->stream));
        HIP_TRY(P->d_granules.alloc((size_t)ng));
        HIP_TRY(hipMemsetAsync(P->d_granules.p, 0, sizeof(unsigned long long) * (size_t)ng, P->stream));   // (stream order: in front of the sweep)
    }
    const size_t n_arrive = (size_t)n_team_blocks * (size_t)n_models + 1;      // [last]: workgroups that have finished
    if (P->d_arrive.n < n_arrive) {
        HIP_TRY(hipStreamSynchronize(P->stream));
        HIP_TRY(P->d_arrive.alloc(n_arrive));
        HIP_TRY(hipMemsetAsync(P->d_arrive.p, 0, sizeof(int32_t) * n_arrive, P->stream));
    }
    P->granule_gen = (P->granule_gen + 1) & 0xFFFFFu;
    if (P->granule_gen == 0) {
        if (P->d_granules.n) HIP_TRY(hipMemsetAsync(P->d_granules.p, 0, sizeof(unsigned long long) * P->d_granules.n, P->stream));
        P->granule_gen = 1;
    }
    A.granules = P->d_granules.p;
    A.tag_base = P->granule_gen << 12;                      // + panel + 1 (blocks of up to 4 094 panels)

    SweepArgs S{};
    S.done = P->d_arrive.p + (n_arrive - 1);
    S.skipped_last = P->d_skipped.p + 1;
    size_t shmem = 0;
    for (int c = 0; c < 3; ++c) {
        EStepArgs<float>& C = S.cls[c];
        C = A;
        const int begin = P->class_begin[c], end = P->class_begin[c + 1];
        C.blocks = P->d_dense.p + begin;
        C.n_blocks = end - begin;
        if (A.blk_group) C.blk_group = A.blk_group + begin;       // (indexed as `blocks`)
        C.counter = c < 2 ? P->d_counters.p + 4 + c : P->d_counters.p + 16;
        // arrival counters: the items of class 0, then those of class 1
        C.arrive = P->d_arrive.p + (c == 1 ? (size_t)(P->class_begin[1] - P->class_begin[0]) * (size_t)n_models : 0);
        C.bottom_mod = 0;
        C.team_size = c < 2 ? team_of[c] : 1;
        if (c == 0 && P->team0 > 0 && team_of == sched_config().class_team) C.team_size = P->team0;
        if (c == 0 && team_of == sched_config().class_team_mix) {
            // a populous large class: more, smaller teams (as abi_plan.hip does for P->team0)
            const int64_t room = (int64_t)P->n_cu * 2 * 5 / 8;
            while (C.team_size > 4 && (int64_t)(end - begin) * n_models * C.team_size > room) C.team_size -= 4;
        }
        C.n_teams = 0;
        S.qcap[c] = 0;
        if (end > begin) {
            const int max_b = P->dense_h[begin].size;      // descending order
            // (the layout the kernel carves: PanelLds, kernels_common.h)
            auto lds_bytes = [&](int qcap) {
                return (size_t)PanelLds(qcap, model == kPanelMixture, mirror).total_floats() * sizeof(float);
            };
            for (;;) {
                S.qcap[c] = (max_b + kPanel - 1) / kPanel * kPanel + kStrip;
                if (c < 2) {
                    // a team member keeps only its own strips (estep_panel.h): strips of the largest block / team size, rounded up
                    // (team strips: estep_panel.h -- narrower for the large teams of class 0 in the upper-triangular form,
                    //  lane-per-SNP models only)
                    const bool narrow = upper && sizeof(U) < 4 && c == 0 && C.team_size >= 8 && model != kPanelMixture && model != kPanelMixtureWide;
                    if (c == 0) S.narrow0 = narrow ? 1 : 0;
                    const int kSW = kPanel * (narrow ? panel_team_cols<U>() : CPL);
                    const int n_strips = ((max_b + kPanel - 1) / kPanel * kPanel + kSW - 1) / kSW;
                    S.qcap[c] = (n_strips + C.team_size - 1) / C.team_size * kSW + kStrip;
                }
                // A team class whose largest block does not fit the 160 KB of a CU at this team size (kMaxDenseBlock in
                // abi_plan.hip budgets the upper form WITHOUT the off-diagonal tile that integer LD stages there too;
                // VIPRS_TEAM0=1 or unusual class limits get there): more members, each holding fewer strips
                if (c < 2 && lds_bytes(S.qcap[c]) > 160 * 1024 && C.team_size < 16) { ++C.team_size; continue; }
                break;
            }
            shmem = std::max(shmem, lds_bytes(S.qcap[c]));
        }
    }
    if (shmem == 0) return P->timing.launcher_start();
    if (shmem > 160 * 1024) return fail(VIPRS_EUNSUPPORTED, "LD block too large for the LDS-resident panel kernel");
    if (shmem > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, nw * 64, shmem));
    per_cu = std::max(1, per_cu);
    if (const char* f = getenv("VIPRS_MAX_WG_PER_CU")) per_cu = std::max(1, std::min(per_cu, atoi(f)));   // experiments
    const int capacity = P->n_cu * per_cu;                  // every workgroup of the grid is resident at once

    // Team classes: teams of TS workgroups, blocks assigned statically (team t: blocks t, t + n_teams, ...).  The teams
    // may take at most 5/8 of the grid when there are small blocks too (the rest works on the small-block queue from
    // the start; team workgroups join it when their team is done).
    const int64_t n_small = (int64_t)S.cls[2].n_blocks * n_models;
    const int team_budget = n_small > 0 ? capacity * 5 / 8 : capacity;
    // The budget is split between the two team classes so that the busier class finishes as early as possible: teams
    // take their class's items round-robin (team 0: items 0, n, 2n, ... of the size-sorted list -- the longest share), a
    // block keeps its team for max(chain, its bytes through TS members).  Handing the budget out first come, first served
    // starves the medium class as soon as the large one is populous -- 28 blocks >= 1 792 SNPs in teams of 12 left 2 teams
    // for 70 medium blocks: an 8 ms sweep instead of 0.8 (tools/sched_sweep.py) -- and could leave it no team at all.
    int team_wgs = 0;
    {
        const double es = (double)sizeof(U);
        auto class_time = [&](int c, int n_teams) {            // seconds until team 0 of class c is done
            const EStepArgs<float>& C = S.cls[c];
            const int64_t n_items = (int64_t)C.n_blocks * n_models;
            double t = 0.0;
            for (int64_t i = 0; i < n_items; i += n_teams) {
                const double sz = (double)P->dense_h[(size_t)(P->class_begin[c] + i / n_models)].size;
                t += std::max(sz * 135e-9, sz * sz * es / (C.team_size * 16e9));
            }
            return t;
        };
        const int64_t items[2] = {(int64_t)S.cls[0].n_blocks * n_models, (int64_t)S.cls[1].n_blocks * n_models};
        const int TS0 = S.cls[0].team_size, TS1 = S.cls[1].team_size;
        int best[2] = {0, 0};
        const int64_t key[6] = {items[0], items[1], TS0, TS1, team_budget, (int64_t)sizeof(U)};
        if (std::equal(key, key + 6, P->team_split.key)) {      // same search as at the last sweep: its result
            best[0] = P->team_split.best[0];
            best[1] = P->team_split.best[1];
        } else if (items[0] > 0 && items[1] > 0) {
            double best_t = 1e30;
            const int max0 = (int)std::min<int64_t>(items[0], std::max(1, (team_budget - TS1) / TS0));
            for (int n0 = 1; n0 <= max0; ++n0) {
                const int n1 = (int)std::min<int64_t>(items[1], std::max(1, (team_budget - n0 * TS0) / TS1));
                const double t = std::max(class_time(0, n0), class_time(1, n1));
                if (t < best_t * (1.0 - 1e-9)) { best_t = t; best[0] = n0; best[1] = n1; }
            }
        } else if (items[0] > 0) {
            best[0] = (int)std::min<int64_t>(items[0], std::max(1, team_budget / TS0));
        } else if (items[1] > 0) {
            best[1] = (int)std::min<int64_t>(items[1], std::max(1, team_budget / TS1));
        }
        std::copy(key, key + 6, P->team_split.key);
        P->team_split.best[0] = best[0];
        P->team_split.best[1] = best[1];
        for (int c = 0; c < 2; ++c) {
            EStepArgs<float>& C = S.cls[c];
            C.n_teams = best[c];
            S.n_wg[c] = C.n_teams * C.team_size;
            team_wgs += S.n_wg[c];
        }
    }
    if (team_wgs > capacity) return fail(VIPRS_EUNSUPPORTED, "team size exceeds the resident workgroups of the device");
    int grid = (int)std::min<int64_t>(capacity, (int64_t)team_wgs + n_small);
    grid = std::max(grid, team_wgs);
    // small-block queue: every bottom_mod-th workgroup takes from the small end of the size-sorted list
    if (n_small >= 4 * (int64_t)P->n_cu) S.cls[2].bottom_mod = sched_config().bottom_mod;

    void* params[] = {(void*)&S};
    if (team_wgs > 0) { const int rc = team_launch_gate(P); if (rc != VIPRS_OK) return rc; }
    { const int rc = P->timing.launcher_start(); if (rc != VIPRS_OK) return rc; }      // (the sweep's start event: adjacent to the launch)
    HIP_TRY(hipLaunchKernel(kfn, dim3(grid), dim3(nw * 64), params, shmem, P->stream));
    if (team_wgs > 0) { const int rc = team_launch_done(P); if (rc != VIPRS_OK) return rc; }
    // (no commit launch: the member of a team that finishes a block last copies its staged eta / q into place)
    return VIPRS_OK;
}

// Waves per workgroup (1 chain + NW - 1 updaters): 4 for every LD type and form.  (Rounds 1-2 ran int8 LD in the symmetric
// form on 2-wave workgroups, 4 per CU -- twice the chains in flight, 0.60 -> 0.55 ms then; with the chain's tiles in LDS
// and the launch bookkeeping folded into the sweep it is the other way round: 0.559 -> 0.539 ms kernel, 0.59 -> 0.55 ms
// per step with 4 waves, tools/ab_bench.py.  -DPANEL_NW=n builds the other variant.)
template <typename U>
int launch_panel(viprs_plan* P, EStepArgs<float> A, int model) {
    constexpr int NW = kPanelWaves, CPL = panel_cols<U>();
    const bool exact = P->math_mode == VIPRS_MATH_EXACT;
    const bool upper = P->low_memory != 0;
    const void* kfn = nullptr;
#define PK(MODEL) (upper ? (const void*)estep_sweep_kernel<U, MODEL, kFormMirror, NW, CPL>       \
                          : (const void*)estep_sweep_kernel<U, MODEL, kFormSym, NW, CPL>)
    // math_mode = fast: spike-and-slab, grid columns and mixtures of up to 8 components (wider mixtures stay exact)
    if (model == kPanelGridColumn) kfn = exact ? PK(GridColumnModel<true>) : PK(GridColumnModel<false>);
    else if (model == kPanelMixture) kfn = exact ? PK(MixtureModel<true>) : PK(MixtureModel<false>);
    else if (model == kPanelMixtureWide) kfn = A.width <= 15 ? PK(MixtureWideModel<15>) : PK(MixtureWideModel<31>);
    else kfn = exact ? PK(SpikeSlabModel<true>) : PK(SpikeSlabModel<false>);
#undef PK
    // (what this launch computes in: math_mode = fast has no wide-mixture instantiation -- viprs_plan_last_math_modes)
    return launch_panel_kernel<U>(P, A, model, kfn, NW, (exact || model == kPanelMixtureWide) ? 1 : 2);
}

template int launch_panel_kernel<PANEL_U>(viprs_plan*, EStepArgs<float>, int, const void*, int, int);
template int launch_panel<PANEL_U>(viprs_plan*, EStepArgs<float>, int);

#if defined(VIPRS_SWEEP_TRACE)
// profiling builds: hand the trace of the last sweep(s) to the host and reset it
#define PANEL_TRACE_FN2(tag) viprs_debug_sweep_trace_##tag
#define PANEL_TRACE_FN(tag) PANEL_TRACE_FN2(tag)
extern "C" int PANEL_TRACE_FN(PANEL_TAG)(unsigned long long* out, int capacity) {
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_sweep_trace_n), sizeof(n)) != hipSuccess) return -1;
    n = std::min<unsigned>(n, std::min<unsigned>(1u << 15, (unsigned)capacity));
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sweep_trace), (size_t)n * 32) != hipSuccess) return -1;
    const unsigned zero = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sweep_trace_n), &zero, sizeof(zero));
    return (int)n;
}
#endif

}  // namespace viprs
