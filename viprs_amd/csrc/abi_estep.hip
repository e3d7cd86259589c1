// C ABI, part 3 (include/viprs_hip.h): the E-step entry points and the sweep schedule -- which kernel family
// serves which blocks of a plan, on which streams -- plus the per-sweep timing hooks.
#include "internal.h"

#include <type_traits>

using namespace viprs;

namespace {

// zeroes the work-queue heads, the skip counter and the team hand-off granules in ONE launch
__global__ void sweep_prologue_kernel(int32_t* counters, int n_counters, unsigned long long* skipped,
                                      unsigned long long* granules, int64_t n_granules) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_counters) counters[i] = 0;
    if (i == 0) { skipped[0] = 0ull; skipped[1] = 0ull; }
    for (int64_t k = i; k < n_granules; k += (int64_t)gridDim.x * blockDim.x) granules[k] = 0ull;
}

// A sweep that is ONE panel launch has no prologue: its last workgroup moves the running skip count [0] to [1].  If the
// sweep before it on this plan ran kernels that count in place (float64 state, batched grid, generic / band kernels: they
// leave their total in [0]), that leftover must not be folded into this sweep's count: one 8-byte memset, only then.
hipError_t clear_stale_skip_count(viprs_plan* P) {
    if (!P->skip_count_in_place) return hipSuccess;
    P->skip_count_in_place = false;
    return hipMemsetAsync(P->d_skipped.p, 0, sizeof(unsigned long long), P->stream);
}

// The prologue launch of a sweep; its kernels count in place.  (Grid launches: one granule set per active model.)
int sweep_prologue(viprs_plan* P, int n_models) {
    P->skip_count_in_place = true;
    const int64_t ng = P->n_granule_rows * kPanel * std::max(1, n_models);
    if (P->d_granules.n < (size_t)ng) {
        HIP_TRY(hipStreamSynchronize(P->stream));
        HIP_TRY(P->d_granules.alloc((size_t)ng));
    }
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ng + 255) / 256, 1024));
    sweep_prologue_kernel<<<grid, 256, 0, P->stream>>>(P->d_counters.p, kPlanCounters, P->d_skipped.p, P->d_granules.p, ng);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}

template <typename T>
EStepArgs<T> make_args(viprs_state* S, double dq) {
    viprs_plan* P = S->plan;
    EStepArgs<T> A{};
    A.skipped = P->d_skipped.p;
    A.lb = P->d_lb.p;
    A.rowstart = P->d_ip.p;
    A.rowlen = P->d_rowlen.p;
    A.ld_rows = P->d_ld_raw.p;
    A.ld_dense = P->d_ld_dense.p;
    A.ld_zero_off = P->dense_elems;          // (abi_plan.hip: zeroed slack of >= 4 * kStrip elements behind the last block)
    A.std_beta = (const T*)S->f[VIPRS_FIELD_STD_BETA].p;
    A.u_logs = (const T*)S->f[VIPRS_FIELD_U_LOGS].p;
    A.shvt = (const T*)S->f[VIPRS_FIELD_SQRT_HALF_VAR_TAU].p;
    A.mu_mult = (const T*)S->f[VIPRS_FIELD_MU_MULT].p;
    A.log_null_pi = (const T*)S->f[VIPRS_FIELD_LOG_NULL_PI].p;
    A.var_gamma = (T*)S->f[VIPRS_FIELD_VAR_GAMMA].p;
    A.var_mu = (T*)S->f[VIPRS_FIELD_VAR_MU].p;
    A.eta = (T*)S->f[VIPRS_FIELD_ETA].p;
    A.q = (T*)S->f[VIPRS_FIELD_Q].p;
    A.eta_diff = (T*)S->f[VIPRS_FIELD_ETA_DIFF].p;
    A.eta_out = (T*)S->eta_out.p;
    A.q_out = (T*)S->q_out.p;
    A.granules = P->d_granules.p;
    A.granule_rows = P->n_granule_rows;
    A.error = P->d_error.p;
    A.dq = (T)dq;
    A.low_memory = P->low_memory;
    A.width = S->width;
    A.m = P->m;
    return A;
}

// One launcher instantiation per LD element type: `f` is called with a value of the type `ld_dtype` names.  The list `Us` is
// explicit at every call site: the launchers are explicitly instantiated per translation unit for exactly those types, and a
// dispatch over all six would ask the linker for instantiations that do not exist.
template <typename U> constexpr int ld_code();
template <> constexpr int ld_code<int8_t>() { return VIPRS_LD_I8; }
template <> constexpr int ld_code<int16_t>() { return VIPRS_LD_I16; }
template <> constexpr int ld_code<int32_t>() { return VIPRS_LD_I32; }
template <> constexpr int ld_code<int64_t>() { return VIPRS_LD_I64; }
template <> constexpr int ld_code<float>() { return VIPRS_LD_F32; }
template <> constexpr int ld_code<double>() { return VIPRS_LD_F64; }

template <typename... Us, typename F>
int for_ld_type(int ld_dtype, const char* otherwise, F&& f) {
    int rc = VIPRS_OK;
    const bool found = ((ld_dtype == ld_code<Us>() && ((rc = f(Us{})), true)) || ...);
    return found ? rc : fail(VIPRS_EINVAL, otherwise);
}

// the batched grid kernel, matrix-core path: chunks of 32 models, each LD row read once per chunk
template <typename U>
int launch_grid_chunks(viprs_state* S, const EStepArgs<float>& A) {
    viprs_plan* P = S->plan;
    const int64_t lists_per_chunk = (int64_t)S->n_groups * kGroupListStride;
    for (int off = 0; off < A.n_active; off += kGridModels) {
        EStepArgs<float> Ac = A;
        Ac.active = A.active + off;
        Ac.n_active = std::min(kGridModels, A.n_active - off);
        if (A.group_cols) Ac.group_lists = S->d_group_lists.p + (off / kGridModels) * lists_per_chunk;
        int rc = off > 0 ? sweep_prologue(P, 1) : VIPRS_OK;
        if (rc == VIPRS_OK) rc = launch_grid_mfma<U>(P, Ac);
        if (rc != VIPRS_OK) return rc;
    }
    return VIPRS_OK;
}

// the launcher of one family of a route over one block list
template <typename T>
int launch_family(viprs_state* S, const EStepArgs<T>& A, int family, int model, bool dense) {
    viprs_plan* P = S->plan;
    if (family == kFamNone) return VIPRS_OK;
    if (family == kFamGeneric)
        return for_ld_type<int8_t, int16_t, int32_t, int64_t, float, double>(P->ld_dtype, "bad LD dtype", [&](auto u) {
            return launch_generic<T, decltype(u)>(P, A, model, dense); });
    if constexpr (std::is_same<T, double>::value) {
        if (family == kFamTileF64)
            return for_ld_type<int8_t, int16_t, int32_t, int64_t, float, double>(P->ld_dtype, "bad LD dtype", [&](auto u) {
                return launch_tile_f64<decltype(u)>(P, A, model, dense); });
    } else {
        // (kPanelGridColumn: ONE launch over (block, model) work items, select_model offsets the columns in-kernel)
        // (the elastic-net and Gibbs policies have their own translation units and launchers: launch_panel_enet.inc,
        //  launch_band_enet.inc, launch_panel_gibbs.inc, launch_band_gibbs.inc; SBayesR likewise: launch_panel_bayesr.inc,
        //  launch_band_bayesr.inc)
        if (family == kFamPanel)
            return for_ld_type<float, int8_t, int16_t>(P->ld_dtype, kDenseLdTypeError, [&](auto u) {
                return model == kPanelElasticNet ? launch_panel_enet<decltype(u)>(P, A)
                       : model == kPanelGibbs    ? launch_panel_gibbs<decltype(u)>(P, A)
                       : model == kPanelBayesR   ? launch_panel_bayesr<decltype(u)>(P, A)
                                                 : launch_panel<decltype(u)>(P, A, model); });
        if (family == kFamBand)
            return for_ld_type<float, int8_t, int16_t>(P->ld_dtype, kBandLdTypeError, [&](auto u) {
                return model == kBandElasticNet ? launch_band_enet<decltype(u)>(P, A)
                       : model == kBandGibbs    ? launch_band_gibbs<decltype(u)>(P, A)
                       : model == kBandBayesR   ? launch_band_bayesr<decltype(u)>(P, A)
                                                : launch_band<decltype(u)>(P, A, model); });
        if (family == kFamGridBatched)
            return for_ld_type<float, int8_t, int16_t>(P->ld_dtype, kDenseLdTypeError, [&](auto u) {
                return launch_grid_chunks<decltype(u)>(S, A); });
    }
    return fail(VIPRS_EINVAL, "kernel family without an instantiation for the state precision");
}

// the launchers of a route, in stream order, between the events of the timing record
template <typename T>
int launch_route(viprs_state* S, const SweepRoute& r, double dq, const int32_t* d_active, int n_active) {
    viprs_plan* P = S->plan;
    EStepArgs<T> A = make_args<T>(S, dq);
    A.active = d_active;
    A.n_active = n_active;
    // a Gibbs sweep: the slot a grid state does not use carries its draws (panel_gibbs.h)
    if constexpr (std::is_same<T, float>::value)
        if (r.dense_model == kPanelGibbs || r.ragged_model == kBandGibbs) A.log_null_pi = gibbs_draws_slot(S);
    if (S->model_kind == VIPRS_MODEL_GRID && !S->group_cols_h.empty()) {     // (group_mask_prepare: fp32 state, dense blocks only)
        A.blk_group = S->d_blk_group.p;
        A.group_cols = S->d_group_cols.p;
    }
    int rc = launch_family<T>(S, A, r.dense_family, r.dense_model, true);
    if (rc != VIPRS_OK) return rc;
    rc = P->timing.dense_done();
    if (rc != VIPRS_OK) return rc;
    return launch_family<T>(S, A, r.ragged_family, r.ragged_model, false);
}

// Environment switches are read per call (tests flip them between sweeps).
bool band_ok(const viprs_plan* P) {
    const char* f = getenv("VIPRS_BAND");
    if (f && !atoi(f)) return false;
    if (P->ld_dtype != VIPRS_LD_F32 && P->ld_dtype != VIPRS_LD_I8 && P->ld_dtype != VIPRS_LD_I16) return false;
    return band_ring_panels(P) <= kBandMaxRingPanels;
}

// One workgroup per LD block: worth it once the blocks can occupy a good part of the chip; with a few
// blocks the (block, model) work items of the panel kernel spread better.  32-bit element offsets.
bool use_grid_mfma(const viprs_plan* P, int width) {
    if ((int64_t)P->m * std::max(1, width) >= (1LL << 31)) return false;
    if (P->grid_mfma >= 0) return P->grid_mfma != 0;
    return (int64_t)P->dense_h.size() * 8 >= (int64_t)P->n_cu * 3;
}

// Executes a route (sweep_route.h): the prologue launch where the route asks for one, the timing slot, the launchers.
int run_route(viprs_state* S, const SweepRoute& r, double dq, const int32_t* d_active, int n_active) {
    viprs_plan* P = S->plan;
    int rc = VIPRS_OK;
    // begin the sweep: the books of the kernels, then the timing slot
    if (r.prologue) rc = sweep_prologue(P, r.prologue_per_model ? n_active : 1);
    else HIP_TRY(clear_stale_skip_count(P));
    if (rc != VIPRS_OK) return rc;
    P->math_used = 0;
    rc = P->timing.open(r.whole_sweep_events, r.dense_bracketed);
    if (rc != VIPRS_OK) return rc;
    if (r.dense_bracketed && r.start_event_by_launcher) P->timing.arm();
    else if (r.dense_bracketed) { rc = P->timing.start(); if (rc != VIPRS_OK) return rc; }
    rc = S->float_dtype == VIPRS_F32 ? launch_route<float>(S, r, dq, d_active, n_active)
                                     : launch_route<double>(S, r, dq, d_active, n_active);
    if (rc != VIPRS_OK) { P->timing.abandon(); return rc; }
    return P->timing.close();
}

// One sweep of any model: the route (sweep_route.h) says which kernel family serves which block list, whether the prologue
// launch is needed and which events are recorded; run_route executes it.
int run_sweep(viprs_state* S, double dq, const int32_t* d_active, int n_active) {
    static_assert(kGenSpikeSlab == VIPRS_MODEL_SPIKE_SLAB && kGenMixture == VIPRS_MODEL_MIXTURE && kGenGrid == VIPRS_MODEL_GRID, "");
    viprs_plan* P = S->plan;
    HIP_TRY(hipSetDevice(P->device));
    const SweepConfig c{S->float_dtype, S->model_kind, S->width, P->ld_dtype, !P->dense_h.empty(), !P->ragged_h.empty(), band_ok(P),
                        use_grid_mfma(P, S->width), getenv("VIPRS_F64_ROW_BY_ROW") != nullptr};
    SweepRoute r;
    std::string err;
    const int rc = sweep_route(c, r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    return run_route(S, r, dq, d_active, n_active);
}

// A grid state with SNP groups under a (group, column) mask (viprs_state_set_group_columns): the batched matrix-core kernel
// and the panel kernel's (block, model) items take the mask; the kernels of the other paths have none and refuse.  The
// group of every block of the dense list, indexed as the list is, is rebuilt whenever the list changes.
int group_mask_prepare(viprs_state* S, const int32_t* active, int n_active) {
    viprs_plan* P = S->plan;
    if (S->float_dtype != VIPRS_F32)
        return fail(VIPRS_EUNSUPPORTED, "grid state with a (group, column) mask: float64 states are not supported");
    if (!P->ragged_h.empty())
        return fail(VIPRS_EUNSUPPORTED, "grid state with a (group, column) mask: ragged / banded LD blocks are not supported "
                                        "(the generic and band kernels take no mask)");
    // the matrix-core kernel's per-group lists of this call: launch k covers active[32 k .. 32 k + 31]; a group's list is
    // that chunk's columns whose mask byte is set, in order, padded with the last of them (or with the chunk's first column
    // when there is none: the block is skipped)
    const int n_chunks = (n_active + kGridModels - 1) / kGridModels;
    std::vector<int32_t> lists((size_t)n_chunks * S->n_groups * kGroupListStride, 0);
    for (int k = 0; k < n_chunks; ++k) {
        const int lo = k * kGridModels, hi = std::min(n_active, lo + kGridModels);
        for (int g = 0; g < S->n_groups; ++g) {
            int32_t* l = lists.data() + ((size_t)k * S->n_groups + g) * kGroupListStride;
            int cnt = 0;
            for (int i = lo; i < hi; ++i)
                if (S->group_cols_h[(size_t)g * S->width + active[i]]) l[1 + cnt++] = active[i];
            l[0] = cnt;
            for (int t = cnt; t < kGridModels; ++t) l[1 + t] = cnt > 0 ? l[cnt] : active[lo];
        }
    }
    HIP_TRY(hipStreamSynchronize(P->stream));              // (a sweep in flight may read the old lists / map)
    if (S->d_group_lists.n < lists.size()) HIP_TRY(S->d_group_lists.alloc(lists.size()));
    HIP_TRY(hipMemcpy(S->d_group_lists.p, lists.data(), lists.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (S->blk_group_gen != P->dense_gen || S->d_blk_group.n < P->dense_h.size()) {
        std::vector<int32_t> map(std::max<size_t>(1, P->dense_h.size()), 0);
        for (size_t k = 0; k < P->dense_h.size(); ++k)     // (an empty group shares its start with the next one: `upper_bound`)
            map[k] = (int32_t)(std::upper_bound(S->group_start.begin(), S->group_start.end(), (int64_t)P->dense_h[k].start) -
                               S->group_start.begin()) - 1;
        HIP_TRY(S->d_blk_group.alloc(map.size()));
        HIP_TRY(hipMemcpy(S->d_blk_group.p, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        S->blk_group_gen = P->dense_gen;
    }
    return VIPRS_OK;
}

// The active list of a grid sweep: null = every model (`all` then holds the list); VIPRS_EINVAL for an index out of range.
int active_list_check(const viprs_state* S, const int32_t*& active, int& n_active, std::vector<int32_t>& all) {
    if (!active) {
        all.resize((size_t)S->width);
        for (int g = 0; g < S->width; ++g) all[(size_t)g] = g;
        active = all.data();
        n_active = S->width;
    }
    for (int i = 0; i < n_active; ++i)
        if (active[i] < 0 || active[i] >= S->width) return fail(VIPRS_EINVAL, "active_model_idx out of range");
    return VIPRS_OK;
}

int active_list_upload(viprs_state* S, const int32_t* active, int n_active) {
    if (S->d_active.n < (size_t)n_active) HIP_TRY(S->d_active.alloc((size_t)std::max(n_active, S->width)));
    HIP_TRY(hipMemcpyAsync(S->d_active.p, active, sizeof(int32_t) * (size_t)n_active, hipMemcpyHostToDevice, S->plan->stream));
    HIP_TRY(hipStreamSynchronize(S->plan->stream));   // `active` may be a temporary
    return VIPRS_OK;
}

// the fields of viprs_route_field, in the order of the enum
void route_fields(const SweepRoute& r, int* route) {
    const int out[VIPRS_ROUTE_COUNT] = {r.dense_family, r.dense_model, r.ragged_family, r.ragged_model, r.prologue,
                                        r.prologue_per_model, r.start_event_by_launcher, r.whole_sweep_events, r.dense_bracketed};
    std::copy(out, out + VIPRS_ROUTE_COUNT, route);
}

}  // namespace

extern "C" {

int viprs_state_e_step(viprs_state* S, double dq_scale, const int32_t* active, int n_active, int sync) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    int rc;
    switch (S->model_kind) {
        case VIPRS_MODEL_SPIKE_SLAB: case VIPRS_MODEL_MIXTURE: rc = run_sweep(S, dq_scale, nullptr, 0); break;
        case VIPRS_MODEL_GRID: {
            std::vector<int32_t> all;
            rc = active_list_check(S, active, n_active, all);
            if (rc != VIPRS_OK) return rc;
            if (n_active == 0) return VIPRS_OK;
            HIP_TRY(hipSetDevice(S->plan->device));
            if (!S->group_cols_h.empty()) {
                rc = group_mask_prepare(S, active, n_active);
                if (rc != VIPRS_OK) return rc;
            }
            rc = active_list_upload(S, active, n_active);
            if (rc != VIPRS_OK) return rc;
            rc = run_sweep(S, dq_scale, S->d_active.p, n_active);
            break;
        }
        default: return fail(VIPRS_EINVAL, "bad model kind");
    }
    if (rc != VIPRS_OK) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(S->plan->stream));
    return VIPRS_OK;
}

int viprs_state_enet_sweep(viprs_state* S, double dq_scale, const int32_t* active, int n_active, int sync) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    // every refusal comes before the first launch
    if (S->model_kind == VIPRS_MODEL_MIXTURE) return fail(VIPRS_EINVAL, "elastic-net sweep: not defined for a mixture state");
    if (S->model_kind != VIPRS_MODEL_SPIKE_SLAB && S->model_kind != VIPRS_MODEL_GRID) return fail(VIPRS_EINVAL, "bad model kind");
    if (S->float_dtype != VIPRS_F32)
        return fail(VIPRS_EUNSUPPORTED, "elastic-net sweep: float64 states are not supported (the kernels are float32)");
    const bool grid = S->model_kind == VIPRS_MODEL_GRID;
    if (grid && !S->group_cols_h.empty())
        return fail(VIPRS_EUNSUPPORTED, "elastic-net sweep: a grid state under a (group, column) mask is not supported");
    viprs_plan* P = S->plan;
    std::vector<int32_t> all;
    if (grid) {
        const int rc = active_list_check(S, active, n_active, all);
        if (rc != VIPRS_OK) return rc;
    } else {
        active = nullptr;
        n_active = 0;
    }
    SweepRoute r;
    std::string err;
    int rc = enet_route(grid, P->ld_dtype, !P->dense_h.empty(), !P->ragged_h.empty(), band_ok(P), r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    if (grid && n_active == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    if (grid) {
        rc = active_list_upload(S, active, n_active);
        if (rc != VIPRS_OK) return rc;
    }
    rc = run_route(S, r, dq_scale, grid ? S->d_active.p : nullptr, n_active);
    if (rc != VIPRS_OK) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(P->stream));
    return VIPRS_OK;
}

int viprs_enet_route(int grid, int ld_dtype, int dense, int ragged, int band_ok, int* route) {
    if (!route) return fail(VIPRS_EINVAL, "null argument");
    SweepRoute r;
    std::string err;
    const int rc = enet_route(grid != 0, ld_dtype, dense != 0, ragged != 0, band_ok != 0, r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    route_fields(r, route);
    return VIPRS_OK;
}

int viprs_state_gibbs_sweep(viprs_state* S, double dq_scale, const int32_t* active, int n_active, uint64_t seed,
                            uint64_t draw_index, int flags, int sync) {
    if (!S) return fail(VIPRS_EINVAL, "null state");
    // every refusal comes before the first launch
    if (S->model_kind != VIPRS_MODEL_GRID)
        return fail(VIPRS_EINVAL, "Gibbs sweep: a state of kind VIPRS_MODEL_GRID is needed (spike-and-slab-kind and mixture "
                                  "states are refused)");
    if (S->float_dtype != VIPRS_F32) return fail(VIPRS_EINVAL, "Gibbs sweep: float64 states are not supported (the kernels are float32)");
    if (!S->group_cols_h.empty()) return fail(VIPRS_EINVAL, "Gibbs sweep: a grid state under a (group, column) mask is not supported");
    if (flags & ~VIPRS_GIBBS_KEEP_DRAWS) return fail(VIPRS_EINVAL, "Gibbs sweep: unknown flag");
    const bool keep = (flags & VIPRS_GIBBS_KEEP_DRAWS) != 0;
    viprs_plan* P = S->plan;
    if (keep && !S->d_gibbs_draws.p && P->m > 0)
        return fail(VIPRS_EINVAL, "Gibbs sweep: VIPRS_GIBBS_KEEP_DRAWS before the draw buffers exist (no draws call, sweep or "
                                  "upload yet)");
    std::vector<int32_t> all;
    int rc = active_list_check(S, active, n_active, all);
    if (rc != VIPRS_OK) return rc;
    SweepRoute r;
    std::string err;
    rc = gibbs_route(P->ld_dtype, !P->dense_h.empty(), !P->ragged_h.empty(), band_ok(P), r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    if (n_active == 0 || P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    rc = active_list_upload(S, active, n_active);
    if (rc != VIPRS_OK) return rc;
    if (!keep) {
        rc = gibbs_enqueue_draws(S, seed, draw_index, S->d_active.p, n_active);
        if (rc != VIPRS_OK) return rc;
    }
    rc = run_route(S, r, dq_scale, S->d_active.p, n_active);
    if (rc != VIPRS_OK) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(P->stream));
    return VIPRS_OK;
}

int viprs_gibbs_route(int ld_dtype, int dense, int ragged, int band_ok, int* route) {
    if (!route) return fail(VIPRS_EINVAL, "null argument");
    SweepRoute r;
    std::string err;
    const int rc = gibbs_route(ld_dtype, dense != 0, ragged != 0, band_ok != 0, r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    route_fields(r, route);
    return VIPRS_OK;
}

// The sweep of SBayesR (panel_bayesr.h; the rest of its calls: abi_bayesr.hip).  It lives here because it is executed by
// run_route like every other sweep: a mixture state runs with n_active == 0, and the `active` slot, which nothing then reads
// but the policy, carries the state's draw allocation.
int viprs_state_bayesr_sweep(viprs_state* S, double dq_scale, uint64_t seed, uint64_t draw_index, int flags, int sync) {
    // every refusal comes before the first launch
    int rc = bayesr_state_check(S, "SBayesR sweep");
    if (rc != VIPRS_OK) return rc;
    if (flags & ~VIPRS_BAYESR_KEEP_DRAWS) return fail(VIPRS_EINVAL, "SBayesR sweep: unknown flag");
    const bool keep = (flags & VIPRS_BAYESR_KEEP_DRAWS) != 0;
    viprs_plan* P = S->plan;
    if (keep && !S->d_bayesr.p && P->m > 0)
        return fail(VIPRS_EINVAL, "SBayesR sweep: VIPRS_BAYESR_KEEP_DRAWS before the draw buffers exist (no draws call, sweep or "
                                  "upload yet)");
    SweepRoute r;
    std::string err;
    // (the band kernel of this policy exists for the symmetric form only: launch_band_bayesr.inc)
    rc = bayesr_route(P->ld_dtype, !P->dense_h.empty(), !P->ragged_h.empty(), band_ok(P) && P->low_memory == 0, r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    rc = keep ? VIPRS_OK : bayesr_enqueue_draws(S, seed, draw_index);
    if (rc != VIPRS_OK) return rc;
    if (!S->d_bayesr.p) return fail(VIPRS_EDEVICE, "SBayesR sweep: no draw buffers");
    rc = run_route(S, r, dq_scale, reinterpret_cast<const int32_t*>(S->d_bayesr.p), 0);
    if (rc != VIPRS_OK) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(P->stream));
    return VIPRS_OK;
}

int viprs_bayesr_route(int ld_dtype, int dense, int ragged, int band_ok, int* route) {
    if (!route) return fail(VIPRS_EINVAL, "null argument");
    SweepRoute r;
    std::string err;
    const int rc = bayesr_route(ld_dtype, dense != 0, ragged != 0, band_ok != 0, r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    route_fields(r, route);
    return VIPRS_OK;
}

// The one-shot calls: the plan's scratch state of that precision, model and width takes the caller's buffers (`host`: one
// pointer per viprs_field, in the order of the enum), is swept once and hands the five state fields back.
static int one_shot(viprs_plan* P, int float_dtype, int model_kind, int width, const void* const (&host)[VIPRS_FIELD_COUNT],
                    double dq, const int32_t* active, int n_active) {
    viprs_state* S = P->scratch;
    if (!S || S->float_dtype != float_dtype || S->model_kind != model_kind || S->width != width) {
        delete P->scratch;
        P->scratch = nullptr;
        int rc = viprs_state_create(&P->scratch, P, float_dtype, model_kind, width);
        if (rc != VIPRS_OK) return rc;
        S = P->scratch;
    }
    const size_t fs = float_size(S->float_dtype);
    HIP_TRY(hipSetDevice(P->device));
    // (a field the model does not have -- log_null_pi outside the mixture -- has no bytes)
    for (int f : {VIPRS_FIELD_STD_BETA, VIPRS_FIELD_LOG_NULL_PI, VIPRS_FIELD_U_LOGS, VIPRS_FIELD_SQRT_HALF_VAR_TAU, VIPRS_FIELD_MU_MULT,
                  VIPRS_FIELD_VAR_GAMMA, VIPRS_FIELD_VAR_MU, VIPRS_FIELD_ETA, VIPRS_FIELD_Q, VIPRS_FIELD_ETA_DIFF}) {
        const size_t bytes = S->field_elems(f) * fs;
        if (bytes == 0) continue;
        if (!host[f]) return fail(VIPRS_EINVAL, "null buffer");
        HIP_TRY(hipMemcpyAsync(S->f[f].p, host[f], bytes, hipMemcpyHostToDevice, P->stream));
    }
    int rc = viprs_state_e_step(S, dq, active, n_active, 0);
    if (rc != VIPRS_OK) return rc;
    for (int f : {VIPRS_FIELD_VAR_GAMMA, VIPRS_FIELD_VAR_MU, VIPRS_FIELD_ETA, VIPRS_FIELD_Q, VIPRS_FIELD_ETA_DIFF})
        HIP_TRY(hipMemcpyAsync(const_cast<void*>(host[f]), S->f[f].p, S->field_elems(f) * fs, hipMemcpyDeviceToHost, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    return check_device_error(P);                      // a timed-out team hand-off must not return silently
}

int viprs_e_step(viprs_plan* P, int float_dtype, const void* std_beta, void* var_gamma, void* var_mu, void* eta,
                 void* q, void* eta_diff, const void* u_logs, const void* shvt, const void* mu_mult,
                 double dq_scale, int threads, int low_memory) {
    (void)threads;
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    if ((low_memory != 0) != (P->low_memory != 0))
        return fail(VIPRS_EINVAL, "low_memory differs from the value the plan was created with");
    if (P->m == 0) return VIPRS_OK;
    const void* const host[] = {std_beta, u_logs, shvt, mu_mult, nullptr, var_gamma, var_mu, eta, q, eta_diff};
    return one_shot(P, float_dtype, VIPRS_MODEL_SPIKE_SLAB, 1, host, dq_scale, nullptr, 0);
}

int viprs_e_step_mixture(viprs_plan* P, int float_dtype, int K, const void* std_beta, void* var_gamma, void* var_mu,
                         void* eta, void* q, void* eta_diff, const void* log_null_pi, const void* u_logs,
                         const void* shvt, const void* mu_mult, double dq_scale, int threads, int low_memory) {
    (void)threads;
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    if ((low_memory != 0) != (P->low_memory != 0))
        return fail(VIPRS_EINVAL, "low_memory differs from the value the plan was created with");
    if (K < 1) return fail(VIPRS_EINVAL, "K must be >= 1");
    if (P->m == 0) return VIPRS_OK;
    const void* const host[] = {std_beta, u_logs, shvt, mu_mult, log_null_pi, var_gamma, var_mu, eta, q, eta_diff};
    return one_shot(P, float_dtype, VIPRS_MODEL_MIXTURE, K, host, dq_scale, nullptr, 0);
}

int viprs_e_step_grid(viprs_plan* P, int float_dtype, int G, const void* std_beta, void* var_gamma, void* var_mu,
                      void* eta, void* q, void* eta_diff, const void* u_logs, const void* half_var_tau,
                      const void* mu_mult, double dq_scale, const int32_t* active_model_idx, int n_active, int threads,
                      int low_memory) {
    (void)threads;
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    if ((low_memory != 0) != (P->low_memory != 0))
        return fail(VIPRS_EINVAL, "low_memory differs from the value the plan was created with");
    if (G < 1) return fail(VIPRS_EINVAL, "G must be >= 1");
    if (n_active < 0 || (n_active > 0 && !active_model_idx)) return fail(VIPRS_EINVAL, "bad active_model_idx");
    if (P->m == 0 || n_active == 0) return VIPRS_OK;
    const void* const host[] = {std_beta, u_logs, half_var_tau, mu_mult, nullptr, var_gamma, var_mu, eta, q, eta_diff};
    return one_shot(P, float_dtype, VIPRS_MODEL_GRID, G, host, dq_scale, active_model_idx, n_active);
}

int viprs_plan_last_kernel_ms(viprs_plan* P, int which, double* ms) {
    if (!P || !ms) return fail(VIPRS_EINVAL, "null argument");
    if (P->timing.sweeps == 0) return fail(VIPRS_EINVAL, "no timed sweep yet");
    HIP_TRY(hipSetDevice(P->device));
    return P->timing.elapsed(P->timing.sweeps - 1, which, ms);
}

int viprs_plan_timing_reset(viprs_plan* P) {
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipStreamSynchronize(P->stream));
    P->timing.reset();
    return VIPRS_OK;
}

int viprs_plan_timing_history(viprs_plan* P, int which, double* ms, int capacity, int* n) {
    if (!P || !ms || !n) return fail(VIPRS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(P->device));
    const int64_t have = std::min<int64_t>(P->timing.sweeps, SweepTiming::kRing);
    const int count = (int)std::min<int64_t>(have, capacity);
    for (int i = 0; i < count; ++i) {
        int rc = P->timing.elapsed(P->timing.sweeps - count + i, which, &ms[i]);
        if (rc != VIPRS_OK) return rc;
    }
    *n = count;
    return VIPRS_OK;
}

int viprs_sweep_route(int float_dtype, int model_kind, int width, int ld_dtype, int dense, int ragged, int band_ok,
                      int grid_mfma, int f64_row_by_row, int* route) {
    if (!route) return fail(VIPRS_EINVAL, "null argument");
    if ((float_dtype != VIPRS_F32 && float_dtype != VIPRS_F64) || model_kind < kGenSpikeSlab || model_kind > kGenGrid || width < 1)
        return fail(VIPRS_EINVAL, "bad state precision, model kind or width");
    const SweepConfig c{float_dtype, model_kind, width, ld_dtype, dense != 0, ragged != 0, band_ok != 0, grid_mfma != 0,
                        f64_row_by_row != 0};
    SweepRoute r;
    std::string err;
    const int rc = sweep_route(c, r, err);
    if (rc != VIPRS_OK) return fail(rc, err);
    route_fields(r, route);
    return VIPRS_OK;
}

int viprs_plan_last_math_modes(const viprs_plan* P, int* mask) {
    if (!P || !mask) return fail(VIPRS_EINVAL, "null argument");
    *mask = P->math_used;
    return VIPRS_OK;
}

int viprs_plan_last_skipped(viprs_plan* P, int64_t* n) {
    if (!P || !n) return fail(VIPRS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipStreamSynchronize(P->stream));
    unsigned long long v[2] = {0, 0};       // [0]: kernels that count in place, [1]: moved there by the panel sweep's last workgroup
    HIP_TRY(hipMemcpy(v, P->d_skipped.p, sizeof(v), hipMemcpyDeviceToHost));
    *n = (int64_t)(v[0] + v[1]);
    return VIPRS_OK;
}

}  // extern "C"
