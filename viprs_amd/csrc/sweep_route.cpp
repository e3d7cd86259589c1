#include "sweep_route.h"

#include "../../include/viprs_hip.h"
#include "kernels_common.h"      // kPanelMaxK, kPanelWideMaxK

namespace viprs {

int sweep_route(const SweepConfig& c, SweepRoute& r, std::string& err) {
    r = SweepRoute{};
    const bool f32 = c.float_dtype == VIPRS_F32;
    const bool spike_slab = c.model == kGenSpikeSlab, grid = c.model == kGenGrid;      // otherwise: mixture
    if (!f32) {
        // float64 state: the panel kernels specialise float; every block takes the panel-walking kernel of estep_tile.h
        r.dense_family = r.ragged_family = c.f64_row_by_row ? kFamGeneric : kFamTileF64;
        r.dense_model = r.ragged_model = c.model;
    } else {
        // fp32 state on dense blocks: the panel kernels with the model's policy; the grid as (block, model) work items of
        // ONE panel launch, or -- once the blocks can occupy a good part of the chip -- on the batched matrix-core kernel.
        // Mixtures beyond the wide chain (K > kPanelWideMaxK) take the generic kernels.
        if (c.dense && (spike_slab || grid || c.width <= kPanelWideMaxK)) {
            r.dense_family = grid && c.grid_mfma ? kFamGridBatched : kFamPanel;
            r.dense_model = spike_slab ? kPanelSpikeSlab
                            : grid     ? kPanelGridColumn
                                       : (c.width <= kPanelMaxK ? kPanelMixture : kPanelMixtureWide);
        } else if (!spike_slab) {
            r.dense_family = kFamGeneric;          // (called with whatever the list holds: it returns early on an empty one)
            r.dense_model = c.model;
        }
        // windowed components: the band kernel where its q ring fits (spike-and-slab, grid columns, mixtures of up to
        // kPanelMaxK components), the generic kernels otherwise
        if (c.ragged && c.band_ok && (spike_slab || grid || c.width <= kPanelMaxK)) {
            r.ragged_family = kFamBand;
            r.ragged_model = spike_slab ? kBandSpikeSlab : (grid ? kBandGridColumn : kBandMixture);
        } else if (c.ragged || !spike_slab) {
            r.ragged_family = kFamGeneric;
            r.ragged_model = c.model;
        }
    }
    // one panel launch and nothing else: no prologue (the batched grid kernel and every other family count on it)
    r.prologue = !(r.dense_family == kFamPanel && !c.ragged);
    r.prologue_per_model = grid;
    r.start_event_by_launcher = r.dense_family == kFamPanel || r.dense_family == kFamGridBatched;
    // spike-and-slab: the dense launcher has its own bracket inside the whole sweep's, unless it is the whole sweep;
    // mixture / grid: one bracket around all kernels of the call
    r.whole_sweep_events = spike_slab && r.prologue;
    r.dense_bracketed = !spike_slab || c.dense;

    const bool three = c.ld_dtype == VIPRS_LD_F32 || c.ld_dtype == VIPRS_LD_I8 || c.ld_dtype == VIPRS_LD_I16;
    if (!three && r.start_event_by_launcher) { err = kDenseLdTypeError; return VIPRS_EINVAL; }
    if (!three && r.ragged_family == kFamBand) { err = kBandLdTypeError; return VIPRS_EINVAL; }
    return VIPRS_OK;
}

int enet_route(bool grid, int ld_dtype, bool dense, bool ragged, bool band_ok, SweepRoute& r, std::string& err) {
    r = SweepRoute{};
    if (ragged && !band_ok) {
        err = "elastic-net sweep: windowed LD blocks the band kernel cannot take (VIPRS_BAND=0, or a window wider than its q "
              "ring): there is no row-by-row kernel for this update";
        return VIPRS_EUNSUPPORTED;
    }
    if (dense) { r.dense_family = kFamPanel; r.dense_model = kPanelElasticNet; }
    if (ragged) { r.ragged_family = kFamBand; r.ragged_model = kBandElasticNet; }
    // as sweep_route: spike-and-slab row (width 1) / grid row
    r.prologue = !(dense && !ragged);
    r.prologue_per_model = grid;
    r.start_event_by_launcher = dense;
    r.whole_sweep_events = !grid && r.prologue;
    r.dense_bracketed = grid || dense;

    const bool three = ld_dtype == VIPRS_LD_F32 || ld_dtype == VIPRS_LD_I8 || ld_dtype == VIPRS_LD_I16;
    if (!three && dense) { err = kDenseLdTypeError; return VIPRS_EINVAL; }
    if (!three && ragged) { err = kBandLdTypeError; return VIPRS_EINVAL; }
    return VIPRS_OK;
}

int gibbs_route(int ld_dtype, bool dense, bool ragged, bool band_ok, SweepRoute& r, std::string& err) {
    r = SweepRoute{};
    if (ragged && !band_ok) {
        err = "Gibbs sweep: windowed LD blocks the band kernel cannot take (VIPRS_BAND=0, or a window wider than its q ring): "
              "there is no row-by-row kernel for this update";
        return VIPRS_EINVAL;
    }
    if (dense) { r.dense_family = kFamPanel; r.dense_model = kPanelGibbs; }
    if (ragged) { r.ragged_family = kFamBand; r.ragged_model = kBandGibbs; }
    // as sweep_route's grid row
    r.prologue = !(dense && !ragged);
    r.prologue_per_model = true;
    r.start_event_by_launcher = dense;
    r.whole_sweep_events = false;
    r.dense_bracketed = true;

    const bool three = ld_dtype == VIPRS_LD_F32 || ld_dtype == VIPRS_LD_I8 || ld_dtype == VIPRS_LD_I16;
    if (!three && dense) { err = kDenseLdTypeError; return VIPRS_EINVAL; }
    if (!three && ragged) { err = kBandLdTypeError; return VIPRS_EINVAL; }
    return VIPRS_OK;
}

int bayesr_route(int ld_dtype, bool dense, bool ragged, bool band_ok, SweepRoute& r, std::string& err) {
    r = SweepRoute{};
    if (ragged && !band_ok) {
        err = "SBayesR sweep: windowed LD blocks the band kernel cannot take (VIPRS_BAND=0, a window wider than its q ring, or "
              "the upper-triangular form: build the plan in the symmetric form, low_memory = 0 / SBayesR(low_memory=False)): there is "
              "no row-by-row kernel for this update";
        return VIPRS_EINVAL;
    }
    if (dense) { r.dense_family = kFamPanel; r.dense_model = kPanelBayesR; }
    if (ragged) { r.ragged_family = kFamBand; r.ragged_model = kBandBayesR; }
    // as sweep_route's mixture row
    r.prologue = !(dense && !ragged);
    r.prologue_per_model = false;
    r.start_event_by_launcher = dense;
    r.whole_sweep_events = false;
    r.dense_bracketed = true;

    const bool three = ld_dtype == VIPRS_LD_F32 || ld_dtype == VIPRS_LD_I8 || ld_dtype == VIPRS_LD_I16;
    if (!three && dense) { err = kDenseLdTypeError; return VIPRS_EINVAL; }
    if (!three && ragged) { err = kBandLdTypeError; return VIPRS_EINVAL; }
    return VIPRS_OK;
}

}  // namespace viprs
