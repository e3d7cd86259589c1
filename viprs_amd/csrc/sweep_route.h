// The route of an E-step sweep: which kernel family serves the dense blocks, which the windowed (ragged) ones, whether a
// prologue launch is needed and which HIP events the sweep records.  One pure function of a handful of facts about the
// state, the plan and the environment; abi_estep.hip gathers the facts per call and executes what comes back.  Pure C++
// (no HIP), so it runs -- and is tested -- on machines without a GPU (viprs_sweep_route, include/viprs_hip.h).
#pragma once
#include <string>

namespace viprs {

// ---- kernel families (one translation unit per family and LD element type) and their model constants -------------
enum { kFamNone = 0, kFamGeneric = 1, kFamTileF64 = 2, kFamPanel = 3, kFamBand = 4, kFamGridBatched = 5 };   // viprs_sweep_family
enum { kGenSpikeSlab = 0, kGenMixture = 1, kGenGrid = 2 };          // = viprs_model_kind; the tile_f64 kernels take them too
enum { kPanelSpikeSlab = 0, kPanelGridColumn = 1, kPanelMixture = 2, kPanelMixtureWide = 3, kPanelElasticNet = 4, kPanelGibbs = 5,
       kPanelBayesR = 6 };
enum { kBandSpikeSlab = 0, kBandGridColumn = 1, kBandMixture = 2, kBandElasticNet = 3, kBandGibbs = 4, kBandBayesR = 5 };

// the launchers' own words for an LD element type they have no instantiation for
constexpr const char* kDenseLdTypeError = "dense schedule with unsupported LD dtype";
constexpr const char* kBandLdTypeError = "band schedule with unsupported LD dtype";

// what the route depends on
struct SweepConfig {
    int float_dtype;           // VIPRS_F32 / VIPRS_F64: precision of the state
    int model;                 // kGenSpikeSlab / kGenMixture / kGenGrid
    int width;                 // mixture: K; grid: G
    int ld_dtype;              // viprs_ld_dtype
    bool dense, ragged;        // the active dense / ragged list is non-empty
    bool band_ok;              // VIPRS_BAND is not 0, the band kernel has the element type, the plan's widest window fits its q ring
    bool grid_mfma;            // grid: the batched matrix-core kernel (VIPRS_GRID_MFMA, or enough blocks to fill the chip)
    bool f64_row_by_row;       // VIPRS_F64_ROW_BY_ROW (experiments / A-B): float64 states on the generic kernels
};

struct SweepRoute {
    int dense_family, dense_model;       // launcher of the dense list and the model constant it takes (kFamNone: none is called)
    int ragged_family, ragged_model;     // ... of the ragged list
    // The prologue launch zeroes the queue heads, the skip counter and the team hand-off granules.  A sweep that is ONE panel
    // launch needs none: the panel sweep keeps its own books -- generation-tagged granules, queue heads reset and the skip
    // count published by its last workgroup.
    bool prologue;
    bool prologue_per_model;             // granules for every active model (grid), not for one
    // The panel and batched-grid launchers record the start event of the dense bracket themselves, adjacent to their (first)
    // kernel launch; otherwise the caller records it in front of the dense launcher.
    bool start_event_by_launcher;
    // ev[0] .. ev[1] around everything, ev[2] .. ev[3] around the dense launcher only.  Without them ev[2] .. ev[3] go around
    // all kernels of the call and stand for both (every event record costs stream time).
    bool whole_sweep_events;
    bool dense_bracketed;                // ev[2] .. ev[3] are recorded at all
};

// VIPRS_OK, or VIPRS_EINVAL with the message the launch would give (`err`) when the chosen family has no instantiation for
// the LD element type.
int sweep_route(const SweepConfig& c, SweepRoute& r, std::string& err);

// The route of an elastic-net sweep (viprs_state_enet_sweep) of an fp32 state of width 1 (`grid` false) or of a grid state:
// the panel sweep for the dense blocks, the band kernel for the windowed ones -- the columns of a grid state as (block,
// model) items, never the batched matrix-core kernel -- with the prologue and the events of the spike-and-slab row of
// sweep_route for width 1 and of its grid row for a grid state.  There is no generic-kernel instantiation: windowed blocks
// the band kernel cannot take (`band_ok` false) are VIPRS_EUNSUPPORTED; an LD element type outside fp32 / int8 / int16 is
// VIPRS_EINVAL with the launcher's message, as above.
int enet_route(bool grid, int ld_dtype, bool dense, bool ragged, bool band_ok, SweepRoute& r, std::string& err);

// The route of an LDpred2 Gibbs sweep (viprs_state_gibbs_sweep) of an fp32 grid state: kPanelGibbs for the dense blocks,
// kBandGibbs for the windowed ones, the columns as (block, model) items, with the prologue and the events of the grid row of
// sweep_route.  Refusals as enet_route's, in its own words.
int gibbs_route(int ld_dtype, bool dense, bool ragged, bool band_ok, SweepRoute& r, std::string& err);

// The route of an SBayesR sweep (viprs_state_bayesr_sweep) of an fp32 mixture state of K <= 4 components: kPanelBayesR for the
// dense blocks, kBandBayesR for the windowed ones, with the prologue and the events of the mixture row of sweep_route.
// Refusals, each VIPRS_EINVAL: windowed blocks the band kernel cannot take (`band_ok` false: for this sweep that includes
// every upper-form plan, whose band instantiation is not shipped); an LD element type outside the shipped ones (fp32 /
// int8 / int16), with the launcher's message.
int bayesr_route(int ld_dtype, bool dense, bool ragged, bool band_ok, SweepRoute& r, std::string& err);

}  // namespace viprs
