// Panel sweep (estep_panel.h) of the elastic-net policy (panel_enet.h) for one LD element type: included by
// panel_enet_f32.hip / panel_enet_i8.hip / panel_enet_i16.hip with PANEL_U defined.  Only the kernel is chosen here: team
// split, LDS sizing, granules and the launch gate are launch_panel_kernel's (launch_panel.inc).
#include "internal.h"
#include "estep_panel.h"
#include "panel_enet.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

// (one arithmetic whatever the plan's math_mode: the update has no transcendental function to approximate)
template <typename U>
int launch_panel_enet(viprs_plan* P, EStepArgs<float> A) {
    constexpr int NW = kPanelWaves, CPL = panel_cols<U>();
    const void* kfn = P->low_memory != 0 ? (const void*)estep_sweep_kernel<U, ElasticNetModel, kFormMirror, NW, CPL>
                                         : (const void*)estep_sweep_kernel<U, ElasticNetModel, kFormSym, NW, CPL>;
    return launch_panel_kernel<U>(P, A, kPanelElasticNet, kfn, NW, 1);
}

template int launch_panel_enet<PANEL_U>(viprs_plan*, EStepArgs<float>);

}  // namespace viprs
