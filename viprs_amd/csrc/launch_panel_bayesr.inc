// Panel sweep (estep_panel.h) of the SBayesR policy (panel_bayesr.h) for one LD element type: included by
// panel_bayesr_f32.hip / panel_bayesr_i8.hip / panel_bayesr_i16.hip with PANEL_U defined.  Only the kernel is chosen here: team
// split, LDS sizing, granules and the launch gate are launch_panel_kernel's (launch_panel.inc).
#include "internal.h"
#include "estep_panel.h"
#include "panel_bayesr.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

// (exact arithmetic whatever the plan's math_mode: a math_mode = fast variant is not built)
template <typename U>
int launch_panel_bayesr(viprs_plan* P, EStepArgs<float> A) {
    constexpr int NW = kPanelWaves, CPL = panel_cols<U>();
    const void* kfn = P->low_memory != 0 ? (const void*)estep_sweep_kernel<U, BayesRModel, kFormMirror, NW, CPL>
                                         : (const void*)estep_sweep_kernel<U, BayesRModel, kFormSym, NW, CPL>;
    return launch_panel_kernel<U>(P, A, kPanelBayesR, kfn, NW, 1);
}

template int launch_panel_bayesr<PANEL_U>(viprs_plan*, EStepArgs<float>);

}  // namespace viprs
