// Band kernel (estep_band.h) of the SBayesR policy (panel_bayesr.h) for one LD element type: included by
// band_bayesr_f32.hip / band_bayesr_i8.hip / band_bayesr_i16.hip with BAND_U defined.  Only the kernel is chosen here: ring
// sizing, the launch and the upper form's epilogue are launch_band_kernel's (launch_band.inc).
#include "internal.h"
#include "estep_band.h"
#include "panel_bayesr.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

// The symmetric form only: the upper form's instantiation keeps 3 registers of its set-up code in scratch (16 B per lane,
// all three LD types), and kernels with scratch are not shipped -- viprs_state_bayesr_sweep refuses windowed blocks of an
// upper-form plan before it gets here.
template <typename U>
int launch_band_bayesr(viprs_plan* P, EStepArgs<float> A) {
    if (P->low_memory != 0) return fail(VIPRS_EINVAL, "SBayesR sweep: no band kernel for the upper-triangular form");
    return launch_band_kernel<U>(P, A, estep_band_kernel<U, BayesRModel, true>, 1);
}

template int launch_band_bayesr<BAND_U>(viprs_plan*, EStepArgs<float>);

}  // namespace viprs
