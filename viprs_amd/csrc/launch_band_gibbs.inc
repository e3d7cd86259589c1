// Band kernel (estep_band.h) of the Gibbs policy (panel_gibbs.h) for one LD element type: included by
// band_gibbs_f32.hip / band_gibbs_i8.hip / band_gibbs_i16.hip with BAND_U defined.  Only the kernel is chosen here: ring
// sizing, the launch and the upper form's epilogue are launch_band_kernel's (launch_band.inc).
#include "internal.h"
#include "estep_band.h"
#include "panel_gibbs.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

template <typename U>
int launch_band_gibbs(viprs_plan* P, EStepArgs<float> A) {
    return launch_band_kernel<U>(P, A, P->low_memory != 0 ? estep_band_kernel<U, GibbsModel, false>
                                                          : estep_band_kernel<U, GibbsModel, true>, 1);
}

template int launch_band_gibbs<BAND_U>(viprs_plan*, EStepArgs<float>);

}  // namespace viprs
