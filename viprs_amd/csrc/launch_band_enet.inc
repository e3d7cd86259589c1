// Band kernel (estep_band.h) of the elastic-net policy (panel_enet.h) for one LD element type: included by
// band_enet_f32.hip / band_enet_i8.hip / band_enet_i16.hip with BAND_U defined.  Only the kernel is chosen here: ring
// sizing, the launch and the upper form's epilogue are launch_band_kernel's (launch_band.inc).
#include "internal.h"
#include "estep_band.h"
#include "panel_enet.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

template <typename U>
int launch_band_enet(viprs_plan* P, EStepArgs<float> A) {
    return launch_band_kernel<U>(P, A, P->low_memory != 0 ? estep_band_kernel<U, ElasticNetModel, false>
                                                          : estep_band_kernel<U, ElasticNetModel, true>, 1);
}

template int launch_band_enet<BAND_U>(viprs_plan*, EStepArgs<float>);

}  // namespace viprs
