// Band kernel (estep_band.h) launchers for one LD element type: windowed (ragged) components, fp32 state.  Included by
// band_f32.hip / band_i8.hip / band_i16.hip with BAND_U defined (one translation unit per type: they compile side by side).
#include "internal.h"
#include "estep_band.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

int band_ring_panels(const viprs_plan* P);

// `kfn`: the estep_band_kernel instantiation of the model's policy for this form (the caller selects it: launch_band below;
// launch_band_enet.inc for the policies that live in translation units of their own); `math_bit`: what it adds to
// viprs_plan_last_math_modes.
template <typename U>
int launch_band_kernel(viprs_plan* P, EStepArgs<float> A, BandKernelFn kfn, int math_bit) {
    A.blocks = P->d_ragged.p;
    A.n_blocks = (int)P->ragged_h.size();
    A.counter = P->d_counters.p + 1;
    const int ring = band_ring_panels(P);
    const size_t shmem = (size_t)band_lds_floats(ring) * sizeof(float);
    P->math_used |= math_bit;
    const bool upper = P->low_memory != 0;
    HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    const int items = A.n_blocks * std::max(A.n_active, 1);
    const int grid = std::min(items, 2 * P->n_cu);
    kfn<<<grid, 64 * kBandWaves, shmem, P->stream>>>(A, ring);
    HIP_TRY(hipGetLastError());
    if (upper) {
        const dim3 egrid((unsigned)std::min(256, (P->max_ragged + 255) / 256), (unsigned)items);
        band_upper_epilogue_kernel<U><<<egrid, 256, 0, P->stream>>>(A);
        HIP_TRY(hipGetLastError());
    }
    return VIPRS_OK;
}

template <typename U>
int launch_band(viprs_plan* P, EStepArgs<float> A, int model) {
    const bool exact = P->math_mode == VIPRS_MATH_EXACT;
    const bool upper = P->low_memory != 0;
    BandKernelFn kfn = nullptr;
#define BK(MODEL) (upper ? estep_band_kernel<U, MODEL, false> : estep_band_kernel<U, MODEL, true>)
    if (model == kBandGridColumn) kfn = exact ? BK(GridColumnModel<true>) : BK(GridColumnModel<false>);
    else if (model == kBandMixture) kfn = exact ? BK(MixtureSerialModel<true>) : BK(MixtureSerialModel<false>);
    else kfn = exact ? BK(SpikeSlabModel<true>) : BK(SpikeSlabModel<false>);
#undef BK
    return launch_band_kernel<U>(P, A, kfn, exact ? 1 : 2);
}

template int launch_band_kernel<BAND_U>(viprs_plan*, EStepArgs<float>, BandKernelFn, int);
template int launch_band<BAND_U>(viprs_plan*, EStepArgs<float>, int);

}  // namespace viprs
