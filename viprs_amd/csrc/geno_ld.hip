// LD from packed genotype rows (geno_ld.h): the two instantiations per output element type and their launcher.
#include "geno_ld.h"

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

template <typename O>
int launch_typed(hipStream_t stream, GenoLdArgs A, const int64_t* d_clean, int64_t n_clean, const int64_t* d_general,
                 int64_t n_general) {
    if (n_clean > 0) {
        A.pairs = d_clean;
        geno_ld_kernel<O, true><<<dim3((unsigned)n_clean), dim3(64), 0, stream>>>(A);
        HIP_TRY(hipGetLastError());
    }
    if (n_general > 0) {
        A.pairs = d_general;
        geno_ld_kernel<O, false><<<dim3((unsigned)n_general), dim3(256), 0, stream>>>(A);
        HIP_TRY(hipGetLastError());
    }
    return VIPRS_OK;
}
}  // namespace

int launch_geno_ld(hipStream_t stream, int out_dtype, GenoLdArgs A, const int64_t* d_pairs_clean, int64_t n_clean,
                   const int64_t* d_pairs_general, int64_t n_general) {
    if (n_clean >= ((int64_t)1 << 31) || n_general >= ((int64_t)1 << 31))
        return fail(VIPRS_EINVAL, "too many tile pairs in one call: give a smaller row range");
    switch (out_dtype) {
        case VIPRS_LD_I8: return launch_typed<int8_t>(stream, A, d_pairs_clean, n_clean, d_pairs_general, n_general);
        case VIPRS_LD_I16: return launch_typed<int16_t>(stream, A, d_pairs_clean, n_clean, d_pairs_general, n_general);
        case VIPRS_LD_F32: return launch_typed<float>(stream, A, d_pairs_clean, n_clean, d_pairs_general, n_general);
        case VIPRS_LD_F64: return launch_typed<double>(stream, A, d_pairs_clean, n_clean, d_pairs_general, n_general);
        default: return fail(VIPRS_EINVAL, "bad LD output dtype code");
    }
}

}  // namespace viprs
