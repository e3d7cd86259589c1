#include "geno_class_sums.h"

#include <algorithm>

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

constexpr int kMaxGroupsPerLaunch = 65535;                      // grid.y

// groups of W columns from A.col0 on, as many as fit below n_cols; the rest goes to the narrower instantiations, so that no
// lane computes a column that is not there
template <int W>
int launch_class_sum_groups(hipStream_t stream, GenoClassSumsArgs& A) {
    const int64_t per_block = (int64_t)kClassSumWaves * kClassSumRows;
    const dim3 block(kClassSumWaves * 64);
    for (int groups = (A.n_cols - A.col0) / W; groups > 0;) {
        const int now = std::min(groups, kMaxGroupsPerLaunch);
        const dim3 grid((unsigned)((A.row1 - A.row0 + per_block - 1) / per_block), (unsigned)now);
        geno_class_sums_kernel<W><<<grid, block, 0, stream>>>(A);
        HIP_TRY(hipGetLastError());
        A.col0 += now * W;
        groups -= now;
    }
    if constexpr (W > 1) return launch_class_sum_groups<W / 2>(stream, A);
    return VIPRS_OK;
}
}  // namespace

int launch_geno_class_sums(hipStream_t stream, GenoClassSumsArgs A) {
    A.col0 = 0;
    return launch_class_sum_groups<kClassSumCols>(stream, A);
}

}  // namespace viprs
