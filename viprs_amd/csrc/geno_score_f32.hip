#include "geno_score.h"

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);
}
template <>
int launch_geno_score<float>(hipStream_t stream, GenoScoreArgs<float> S, GenoReduceArgs<float> R) {
    return launch_geno_score_impl<float>(stream, S, R);
}
}  // namespace viprs
