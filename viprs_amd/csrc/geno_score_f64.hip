#include "geno_score.h"

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);
}
template <>
int launch_geno_score<double>(hipStream_t stream, GenoScoreArgs<double> S, GenoReduceArgs<double> R) {
    return launch_geno_score_impl<double>(stream, S, R);
}
}  // namespace viprs
