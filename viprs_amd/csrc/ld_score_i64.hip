#define SCORE_U int64_t
#define SCORE_DENSE 0
#include "launch_ld_score.inc"
