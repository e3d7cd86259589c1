#define SCORE_U int32_t
#define SCORE_DENSE 0
#include "launch_ld_score.inc"
