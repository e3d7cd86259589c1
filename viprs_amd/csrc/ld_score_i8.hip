#define SCORE_U int8_t
#define SCORE_DENSE 1
#include "launch_ld_score.inc"
