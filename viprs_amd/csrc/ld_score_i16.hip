#define SCORE_U int16_t
#define SCORE_DENSE 1
#include "launch_ld_score.inc"
