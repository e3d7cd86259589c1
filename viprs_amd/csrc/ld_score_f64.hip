#define SCORE_U double
#define SCORE_DENSE 0
#include "launch_ld_score.inc"
