#define SCORE_U float
#define SCORE_DENSE 1
#include "launch_ld_score.inc"
