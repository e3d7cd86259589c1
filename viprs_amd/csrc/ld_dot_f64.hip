#define DOT_U double
#define DOT_DENSE 0
#include "launch_ld_dot.inc"
