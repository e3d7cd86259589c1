#define DOT_U float
#define DOT_DENSE 1
#include "launch_ld_dot.inc"
