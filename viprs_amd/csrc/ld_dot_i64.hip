#define DOT_U int64_t
#define DOT_DENSE 0
#include "launch_ld_dot.inc"
