#define DOT_U int32_t
#define DOT_DENSE 0
#include "launch_ld_dot.inc"
