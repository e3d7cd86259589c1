#define DOT_U int16_t
#define DOT_DENSE 1
#include "launch_ld_dot.inc"
