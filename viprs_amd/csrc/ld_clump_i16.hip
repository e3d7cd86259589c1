#define CLUMP_U int16_t
#define CLUMP_DENSE 1
#include "launch_ld_clump.inc"
