#define CLUMP_U int32_t
#define CLUMP_DENSE 0
#include "launch_ld_clump.inc"
