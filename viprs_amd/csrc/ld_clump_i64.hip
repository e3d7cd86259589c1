#define CLUMP_U int64_t
#define CLUMP_DENSE 0
#include "launch_ld_clump.inc"
