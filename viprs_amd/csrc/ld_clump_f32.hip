#define CLUMP_U float
#define CLUMP_DENSE 1
#include "launch_ld_clump.inc"
