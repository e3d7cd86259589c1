#define CLUMP_U double
#define CLUMP_DENSE 0
#include "launch_ld_clump.inc"
