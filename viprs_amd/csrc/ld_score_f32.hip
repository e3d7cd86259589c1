#define ROWS_U float
#define ROWS_DENSE 1
#define ROWS_SCORE 1
#include "launch_ld_rows.inc"
