#define ROWS_U double
#define ROWS_DENSE 0
#define ROWS_SCORE 1
#include "launch_ld_rows.inc"
