#define ROWS_U int8_t
#define ROWS_DENSE 1
#define ROWS_SCORE 0
#include "launch_ld_rows.inc"
