#define BAND_U float
#include "launch_band_bayesr.inc"
