#define PANEL_U int8_t
#include "launch_panel_bayesr.inc"
