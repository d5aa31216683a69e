// bx_boost_tab.hip - boost_frame_kernel's build for an engine with a per-sequence parameter
// table (bx_boost_set_seq_params_host), in a code object of its own: bx_boost.hip up to the frame
// kernel, its TAB = true instantiation and the two entry points bx_boost.hip's host code calls.
#define BX_BOOST_TAB_UNIT
#include "bx_boost.hip"
