// bx_strongsort_tab.hip - the StrongSort kernels' builds for an engine with a per-sequence
// parameter table (bx_ss_set_seq_params_host), in a code object of their own: bx_strongsort.hip
// up to the end of its kernels, the TAB = true instantiations of the kernels that read a
// parameter and the entry points bx_strongsort.hip's host code calls.
#define BX_SS_TAB_UNIT
#include "bx_strongsort.hip"
