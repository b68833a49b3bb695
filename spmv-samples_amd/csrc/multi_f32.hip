// multi_f32.hip — the fp32 instantiations of multi-vector SpMV: launch_multi over both offset widths, the five semirings,
// valued and pattern matrices (multi_kernels.hpp; see the head of multi.hip).
#define MI355_MULTI_TU float
#include "multi.hip"
