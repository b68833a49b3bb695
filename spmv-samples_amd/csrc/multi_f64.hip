// multi_f64.hip — the fp64 instantiations of multi-vector SpMV: launch_multi over both offset widths, the five semirings,
// valued and pattern matrices (multi_kernels.hpp; see the head of multi.hip).
#define MI355_MULTI_TU double
#include "multi.hip"
