// multi_perm_f64.hip — the fp64 instantiations of the permuted multi-vector kernels: launch_multi_perm over both offset
// widths (multi_kernels.hpp; see the head of multi.hip).
#define MI355_MULTI_PERM_TU double
#include "multi.hip"
