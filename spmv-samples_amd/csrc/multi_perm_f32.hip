// multi_perm_f32.hip — the fp32 instantiations of the permuted multi-vector kernels: launch_multi_perm over both offset
// widths (multi_kernels.hpp; see the head of multi.hip).
#define MI355_MULTI_PERM_TU float
#include "multi.hip"
