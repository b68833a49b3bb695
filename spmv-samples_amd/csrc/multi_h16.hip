// multi_h16.hip — the instantiations of multi-vector SpMV with 16-bit vectors: launch_multi_half over both offset widths,
// binary16 and bfloat16 vectors, the matrix in the vectors' type and in fp32 (multi_half_kernels.hpp; see the head of
// multi.hip).
#define MI355_MULTI_HALF_TU 1
#include "multi.hip"
