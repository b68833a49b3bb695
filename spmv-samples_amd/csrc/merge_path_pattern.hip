// the merge kind's tile kernels for pattern matrices (MI355_VAL_PATTERN: no stored values): a translation unit of their own
#define MI355_TU_PATTERN 1
#include "merge_path.hip"
