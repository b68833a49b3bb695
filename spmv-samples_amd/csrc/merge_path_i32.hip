// merge_path_i32.hip — the 32-bit-integer-value instantiations of the MERGE kind (see merge_path_f32.hip).
#include "merge_launch.hpp"

namespace mi355 {
// 32-bit integer values (MI355_VAL_I32: every semiring, exact)
template int launch_merge<int32_t, int32_t, int32_t>(Plan&, const int32_t*, const int32_t*, const int32_t*, int32_t*, hipStream_t);
template int launch_merge<int64_t, int32_t, int32_t>(Plan&, const int64_t*, const int32_t*, const int32_t*, int32_t*, hipStream_t);
}  // namespace mi355
