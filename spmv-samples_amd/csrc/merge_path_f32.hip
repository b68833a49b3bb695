// merge_path_f32.hip — the fp32 instantiations of the MERGE kind's launch path (merge_launch.hpp).  One translation unit per
// value type (merge_path_f64.hip, merge_path_i32.hip) and one for pattern matrices (merge_path_pattern.hip): the four
// parts of the instantiations compile side by side.
#include "merge_launch.hpp"

namespace mi355 {
template int launch_merge<int32_t, float, float>(Plan&, const int32_t*, const float*, const float*, float*, hipStream_t);
template int launch_merge<int64_t, float, float>(Plan&, const int64_t*, const float*, const float*, float*, hipStream_t);
}  // namespace mi355
