// the merge kind's tile kernels for pattern matrices (MI355_VAL_PATTERN: no stored values), for all three vector types: a
// translation unit of their own (see merge_path_f32.hip)
#include "merge_launch.hpp"

namespace mi355 {
template int launch_merge<int32_t, float, PatternOnes>(Plan&, const int32_t*, const PatternOnes*, const float*, float*, hipStream_t);
template int launch_merge<int64_t, float, PatternOnes>(Plan&, const int64_t*, const PatternOnes*, const float*, float*, hipStream_t);
template int launch_merge<int32_t, double, PatternOnes>(Plan&, const int32_t*, const PatternOnes*, const double*, double*, hipStream_t);
template int launch_merge<int64_t, double, PatternOnes>(Plan&, const int64_t*, const PatternOnes*, const double*, double*, hipStream_t);
template int launch_merge<int32_t, int32_t, PatternOnes>(Plan&, const int32_t*, const PatternOnes*, const int32_t*, int32_t*, hipStream_t);
template int launch_merge<int64_t, int32_t, PatternOnes>(Plan&, const int64_t*, const PatternOnes*, const int32_t*, int32_t*, hipStream_t);
}  // namespace mi355
