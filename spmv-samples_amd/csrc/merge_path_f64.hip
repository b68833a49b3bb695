// merge_path_f64.hip — the fp64 (and fp32-matrix-under-fp64-vectors) instantiations of the MERGE kind (see merge_path_f32.hip).
#include "merge_launch.hpp"

namespace mi355 {
template int launch_merge<int32_t, double, double>(Plan&, const int32_t*, const double*, const double*, double*, hipStream_t);
template int launch_merge<int64_t, double, double>(Plan&, const int64_t*, const double*, const double*, double*, hipStream_t);
// fp32 matrix under fp64 vectors (mi355_spmv_plan_create_typed)
template int launch_merge<int32_t, double, float>(Plan&, const int32_t*, const float*, const double*, double*, hipStream_t);
template int launch_merge<int64_t, double, float>(Plan&, const int64_t*, const float*, const double*, double*, hipStream_t);
}  // namespace mi355
