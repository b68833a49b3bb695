// semiring.hpp — the enumerated semirings (MI355_SEMIRING_* of include/mi355_spmv.h) as compile-time traits: what the
// merge kind's kernels (merge_path.hip, merge_plan.hip) and the multi-vector kernels (multi_kernels.hpp) are
// instantiated over.  Device code only, and nothing beyond <hip/hip_runtime.h>'s __device__ / __forceinline__.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/mi355_spmv.h"

namespace mi355 {

// ---- semirings --------------------------------------------------------------
// The reference's generalized merge kind takes a functor with initialize / combine / reduce
// (include/spmv/merge_genl/merge_genl.cuh:19-38, agent_spmv_orig.cuh:98-124; CPU twin
// include/spmv/cpu_navie.hpp:20-34) and ships one instance, (+, *).  A C ABI cannot take a C++
// functor, so the semirings are enumerated (include/mi355_spmv.h).  min/max never round, so
// MIN_PLUS and MAX_TIMES results are bit-exact whatever the reduction order.
// "infinities" of a value type: +-inf for floating point, the extreme integers for int32 (min-plus / max-plus on
// integer weights: an identity only ever meets reduce(), never combine(), so it cannot overflow)
template <typename val_t> struct Extreme {
    __device__ static __forceinline__ val_t hi() { return val_t(INFINITY); }
    __device__ static __forceinline__ val_t lo() { return val_t(-INFINITY); }
};
template <> struct Extreme<int32_t> {
    __device__ static __forceinline__ int32_t hi() { return INT32_MAX; }
    __device__ static __forceinline__ int32_t lo() { return INT32_MIN; }
};
template <int S, typename val_t> struct Semiring;
template <typename val_t> struct Semiring<MI355_SEMIRING_PLUS_TIMES, val_t> {
    __device__ static __forceinline__ val_t identity() { return val_t(0); }
    __device__ static __forceinline__ val_t combine(val_t a, val_t x) { return a * x; }
    __device__ static __forceinline__ val_t reduce(val_t u, val_t v) { return u + v; }
};
template <typename val_t> struct Semiring<MI355_SEMIRING_MIN_PLUS, val_t> {
    __device__ static __forceinline__ val_t identity() { return Extreme<val_t>::hi(); }
    __device__ static __forceinline__ val_t combine(val_t a, val_t x) { return a + x; }
    __device__ static __forceinline__ val_t reduce(val_t u, val_t v) { return v < u ? v : u; }
};
template <typename val_t> struct Semiring<MI355_SEMIRING_MAX_TIMES, val_t> {
    __device__ static __forceinline__ val_t identity() { return Extreme<val_t>::lo(); }
    __device__ static __forceinline__ val_t combine(val_t a, val_t x) { return a * x; }
    __device__ static __forceinline__ val_t reduce(val_t u, val_t v) { return u < v ? v : u; }
};

template <typename val_t> struct Semiring<MI355_SEMIRING_MAX_PLUS, val_t> {
    __device__ static __forceinline__ val_t identity() { return Extreme<val_t>::lo(); }
    __device__ static __forceinline__ val_t combine(val_t a, val_t x) { return a + x; }
    __device__ static __forceinline__ val_t reduce(val_t u, val_t v) { return u < v ? v : u; }
};
template <typename val_t> struct Semiring<MI355_SEMIRING_OR_AND, val_t> {   // booleans carried as 0.0 / 1.0
    __device__ static __forceinline__ val_t identity() { return val_t(0); }
    __device__ static __forceinline__ val_t combine(val_t a, val_t x) { return (a != val_t(0) && x != val_t(0)) ? val_t(1) : val_t(0); }
    __device__ static __forceinline__ val_t reduce(val_t u, val_t v) { return (u != val_t(0) || v != val_t(0)) ? val_t(1) : val_t(0); }
};

}  // namespace mi355
