// slice_cut.hpp — what the slice kinds share: multi-vector SpMV (multi_kernels.hpp, multi_half_kernels.hpp) and SDDMM
// (sddmm.hip, sddmm_half_kernel.hpp; their one walk, sddmm_slice_walk.inc).  Both cut A into slices of kSliceLen merge items (row ends + nonzeros: a run of empty rows cannot make
// the row range of a slice unbounded, a hub row is spread over as many waves as it has slices), give one WAVE a slice,
// and spread a step's nonzeros over (nonzero slot x 16-byte column group) lanes.  Here: the geometry and its host
// arithmetic, the 16-byte column access of a lane, and the steps of a group of 64 nonzeros.  The cut itself — the wave's
// two diagonals and its rows' offsets in LDS — and the search of a nonzero's row in them are text: slice_cut.inc,
// slice_cut_row.inc.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace mi355 {

constexpr int kSliceLen = 1024;                 // merge items per slice (= per wave)
constexpr int kSliceGroupsMax = 8;              // most 16-byte column groups of a tile: 32 fp32 / int32, 16 fp64, 64 16-bit columns
constexpr int kSliceWaves = kBlock / kWave;     // slices per workgroup

inline int64_t slice_count(int32_t n_rows, int64_t nnz) { return (int64_t(n_rows) + nnz + kSliceLen - 1) / kSliceLen; }
inline int64_t slice_grid(int64_t n_slices) { return (n_slices + kSliceWaves - 1) / kSliceWaves; }

// rows of a row-major operand are 16-byte aligned: a lane may take its column group in one 16-byte access
template <typename T>
bool rows_aligned16(const void* p, int64_t ld) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (size_t(ld) * sizeof(T)) % 16 == 0;
}

// f(lanes) with lanes::value = C, the lanes per nonzero slot for a tile of `groups` 16-byte column groups
template <typename F>
void with_slot_lanes(int groups, F f) {
    if (groups <= 1) f(std::integral_constant<int, 1>());
    else if (groups <= 2) f(std::integral_constant<int, 2>());
    else if (groups <= 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, kSliceGroupsMax>());
}

struct alignas(16) I32x4 { int32_t x, y, z, w; };   // four int32 columns per lane, as float4 for fp32
template <typename val_t> struct Pack16;
template <> struct Pack16<float> { using type = float4; };
template <> struct Pack16<double> { using type = double2; };
template <> struct Pack16<int32_t> { using type = I32x4; };

// the lane's V columns of a row: one 16-byte access when the row is aligned and all V exist, else the nv that do; a
// column that does not exist is loaded as 0 and is never read or written
template <typename val_t, int V>
__device__ __forceinline__ void load_cols(val_t (&v)[V], const val_t* p, int nv, bool vec) {
    if (vec && nv == V) {
        const auto t = *reinterpret_cast<const typename Pack16<val_t>::type*>(p);
        v[0] = t.x; v[1] = t.y;
        if constexpr (V == 4) { v[2] = t.z; v[3] = t.w; }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = j < nv ? p[j] : val_t(0);
    }
}

template <typename val_t, int V>
__device__ __forceinline__ void store_cols(const val_t (&v)[V], val_t* p, int nv, bool vec) {
    if (vec && nv == V) {
        typename Pack16<val_t>::type t;
        t.x = v[0]; t.y = v[1];
        if constexpr (V == 4) { t.z = v[2]; t.w = v[3]; }
        *reinterpret_cast<typename Pack16<val_t>::type*>(p) = t;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < nv) p[j] = v[j];
    }
}

// steps of a group of 64 nonzeros of which `left` exist: S = 64 / C slots take S nonzeros per step
template <int C>
__device__ __forceinline__ int slice_group_steps(int left) {
    constexpr int S = kWave / C;
    return left >= kWave ? C : (left + S - 1) / S;
}

}  // namespace mi355
