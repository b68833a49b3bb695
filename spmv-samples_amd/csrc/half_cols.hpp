// half_cols.hpp — a lane's 16 bytes of a row held in 16 bits: EIGHT columns of binary16 / bfloat16, widened exactly into
// eight fp32 registers (half_convert.hpp's widen), and stored from them, each narrowed once (narrow_to).  What the kinds
// that hold rows in 16 bits share: multi-vector SpMV with 16-bit X and Y (multi_half_kernels.hpp), SDDMM with 16-bit U and V
// (sddmm_half_kernel.hpp, which hands load_cols to sddmm_slice_walk.inc by a using-declaration) and fused attention with
// 16-bit Q, K, V and O (attention_half_kernel.hpp, which hands both to attention_slice_walk.inc the same way).  The names
// stay in mh, the namespace they were written in: multi_half_slice_kernel compiles to the device code on record, and what
// a kernel calls does not enter its name.
#pragma once

#include "half_convert.hpp"

namespace mi355 {
namespace mh {

constexpr int kHalfV = 8;   // columns of a lane: 16 bytes of a row of 16-bit values

struct __attribute__((aligned(16), may_alias)) U32x4 { uint32_t x, y, z, w; };   // eight 16-bit columns per lane

// the lane's 8 columns of a row, widened: one 16-byte access when the row is aligned and all 8 exist, else the nv that do
template <typename vec_t>
__device__ __forceinline__ void load_cols(float (&v)[kHalfV], const vec_t* p, int nv, bool vec) {
    if (vec && nv == kHalfV) {
        const U32x4 t = *reinterpret_cast<const U32x4*>(p);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[2 * q] = widen(from_bits(uint16_t(w[q] & 0xFFFFu), vec_t()));
            v[2 * q + 1] = widen(from_bits(uint16_t(w[q] >> 16), vec_t()));
        }
    } else {
#pragma unroll
        for (int j = 0; j < kHalfV; ++j) v[j] = j < nv ? widen(p[j]) : 0.0f;
    }
}

// the lane's 8 columns of a row, each narrowed once (narrow_to: nearest even): one 16-byte store when the row is aligned
// and all 8 exist, else the nv that do
template <typename vec_t>
__device__ __forceinline__ void store_cols(const float (&v)[kHalfV], vec_t* p, int nv, bool vec) {
    if (vec && nv == kHalfV) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            w[q] = uint32_t(bits_of(narrow_to(v[2 * q], vec_t()))) | (uint32_t(bits_of(narrow_to(v[2 * q + 1], vec_t()))) << 16);
        *reinterpret_cast<U32x4*>(p) = U32x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
        for (int j = 0; j < kHalfV; ++j)
            if (j < nv) p[j] = narrow_to(v[j], vec_t());
    }
}

}  // namespace mh
}  // namespace mi355
