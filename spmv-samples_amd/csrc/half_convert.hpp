// half_convert.hpp — the 16-bit storage types (binary16 as F16, bfloat16 as common.hpp's Bf16) and their conversions to and
// from fp32: widen is exact; narrow_to rounds to nearest even (overflow to +-inf, NaN stays NaN, subnormals kept).
// What csr_vector_h16.hip (narrowing a matrix's values), multi_half_kernels.hpp (16-bit X and Y) and sddmm_half_kernel.hpp
// (16-bit U and V, through sddmm_slice_walk.inc's load_cols) convert with; the widening load of a lane's eight columns built on them: half_cols.hpp.
// Plain C++ (casts and integer bit operations); where the compiler has no _Float16 (the host compiler of the
// lane-by-lane simulation) binary16 is held as uint16_t and converted in software.
#pragma once

#include "common.hpp"

namespace mi355 {

#ifdef __FLT16_MANT_DIG__
using F16 = _Float16;
__host__ __device__ __forceinline__ float widen(F16 v) { return float(v); }                           // (v_cvt_f32_f16)
__host__ __device__ __forceinline__ F16 narrow_to(float v, F16) { return F16(v); }                    // (v_cvt_f16_f32)
__host__ __device__ __forceinline__ uint16_t bits_of(F16 v) { return __builtin_bit_cast(uint16_t, v); }
__host__ __device__ __forceinline__ F16 from_bits(uint16_t b, F16) { return __builtin_bit_cast(F16, b); }
#else
struct F16 { uint16_t bits; };
inline float widen(F16 h) {
    const uint32_t s = uint32_t(h.bits & 0x8000u) << 16, e = (h.bits >> 10) & 31u, m = h.bits & 0x3FFu;
    if (e == 0) {       // zero or subnormal: m * 2^-24, exact in fp32
        const float v = float(m) * 5.9604644775390625e-08f;
        return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) | s);
    }
    if (e == 31) return __builtin_bit_cast(float, s | 0x7F800000u | (m << 13));
    return __builtin_bit_cast(float, s | ((e + 112u) << 23) | (m << 13));
}
inline F16 narrow_to(float v, F16) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v), s = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return F16{uint16_t(s | 0x7E00u | ((a >> 13) & 0x3FFu))};      // NaN stays NaN (quiet)
    if (a >= 0x47800000u) return F16{uint16_t(s | 0x7C00u)};                            // 65 536 and beyond: inf
    if (a >= 0x38800000u) {                                                             // normal: nearest, ties to even
        uint32_t r = a - (112u << 23);
        r += 0xFFFu + ((r >> 13) & 1u);                                                 // (65 520 and beyond carry into inf)
        return F16{uint16_t(s | (r >> 13))};
    }
    if (a <= 0x33000000u) return F16{uint16_t(s)};                                      // up to 2^-25 (a tie to even): zero
    const uint32_t mant = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - (a >> 23);        // 14 .. 24
    uint32_t h = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (h & 1u))) ++h;                                   // (0x400 = the smallest normal)
    return F16{uint16_t(s | h)};
}
inline uint16_t bits_of(F16 v) { return v.bits; }
inline F16 from_bits(uint16_t b, F16) { return F16{b}; }
#endif

// bfloat16 is the upper half of an fp32
__host__ __device__ __forceinline__ float widen(Bf16 v) { return __builtin_bit_cast(float, uint32_t(v.bits) << 16); }
__host__ __device__ __forceinline__ Bf16 narrow_to(float v, Bf16) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) u |= 0x00400000u;      // NaN: keep it one (quiet) when the payload's low bits go
    else u += 0x7FFFu + ((u >> 16) & 1u);                       // nearest, ties to even; carries into the exponent up to inf
    return Bf16{uint16_t(u >> 16)};
}
__host__ __device__ __forceinline__ uint16_t bits_of(Bf16 v) { return v.bits; }
__host__ __device__ __forceinline__ Bf16 from_bits(uint16_t b, Bf16) { return Bf16{b}; }
__host__ __device__ __forceinline__ float widen(float v) { return v; }      // an fp32 matrix under 16-bit vectors

}  // namespace mi355
