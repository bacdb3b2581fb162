// "bf16x3": fp32 products on the bf16 matrix pipe with BOTH operands split exactly into three bf16 pieces.
//
// gfx950's fp32-input MFMA runs at 1/16 of the bf16 rate.  Every fp32 value is the exact sum of three bf16 numbers
// (x = h + m + l: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even; 3 x 8 mantissa bits, the fp32
// exponent range), so a product x * u is the sum of nine piece products, each exact in fp32.  Six are kept —
// h*H, h*M, m*H, m*M, h*L, l*H; the dropped m*L, l*M, l*L are <= 2^-24 of |x u|, the size of ONE fp32 rounding — and summed
// by v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16 into fp32 accumulators: 6 instructions of 32 cycles per 16 channels
// where the fp32 form issues 8 of 64 cycles, 2.67x fewer matrix-pipe cycles.  Measured against the float64 oracle the logits of
// TIMED-synth are as close as with fp32 products (6.6e-7 either way, 20 classes; 8.9e-7 against 9.3e-7, 338 classes:
// tests/winograd_numerics.py --split); SURVEY.md §7 ("hard parts") names the technique as the one way below the fp32 matrix rate
// that keeps the bound.
//
// This header holds the split itself — on the device a pair of floats at a time (the data operand), on the host from double
// (the weights: residuals in double, so the pieces carry 24 significant bits of a double-precision transform) — and the vector
// types of the MFMA operands.  The ORDER in which a kernel issues its six products fixes the bits of its result and is the
// kernel's own: it is written where the MFMAs are (conv_wino.hip, conv_first_b3.hip, conv_wfsplit.hip, conv_first5.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace bf16x3 {

// two floats -> one word of two bf16 (x in the low half), round to nearest even: v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned pk(f32x2 x) { return __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2)); }
__device__ __forceinline__ unsigned pk(float lo, float hi) { return pk((f32x2){lo, hi}); }
__device__ __forceinline__ float lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
__device__ __forceinline__ f32x2 unpk(unsigned w) { return (f32x2){lo(w), hi(w)}; }

// a pair of floats -> the three packed words h, m, l
__device__ __forceinline__ void split(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = pk(x0, x1);
    const float r0 = x0 - lo(h), r1 = x1 - hi(h);
    m = pk(r0, r1);
    const float s0 = r0 - lo(m), s1 = r1 - hi(m);
    l = pk(s0, s1);
}
// four floats -> the pieces as three pairs of words: the same sequence on both pairs, step by step (written pair after pair the
// second pair's dependent chain costs a wait state in front of every conversion)
__device__ __forceinline__ void split(const float4& x, uint2& h, uint2& m, uint2& l) {
    h = make_uint2(pk(x.x, x.y), pk(x.z, x.w));
    const float rx = x.x - lo(h.x), ry = x.y - hi(h.x), rz = x.z - lo(h.y), rw = x.w - hi(h.y);
    m = make_uint2(pk(rx, ry), pk(rz, rw));
    const float sx = rx - lo(m.x), sy = ry - hi(m.x), sz = rz - lo(m.y), sw = rw - hi(m.y);
    l = make_uint2(pk(sx, sy), pk(sz, sw));
}

// host: the same split from double
inline uint16_t bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16);      // inf / nan: truncate
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline double bf16_val(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return (double)f;
}
inline void split3(double x, uint16_t (&pc)[3]) {
    pc[0] = bf16_rne((float)x);
    const double r1 = x - bf16_val(pc[0]);
    pc[1] = bf16_rne((float)r1);
    const double r2 = r1 - bf16_val(pc[1]);
    pc[2] = bf16_rne((float)r2);
}

}  // namespace bf16x3
