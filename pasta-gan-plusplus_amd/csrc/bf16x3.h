// The three-term bf16 split: float32 multiplies on the bf16 matrix pipe.  The one home of the arithmetic shared by the F(4x4) Winograd X3 form
// (conv2d_wino4.h), the `up = 2` transposed 3x3 (conv2d_up2x3.h), the stride-2 3x3 (conv2d_s2x3.h), the 7x7 stem (conv2d_stem7x3.h), the bf16x3 weight
// gradient (conv2d_wgrad.hip) and the packers of their weight planes.
//
// The contract:
//   * split: a finite float32 x is the EXACT sum of three bf16 values, x == p0 + p1 + p2, made by truncation: p0 = the leading 16 bits of x, p1 = the leading
//     16 bits of x - p0, p2 = the leading 16 bits of x - p0 - p1 (8 + 8 + 8 significand bits; both subtractions are exact, what is left below p2 is zero).
//   * product: of the nine plane products of a * b the six largest are kept -- a0 b0, a0 b1, a1 b0, a1 b1, a0 b2, a2 b0 -- and the three smallest (a1 b2, a2 b1,
//     a2 b2) dropped: each dropped product is below 2^-24 of the product.  A kept product is bf16 x bf16, exact in float32, and is accumulated in float32 by
//     v_mfma_f32_32x32x16_bf16 with the small products first (X3_PA / X3_PB): float32-class results at 6 / 16 of the fp32 MFMA's issue time.
//   * non-finite operands: the unguarded split (x3_split, x3_split_pair) turns +-inf into inf - inf = NaN in the second plane, so an infinite operand yields
//     NaN where an fp32 kernel yields +-inf; NaN stays NaN.  The guarded split (x3_split_guarded) keeps +-inf (and NaN) in the leading plane with zero remainders.
//   * locality: a NaN sample reaches only the outputs that depend on it (tests/test_nonfinite_locality.py).  A kernel built on the split feeds
//     the multiplier no sample outside its window: a K slot that exists only as padding holds a ZERO operand, not a real sample against a zero weight (0 x NaN).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pgconv {

typedef __bf16 x3_bf16x8 __attribute__((ext_vector_type(8)));       // one lane's A / B operand of v_mfma_f32_32x32x16_bf16
typedef unsigned x3_u32x4 __attribute__((ext_vector_type(4)));      // the same 16 bytes as four packed pairs

// The product order, small products first: step t multiplies plane X3_PA[t] of A by plane X3_PB[t] of B:  a2 b0,  a1 b1,  a1 b0,  a0 b2,  a0 b1,  a0 b0
constexpr int X3_PA[6] = {2, 1, 1, 0, 0, 0}, X3_PB[6] = {0, 1, 0, 2, 1, 0};

// Two values of adjacent K slots -> the three packed operand words (plane 0 = leading bits, 1 = middle, 2 = trailing), low half = the first value:
// 4 v_and + 4 v_sub + 3 v_perm per pair.
__device__ __forceinline__ void x3_split_pair(float va, float vb, unsigned& p0, unsigned& p1, unsigned& p2) {
    const unsigned ua = __float_as_uint(va), ub = __float_as_uint(vb);
    const float ra = va - __uint_as_float(ua & 0xffff0000u), rb = vb - __uint_as_float(ub & 0xffff0000u);
    const unsigned ura = __float_as_uint(ra), urb = __float_as_uint(rb);
    const float la = ra - __uint_as_float(ura & 0xffff0000u), lb = rb - __uint_as_float(urb & 0xffff0000u);
    p0 = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
    p1 = __builtin_amdgcn_perm(urb, ura, 0x07060302u);
    p2 = __builtin_amdgcn_perm(__float_as_uint(lb), __float_as_uint(la), 0x07060302u);
}

// One value -> its three bf16 terms in the low halves.  x3_split: the convolution kernels' activations and every weight packer (weights are finite; an
// infinite activation is documented above).  x3_split_guarded: pg_split3_bf16_cl, whose dy may have overflowed -- it must stay +-inf as in the fp32 kernel.
__device__ __forceinline__ void x3_split(float v, unsigned& b0, unsigned& b1, unsigned& b2) {
    const unsigned h0 = __float_as_uint(v) & 0xffff0000u;
    const float r = v - __uint_as_float(h0);
    const unsigned h1 = __float_as_uint(r) & 0xffff0000u;
    const float r2 = r - __uint_as_float(h1);
    b0 = h0 >> 16; b1 = h1 >> 16; b2 = __float_as_uint(r2) >> 16;
}
__device__ __forceinline__ void x3_split_guarded(float v, unsigned& b0, unsigned& b1, unsigned& b2) {      // (the casts spelt as split3_bf16_cl_kernel had them: its schedule depends on it)
    const unsigned h0 = __builtin_bit_cast(unsigned, v) & 0xffff0000u;
    const bool fin = (h0 & 0x7f800000u) != 0x7f800000u;
    const float r = fin ? v - __builtin_bit_cast(float, h0) : 0.f;
    const unsigned h1 = __builtin_bit_cast(unsigned, r) & 0xffff0000u;
    const float r2 = r - __builtin_bit_cast(float, h1);
    b0 = h0 >> 16; b1 = h1 >> 16; b2 = __builtin_bit_cast(unsigned, r2) >> 16;
}

// The packers' store: the three planes of v to out[dst], out[dst + stride], out[dst + 2 * stride]
__device__ __forceinline__ void x3_store_planes(unsigned short* __restrict__ out, int64_t dst, int64_t stride, float v) {
    unsigned b0, b1, b2;
    x3_split(v, b0, b1, b2);
    out[dst] = (unsigned short)b0;
    out[dst + stride] = (unsigned short)b1;
    out[dst + 2 * stride] = (unsigned short)b2;
}

}  // namespace pgconv
