// Device helpers of the uint8 NHWC -> float32 NCHW staging kernels (csrc/tryon.hip, csrc/train_fetch.hip).  One lane = 4 consecutive pixels of a
// row: the uint8 side is read as dwords (non-temporal), each float plane is written with one 16-byte non-temporal store.  `unit` is torch's GPU
// arithmetic for `u / 127.5 - 1`: a product with the rounded reciprocal, then a separately rounded subtraction (nothing here may be contracted into a
// fused multiply-add: the pragma below, which holds to the end of the including translation unit).
#pragma once
#include <cstdint>

#pragma clang fp contract(off)

namespace pg {
namespace stage {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr float kInv = 1.0f / 127.5f;            // what torch multiplies by for `t / 127.5` on a GPU tensor

__device__ __forceinline__ float unit(float u) { return u * kInv - 1.0f; }
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

template <int C>
__device__ __forceinline__ void load_px4(const uint8_t* __restrict__ p, uint32_t (&w)[C]) {      // 4 pixels x C bytes, dword aligned
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < C; i++) w[i] = __builtin_nontemporal_load(q + i);
}

__device__ __forceinline__ void store4(float* __restrict__ p, float a, float b, float c, float d) {
    __builtin_nontemporal_store(f32x4{a, b, c, d}, reinterpret_cast<f32x4*>(p));
}

}  // namespace stage
}  // namespace pg
