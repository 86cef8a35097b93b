// The bf16 plane stream of a 3x3 kernel from its float32 pack (bf16x3.h's split): wp32 = pg_conv2d_pack_weight's [Cin][9][CoutP32] (weight gain / flip folded
// in) -> three bf16 planes where the kernel's waves read them.  Where element (co, tap, ci) goes is the layout's business -- one struct per kernel
// (X3PackUp2 in conv2d_up2x3.h, X3PackS2 in conv2d_s2x3.h), as Wino4PackF4* for the Winograd forms:
//   static int cout_padded(int Cout)                           couts of the stream (zero beyond Cout)
//   static int64_t dst(int co, int tap, int ci, int nchunks)   index of the plane-0 value, in 16-bit words; nchunks = Cin / 16
//   static constexpr int PLANE                                 words from one plane of a value to the next
#pragma once
#include "bf16x3.h"
#include "pg_common.h"

namespace pgconv {

template <class Layout>
__global__ __launch_bounds__(256) void x3_pack_kernel(const float* __restrict__ wp32, unsigned short* __restrict__ out, int Cin, int CoutPad, int CoutP32) {
    const int nchunks = Cin / 16;
    const int64_t total = (int64_t)Cin * 9 * CoutPad;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int co = (int)(i % CoutPad), tap = (int)((i / CoutPad) % 9), ci = (int)(i / ((int64_t)CoutPad * 9));
        const float v = co < CoutP32 ? wp32[((int64_t)ci * 9 + tap) * CoutP32 + co] : 0.f;
        x3_store_planes(out, Layout::dst(co, tap, ci, nchunks), Layout::PLANE, v);
    }
}

template <class Layout>
inline int launch_x3_pack(const float* packed, void* packed_x3, int Cout, int Cin, hipStream_t s) {
    const int CoutP32 = (Cout + 31) / 32 * 32, CoutPad = Layout::cout_padded(Cout);
    int64_t blocks = ((int64_t)Cin * 9 * CoutPad + 255) / 256;
    if (blocks > (int64_t)pg::max_stream_blocks()) blocks = pg::max_stream_blocks();
    hipLaunchKernelGGL(x3_pack_kernel<Layout>, dim3((unsigned)blocks), dim3(256), 0, s, packed, (unsigned short*)packed_x3, Cin, CoutPad, CoutP32);
    return pg::launch_status();
}

}  // namespace pgconv
