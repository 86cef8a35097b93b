// Packing of the training driver's image snapshots on gfx950 (training/snapshot_grid.py; the reference's save_image_grid,
// training_loop_fullbody.py:313-340, with the parsing colours of :709-719): a chunk of generator outputs -> its cells of the two uint8 grid images.
// Image bytes: clip(rint((x + 1) * 127.5), 0, 255) with the float32 operations NumPy runs, in its order, nothing contracted into a fused multiply-add
// (the pragma below); NaN -> 0.  Parsing bytes: grey[first index of the maximal logit].
// A memory-bound stream: one lane = 4 consecutive pixels of a row -> 16-byte loads per plane, three dword stores per grid.
#include "pg_common.h"
#include "pg_stage.h"
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

using namespace pg::stage;

constexpr int kMaxClasses = 16;

__device__ __forceinline__ uint32_t image_byte(float x) {
    float v = rintf((x + 1.0f) * 127.5f);                            // round half to even, as np.rint
    if (v != v) return 0u;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return (uint32_t)(int)v;
}

__global__ __launch_bounds__(256) void snapshot_cells_u8_kernel(const float* __restrict__ fin, const float* __restrict__ par, const uint8_t* __restrict__ grey,
                                                                uint8_t* __restrict__ grid_img, uint8_t* __restrict__ grid_par, int n, int C, int H, int W, int gw,
                                                                int first_cell) {
    __shared__ uint32_t s_grey[kMaxClasses];
    if ((int)threadIdx.x < C) s_grey[threadIdx.x] = grey[threadIdx.x];
    __syncthreads();
    const int qpr = W / 4;                                           // quads per cell row
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)n * H * qpr) return;
    const int x = (int)(q % qpr) * 4;
    const int y = (int)((q / qpr) % H);
    const int i = (int)(q / ((int64_t)qpr * H));
    const int64_t HW = (int64_t)H * W;
    const int cell = first_cell + i;
    const int64_t row_bytes = (int64_t)(gw + 1) * W * 3;
    const int64_t off = ((int64_t)(1 + cell / gw) * H + y) * row_bytes + ((int64_t)(1 + cell % gw) * W + x) * 3;

    uint32_t o[3] = {0u, 0u, 0u};
    const float* f = fin + (int64_t)i * 3 * HW + (int64_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(f + c * HW));
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int b = 3 * k + c;
            o[b >> 2] |= image_byte(vv[k]) << ((b & 3) * 8);
        }
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(grid_img + off);
#pragma unroll
    for (int j = 0; j < 3; j++) __builtin_nontemporal_store(o[j], d + j);

    const float* g = par + (int64_t)i * C * HW + (int64_t)y * W + x;
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};    // (a NaN logit compares false: it never wins; all NaN or -inf -> class 0)
    int arg[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; c++) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + c * HW));
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (vv[k] > best[k]) { best[k] = vv[k]; arg[k] = c; }     // strict: the first index of the maximum stays
    }
    uint32_t p[3] = {0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 12; b++) p[b >> 2] |= s_grey[arg[b / 3]] << ((b & 3) * 8);
    uint32_t* dp = reinterpret_cast<uint32_t*>(grid_par + off);
#pragma unroll
    for (int j = 0; j < 3; j++) __builtin_nontemporal_store(p[j], dp + j);
}

}  // namespace

PG_EXPORT int pg_snapshot_grid_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_snapshot_cells_u8(const float* finetune_img, const float* pred_parsing, const unsigned char* grey, unsigned char* grid_img,
                                   unsigned char* grid_parsing, int n, int C, int H, int W, int gh, int gw, int first_cell, void* stream) {
    if (!finetune_img || !pred_parsing || !grey || !grid_img || !grid_parsing || n <= 0 || H <= 0 || W <= 0 || gh <= 0 || gw <= 0) return PG_ERR_INVALID_ARG;
    if (C < 1 || C > kMaxClasses) return PG_ERR_INVALID_ARG;
    if (first_cell < 0 || (int64_t)first_cell + n > (int64_t)gh * gw) return PG_ERR_INVALID_ARG;
    if (W % 4 || !pg::aligned16(finetune_img) || !pg::aligned16(pred_parsing) ||
        (reinterpret_cast<uintptr_t>(grid_img) | reinterpret_cast<uintptr_t>(grid_parsing)) & 3u)
        return PG_ERR_UNSUPPORTED;
    const int64_t quads = (int64_t)n * H * (W / 4);
    if ((quads + 255) / 256 > 0x7fffffffLL || (int64_t)H * W > 0x3fffffffLL) return PG_ERR_TOO_LARGE;
    hipLaunchKernelGGL(snapshot_cells_u8_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, finetune_img, pred_parsing, grey,
                       grid_img, grid_parsing, n, C, H, W, gw, first_cell);
    return pg::launch_status();
}
