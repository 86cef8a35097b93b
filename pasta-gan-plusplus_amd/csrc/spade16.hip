// SPADE normalisation of the 16-bit (bf16 / fp16) channels-last route: the instance-norm statistics of a [N, H, W, C] tensor and the combine
//     y = clamp(act(((x - mean) * rstd) * (1 + gamma) + beta) * gain)
// (Spade_Norm_Block, networks.py:1713-1723, with the pre-activation of the one Spade_Conv2dLayer that consumes y, networks.py:1627-1633).
//
// Both are HBM streams, no matrix pipe: a pixel's C channels are C / 8 aligned 16-byte words, consecutive lanes take consecutive words, so every load and
// store instruction of a wave covers 1 KB of contiguous memory.
//
// Statistics, two levels, no atomics, a fixed order (bit-identical repeats):
//   level 1  one workgroup per (sample, pixel chunk): G = C / 8 lanes hold a pixel, 256 / G pixels per pass, four passes in flight.  A lane sums x - K and
//            (x - K)^2 of its 8 channels with K = the chunk's first pixel (shifted data: no cancellation when |mean| >> std), the lanes of a channel group are
//            folded through LDS in lane order, and the chunk's (mean, M2) per channel go to the workspace;
//   level 2  one thread per (n, c) folds the chunks in chunk order, again as shifted sums (shift = the first chunk's mean).
// Bytes: 2 * N * H * W * C in, 2 * 4 * N * C out (+ the workspace, 8 * N * chunks * C each way): the input stream at HBM bandwidth.
//
// Combine: one thread per (pixel, 8 channels): x and y 16 bytes, gamma and beta 16 bytes each out of the [N, H, W, 2C] output of the stacked gamma || beta
// convolution (gamma first).  Bytes: 2 * N * H * W * C * (1 + 2 + 1).  The arithmetic runs in float64 registers and is rounded once on the store: with float32
// the product and beta cancel on some elements and the result would miss one ulp of the 16-bit type; the stream hides the extra VALU work (8 bytes and about a
// dozen operations per element against ~5 TB/s).
#include "conv2d_kernel16.h"
#include "pg_common.h"

namespace pgconv16 {
namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_CHUNKS = PG_STATS16_MAX_CHUNKS;
constexpr int ST_UNROLL = 4;

template <typename T>
__device__ __forceinline__ void widen8(const u32x4 v, float* o) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
        o[2 * d] = Half16<T>::widen((unsigned short)(v[d] & 0xffff));
        o[2 * d + 1] = Half16<T>::widen((unsigned short)(v[d] >> 16));
    }
}

// level 1: grid (chunks, N); ws[((n * chunks + chunk) * 2 + {0: mean, 1: M2}) * C + c]
template <typename T>
__global__ __launch_bounds__(ST_THREADS) void stats16_chunk_kernel(const unsigned short* __restrict__ x, float* __restrict__ ws, int C, int64_t HW, int64_t chunk) {
    __shared__ float red[ST_THREADS * 16];
    const int G = C >> 3, R = ST_THREADS / G;                        // 16-byte groups per pixel, pixels per pass
    const int t = threadIdx.x, row = t / G, g = t - row * G;
    const bool active = row < R;
    const int n = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    const int64_t p1 = p0 + chunk < HW ? p0 + chunk : HW;            // p0 < HW: the host launches no empty chunk
    const unsigned short* xn = x + (int64_t)n * HW * C;
    float K[8], s[8], q[8];
#pragma unroll
    for (int d = 0; d < 8; d++) s[d] = q[d] = 0.f;
    if (active) {
        widen8<T>(*(const u32x4*)(xn + p0 * C + g * 8), K);
        int64_t p = p0 + row;
        for (; p + (int64_t)(ST_UNROLL - 1) * R < p1; p += (int64_t)ST_UNROLL * R) {
            u32x4 v[ST_UNROLL];
#pragma unroll
            for (int u = 0; u < ST_UNROLL; u++) v[u] = *(const u32x4*)(xn + (p + (int64_t)u * R) * C + g * 8);
#pragma unroll
            for (int u = 0; u < ST_UNROLL; u++) {
                float f[8];
                widen8<T>(v[u], f);
#pragma unroll
                for (int d = 0; d < 8; d++) { const float a = f[d] - K[d]; s[d] += a; q[d] = fmaf(a, a, q[d]); }
            }
        }
        for (; p < p1; p += R) {
            float f[8];
            widen8<T>(*(const u32x4*)(xn + p * C + g * 8), f);
#pragma unroll
            for (int d = 0; d < 8; d++) { const float a = f[d] - K[d]; s[d] += a; q[d] = fmaf(a, a, q[d]); }
        }
    }
#pragma unroll
    for (int d = 0; d < 8; d++) { red[t * 16 + d] = s[d]; red[t * 16 + 8 + d] = q[d]; }
    __syncthreads();
    const float cnt = (float)(p1 - p0);
    float* out = ws + ((int64_t)n * gridDim.x + blockIdx.x) * 2 * C;
    for (int c = t; c < C; c += ST_THREADS) {
        const int cg = c >> 3, d = c & 7;
        float S = 0.f, Q = 0.f;
        for (int r = 0; r < R; r++) { S += red[(r * G + cg) * 16 + d]; Q += red[(r * G + cg) * 16 + 8 + d]; }
        const float k = Half16<T>::widen(xn[p0 * C + c]);
        out[c] = k + S / cnt;
        out[C + c] = fmaxf(Q - S * (S / cnt), 0.f);
    }
}

// level 2: one thread per (n, c), chunks in order
__global__ __launch_bounds__(256) void stats16_fold_kernel(const float* __restrict__ ws, float* __restrict__ mean, float* __restrict__ rstd, int NC, int C, int chunks,
                                                           int64_t HW, int64_t chunk, float eps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    const int n = i / C, c = i - n * C;
    const float* w = ws + (int64_t)n * chunks * 2 * C + c;
    const float K = w[0];
    float S = 0.f, Q = 0.f;
    for (int k = 0; k < chunks; k++) {
        const int64_t p0 = (int64_t)k * chunk;
        const float cnt = (float)((p0 + chunk < HW ? p0 + chunk : HW) - p0);
        const float d = w[(int64_t)k * 2 * C] - K;
        S = fmaf(cnt, d, S);
        Q += w[(int64_t)k * 2 * C + C] + cnt * d * d;
    }
    const float ms = S / (float)HW;
    const float var = fmaxf(Q / (float)HW - ms * ms, 0.f);
    mean[i] = K + ms;
    rstd[i] = 1.0f / sqrtf(var + eps);
}

// float64 -> 16 bit with ONE rounding: float32 by round-to-odd (truncate, set the last bit when inexact), which the nearest-even conversion to the 11- or
// 8-bit significand then rounds as if it had seen the float64 value
template <typename T>
__device__ __forceinline__ unsigned short narrow(double v) {
    float f = (float)v;
    const double r = v - (double)f;
    if (r != 0.0 && fabs(v) < 3.0e38) {
        unsigned b = __builtin_bit_cast(unsigned, f);
        if ((r < 0.0 && f > 0.f) || (r > 0.0 && f < 0.f)) b -= 1u;      // the conversion rounded away from zero
        if (f == 0.f) b = v < 0.0 ? 0x80000000u : 0u;
        f = __builtin_bit_cast(float, b | 1u);
    }
    return (unsigned short)(Half16<T>::pack(f, 0.f) & 0xffff);
}

// one thread per (pixel, 8 channels); total = N * HW * G < 2^31
template <typename T>
__global__ __launch_bounds__(256) void spade_combine16_kernel(const unsigned short* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const unsigned short* __restrict__ gb, unsigned short* __restrict__ y, unsigned G, unsigned HW,
                                                              unsigned total, int act, float alpha, float gain, float clamp) {
    const double slope = act == PG_ACT_RELU ? 0.0 : (act == PG_ACT_LRELU ? (double)alpha : 1.0);
    const double cl = clamp >= 0.f ? (double)clamp : (double)__builtin_inff();
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned pix = i / G, g = i - pix * G, n = pix / HW;
        const u32x4 xv = *(const u32x4*)(x + (int64_t)i * 8);
        const u32x4 gv = *(const u32x4*)(gb + ((int64_t)pix * 2 * G + g) * 8);
        const u32x4 bv = *(const u32x4*)(gb + ((int64_t)pix * 2 * G + G + g) * 8);
        const float* mp = mean + (int64_t)n * G * 8 + g * 8;
        const float* rp = rstd + (int64_t)n * G * 8 + g * 8;
        const f32x4 m0 = *(const f32x4*)mp, m1 = *(const f32x4*)(mp + 4), r0 = *(const f32x4*)rp, r1 = *(const f32x4*)(rp + 4);
        float xf[8], gf[8], bf[8];
        widen8<T>(xv, xf);
        widen8<T>(gv, gf);
        widen8<T>(bv, bf);
        unsigned short o[8];
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const double m = d < 4 ? m0[d & 3] : m1[d & 3], r = d < 4 ? r0[d & 3] : r1[d & 3];
            double v = ((double)xf[d] - m) * r * (1.0 + (double)gf[d]) + (double)bf[d];
            v = (v < 0.0 ? v * slope : v) * (double)gain;
            if (clamp >= 0.f) v = (v > -cl && v < cl) ? v : (v >= 0.0 ? cl : -cl);      // the plugin's select: a NaN becomes -clamp, as in every fused tail (pg_common.h)
            o[d] = narrow<T>(v);
        }
        u32x4 ov;
#pragma unroll
        for (int d = 0; d < 4; d++) ov[d] = (unsigned)o[2 * d] | ((unsigned)o[2 * d + 1] << 16);
        *(u32x4*)(y + (int64_t)i * 8) = ov;
    }
}

}  // namespace
}  // namespace pgconv16

using namespace pgconv16;

PG_EXPORT int pg_instance_norm_stats_cl16(const void* x, float* mean, float* rstd, float* workspace, int dtype, int N, int64_t HW, int C, float eps, void* stream) {
    if (!x || !mean || !rstd || !workspace || N <= 0 || HW <= 0 || C <= 0) return PG_ERR_INVALID_ARG;
    if (dtype != PG_BF16 && dtype != PG_F16) return PG_ERR_INVALID_ARG;
    if (C % 16 != 0 || C > 8 * ST_THREADS || !pg::aligned16(x) || N > 65535) return PG_ERR_UNSUPPORTED;
    if ((int64_t)N * C > 0x7fffffffLL) return PG_ERR_TOO_LARGE;
    const int R = ST_THREADS / (C / 8);
    // >= ST_UNROLL passes per chunk, at most ST_MAX_CHUNKS chunks; a function of the shape alone (the reduction order must not depend on the device)
    int64_t chunks = HW / ((int64_t)ST_UNROLL * R);
    chunks = chunks < 1 ? 1 : (chunks > ST_MAX_CHUNKS ? ST_MAX_CHUNKS : chunks);
    const int64_t chunk = (HW + chunks - 1) / chunks;
    chunks = (HW + chunk - 1) / chunk;                               // no empty chunk
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks, (unsigned)N);
    if (dtype == PG_BF16)
        hipLaunchKernelGGL(stats16_chunk_kernel<bf16_t>, grid, dim3(ST_THREADS), 0, s, (const unsigned short*)x, workspace, C, HW, chunk);
    else
        hipLaunchKernelGGL(stats16_chunk_kernel<f16_t>, grid, dim3(ST_THREADS), 0, s, (const unsigned short*)x, workspace, C, HW, chunk);
    int st = pg::launch_status();
    if (st != PG_OK) return st;
    const int NC = N * C;
    hipLaunchKernelGGL(stats16_fold_kernel, dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, s, workspace, mean, rstd, NC, C, (int)chunks, HW, chunk, eps);
    return pg::launch_status();
}

PG_EXPORT int pg_spade_combine_cl16(const void* x, const float* mean, const float* rstd, const void* gamma_beta, void* y, int dtype, int N, int64_t HW, int C,
                                    int act, float alpha, float gain, float clamp, void* stream) {
    if (!x || !mean || !rstd || !gamma_beta || !y || N <= 0 || HW <= 0 || C <= 0) return PG_ERR_INVALID_ARG;
    if (dtype != PG_BF16 && dtype != PG_F16) return PG_ERR_INVALID_ARG;
    if (act == 0) act = PG_ACT_LINEAR;
    if (act != PG_ACT_LINEAR && act != PG_ACT_RELU && act != PG_ACT_LRELU) return PG_ERR_UNSUPPORTED;
    if (C % 16 != 0 || !pg::aligned16(x) || !pg::aligned16(gamma_beta) || !pg::aligned16(y) || !pg::aligned16(mean) || !pg::aligned16(rstd)) return PG_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)N * HW * (C / 8);
    if (total > 0x7fffffffLL || HW > 0x7fffffffLL) return PG_ERR_TOO_LARGE;
    int64_t blocks = (total + 255) / 256;
    if (blocks > pg::max_stream_blocks()) blocks = pg::max_stream_blocks();
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PG_BF16)
        hipLaunchKernelGGL(spade_combine16_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, (const unsigned short*)x, mean, rstd,
                           (const unsigned short*)gamma_beta, (unsigned short*)y, (unsigned)(C / 8), (unsigned)HW, (unsigned)total, act, alpha, gain, clamp);
    else
        hipLaunchKernelGGL(spade_combine16_kernel<f16_t>, dim3((unsigned)blocks), dim3(256), 0, s, (const unsigned short*)x, mean, rstd,
                           (const unsigned short*)gamma_beta, (unsigned short*)y, (unsigned)(C / 8), (unsigned)HW, (unsigned)total, act, alpha, gain, clamp);
    return pg::launch_status();
}
