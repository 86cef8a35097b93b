// Folded 1x1 heads of the fp32 stack: a linear 1x1 convolution over [x ; x2] (merge_conv of a style block, networks.py:2160-2162) followed by the modulated
// 1x1 ToRGB / parsing heads (networks.py:287-316, demodulate=False) is, per sample, ONE linear map of the merge inputs:
//     head_n([x ; x2]) = (W_head o s_n) (g W_m [x ; x2] + b_m) + b_head = W'_n [x ; x2] + b'_n,      W'_n [Cout][C1 + C2], b'_n [Cout].
// Where nothing else reads the merged feature map (the last style block), it need not exist: conv1x1_fold_prep_kernel composes W'_n / b'_n (a few hundred
// kFLOP, accumulated in float64 so that the composed weights are correctly rounded float32), and conv1x1_fold_heads_kernel streams the two inputs once.
//   * a thread owns 4 adjacent pixels and walks the channels of x, then of x2, with 16-byte loads (one contiguous 1 KB per wave instruction, 8 channel planes
//     in flight), like conv1x1_small_f32_kernel (conv2d.hip);
//   * the sample's weights sit in LDS as [C1 + C2][CP] (CP = Cout rounded up to 4, zero-padded): CP / 4 broadcast reads per channel; all Cout x 4 sums stay
//     in registers;
//   * outputs [0, c_a) go to y_a and [c_a, Cout) to y_b (rgb and parsing stay the two dense tensors they were); bias, clamp and the skip image (added to the
//     first n_skip channels, after the clamp, as the head kernel does) ride in the tail.
// HBM-bound: 4 * (C1 + C2) bytes read + 4 * Cout written (+ 4 * n_skip skip image) per pixel.
#include "pg_common.h"

#ifndef PG_FOLD_MIN_WAVES
#define PG_FOLD_MIN_WAVES 1      // waves per SIMD the register allocation of the streaming kernel is held to (-D: development variants)
#endif
#ifndef PG_FOLD_UNROLL
#define PG_FOLD_UNROLL 8         // channel planes in flight per thread
#endif

namespace {
typedef float f32x4s __attribute__((ext_vector_type(4)));

// w_out[n][o][c] = sum_k wh[o][k] * s[n][k] * wm[k][c],   b_out[n][o] = sum_k wh[o][k] * s[n][k] * bm[k] + bh[o];  grid (Cout, N), column C = the bias
__global__ __launch_bounds__(256) void conv1x1_fold_prep_kernel(const float* __restrict__ wm, const float* __restrict__ bm, const float* __restrict__ wh,
                                                                const float* __restrict__ bh, const float* __restrict__ styles, float* __restrict__ w_out,
                                                                float* __restrict__ b_out, int Cm, int C, int Cout) {
    const int o = blockIdx.x, n = blockIdx.y;
    const float* who = wh + (int64_t)o * Cm;
    const float* sn = styles ? styles + (int64_t)n * Cm : nullptr;
    for (int c = threadIdx.x; c <= C; c += 256) {
        double acc = 0.0;
        if (c < C) {
            for (int k = 0; k < Cm; k++) acc += (double)who[k] * (double)(sn ? sn[k] : 1.f) * (double)wm[(int64_t)k * C + c];
            w_out[((int64_t)n * Cout + o) * C + c] = (float)acc;
        } else {
            if (bm)
                for (int k = 0; k < Cm; k++) acc += (double)who[k] * (double)(sn ? sn[k] : 1.f) * (double)bm[k];
            b_out[(int64_t)n * Cout + o] = (float)(acc + (double)(bh ? bh[o] : 0.f));
        }
    }
}

template <int CP>      // accumulator rows: Cout rounded up to a multiple of 4
__global__ __launch_bounds__(256, PG_FOLD_MIN_WAVES) void conv1x1_fold_heads_kernel(const float* __restrict__ x, const float* __restrict__ x2, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, const float* __restrict__ skip, float* __restrict__ ya,
                                                                 float* __restrict__ yb, int C1, int C2, int64_t HW4, int Cout, int c_a, int n_skip, float clamp) {
    extern __shared__ __attribute__((aligned(16))) float wl[];          // [C1 + C2][CP]
    const int n = blockIdx.y, C = C1 + C2;
    const float* wn = w + (int64_t)n * Cout * C;
    for (int e = threadIdx.x; e < CP * C; e += 256) {
        const int c = e / CP, o = e % CP;
        wl[e] = o < Cout ? wn[o * C + c] : 0.f;
    }
    __syncthreads();
    const float cl = pg::clamp_bound(clamp);
    const f32x4s* xa = (const f32x4s*)x + (int64_t)n * C1 * HW4;
    const f32x4s* xb = (const f32x4s*)x2 + (int64_t)n * C2 * HW4;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW4; p += (int64_t)gridDim.x * 256) {
        f32x4s acc[CP];
#pragma unroll
        for (int o = 0; o < CP; o++) acc[o] = (f32x4s){0.f, 0.f, 0.f, 0.f};
        auto mac = [&](const f32x4s& xv, const float* wc) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < CP / 4; q++) {
                const f32x4s wq = *(const f32x4s*)(wc + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; j++) acc[4 * q + j] += xv * wq[j];
            }
        };
        auto walk = [&](const f32x4s* xs, int Cs, const float* ws) __attribute__((always_inline)) {
            int c0 = 0;
            for (; c0 + PG_FOLD_UNROLL <= Cs; c0 += PG_FOLD_UNROLL) {     // PG_FOLD_UNROLL channel planes in flight, no branch between them
                f32x4s v[PG_FOLD_UNROLL];
#pragma unroll
                for (int u = 0; u < PG_FOLD_UNROLL; u++) v[u] = xs[(int64_t)(c0 + u) * HW4 + p];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < PG_FOLD_UNROLL; u++) mac(v[u], ws + (c0 + u) * CP);
            }
            for (; c0 < Cs; c0++) mac(xs[(int64_t)c0 * HW4 + p], ws + c0 * CP);
        };
        walk(xa, C1, wl);
        walk(xb, C2, wl + C1 * CP);
#pragma unroll
        for (int o = 0; o < CP; o++) {
            if (o < Cout) {
                f32x4s r = acc[o] + bias[(int64_t)n * Cout + o];
#pragma unroll
                for (int e = 0; e < 4; e++) r[e] = fminf(fmaxf(r[e], -cl), cl);
                if (o < n_skip) r += ((const f32x4s*)skip)[((int64_t)n * n_skip + o) * HW4 + p];
                if (o < c_a) ((f32x4s*)ya)[((int64_t)n * c_a + o) * HW4 + p] = r;
                else ((f32x4s*)yb)[((int64_t)n * (Cout - c_a) + (o - c_a)) * HW4 + p] = r;
            }
        }
    }
}
}  // namespace

PG_EXPORT int pg_conv1x1_fold_prep(const float* wm, const float* bm, const float* wh, const float* bh, const float* styles, float* w_out, float* b_out,
                                   int N, int Cm, int C, int Cout, void* stream) {
    if (!wm || !wh || !w_out || !b_out || N <= 0 || Cm <= 0 || C <= 0 || Cout <= 0) return PG_ERR_INVALID_ARG;
    if (N > 65535) return PG_ERR_TOO_LARGE;
    hipLaunchKernelGGL(conv1x1_fold_prep_kernel, dim3((unsigned)Cout, (unsigned)N), dim3(256), 0, (hipStream_t)stream, wm, bm, wh, bh, styles, w_out, b_out, Cm, C, Cout);
    return pg::launch_status();
}

PG_EXPORT int pg_conv1x1_fold_heads(const float* x, const float* x2, const float* w, const float* bias, const float* skip, float* y_a, float* y_b,
                                    int N, int C1, int C2, int64_t HW, int Cout, int c_a, int n_skip, float clamp, void* stream) {
    if (!x || !w || !bias || !y_a || N <= 0 || C1 <= 0 || C2 < 0 || HW <= 0 || Cout <= 0 || c_a <= 0 || c_a > Cout || n_skip < 0 || n_skip > Cout) return PG_ERR_INVALID_ARG;
    if ((C2 > 0 && !x2) || (c_a < Cout && !y_b) || (n_skip > 0 && !skip)) return PG_ERR_INVALID_ARG;
    const int CP = (Cout + 3) / 4 * 4;
    const size_t lds = (size_t)(C1 + C2) * CP * sizeof(float);
    if (Cout > 16 || HW % 4 != 0 || !pg::aligned16(x) || (C2 > 0 && !pg::aligned16(x2)) || !pg::aligned16(y_a) || (c_a < Cout && !pg::aligned16(y_b)) ||
        (n_skip > 0 && !pg::aligned16(skip)) || lds > 64 * 1024)
        return PG_ERR_UNSUPPORTED;
    if (N > 65535) return PG_ERR_TOO_LARGE;
    const int64_t HW4 = HW / 4;
    int64_t bx = (HW4 + 255) / 256;
    const int64_t cap = (int64_t)pg::num_cu() * 8 / N + 1;
    if (bx > cap) bx = cap;
    const dim3 grid((unsigned)bx, (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
#define PG_FOLD(P) case P: hipLaunchKernelGGL((conv1x1_fold_heads_kernel<P>), grid, dim3(256), lds, s, x, x2, w, bias, skip, y_a, y_b, C1, C2, HW4, Cout, c_a, n_skip, clamp); break;
    switch (CP) { PG_FOLD(4) PG_FOLD(8) PG_FOLD(12) PG_FOLD(16) }
#undef PG_FOLD
    return pg::launch_status();
}
