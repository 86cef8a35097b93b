// The two operators of the VGG19 perceptual loss (training/vgg_loss.py) that are not convolutions, on gfx950: the 2x2 max-pool between the trunk's
// stages and the feature-space L1 means, each with its backward.  float32, dense NCHW.  All four are memory-bound streams: on the aligned path one lane
// moves 16-byte vectors (a pool lane owns four windows: 4 x 16 B in, 16 B out), on odd widths / misaligned bases a plain path moves single floats.
//   pool      y = max over the window, aten's rule: scan the window row-major from -inf, take v when v > max or v is NaN.
//   pool bwd  the same scan again on x (no index tensor); dx = dy at the chosen element, 0 elsewhere, and 0 in a trailing odd row / column: the
//             kernel writes every element of dx.
//   l1 sum    G groups of x stacked on the batch axis against ONE y (read once for all groups): per-block partial sums in a fixed order, then one
//             small block per group adds the partials in double -> out[g] = sum * scale.  No atomics: bit-identical run to run.
//   l1 grad   dx_g = sgn(x_g - y) * (s[g] / denom), s on the device.
#include "pg_common.h"
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMaxGroups = 8;            // == PG_L1_PAIR_MAX_GROUPS

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// aten's max_pool2d scan of one window {a b / c d}: returns the maximum, `k` = its position 0..3 (first maximum in row-major order; a NaN wins, the
// last NaN stays)
__device__ __forceinline__ float scan4(float a, float b, float c, float d, int& k) {
    float m = -INFINITY;
    k = 0;
    if (a > m || a != a) { m = a; k = 0; }
    if (b > m || b != b) { m = b; k = 1; }
    if (c > m || c != c) { m = c; k = 2; }
    if (d > m || d != d) { m = d; k = 3; }
    return m;
}

// ---------------------------------------------------------------- pool, aligned path: W % 8 == 0, one lane = 4 windows of one output row
__global__ __launch_bounds__(kThreads) void maxpool_fwd_v4(const float* __restrict__ x, float* __restrict__ y, int64_t lanes, int H, int W, int Ho) {
    const int qpr = W >> 3;                                           // lanes per output row
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < lanes; q += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(q % qpr);
        const int64_t r = q / qpr;                                    // plane * Ho + i
        const int i = (int)(r % Ho);
        const int64_t plane = r / Ho;
        const float* p = x + (plane * H + 2 * i) * W + 8 * j;
        const f32x4 a0 = ld4(p), a1 = ld4(p + 4), b0 = ld4(p + W), b1 = ld4(p + W + 4);
        int k;
        f32x4 o;
        o.x = scan4(a0.x, a0.y, b0.x, b0.y, k);
        o.y = scan4(a0.z, a0.w, b0.z, b0.w, k);
        o.z = scan4(a1.x, a1.y, b1.x, b1.y, k);
        o.w = scan4(a1.z, a1.w, b1.z, b1.w, k);
        st4(y + r * (W >> 1) + 4 * j, o);
    }
}

// rows = planes * ceil(H / 2): the last row of a plane with odd H is its dropped input row, written as zeros
__global__ __launch_bounds__(kThreads) void maxpool_bwd_v4(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int64_t lanes,
                                                           int H, int W, int Ho) {
    const int qpr = W >> 3;
    const int Hc = (H + 1) >> 1;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < lanes; q += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(q % qpr);
        const int64_t r = q / qpr;
        const int i = (int)(r % Hc);
        const int64_t plane = r / Hc;
        const int64_t off = (plane * H + 2 * i) * W + 8 * j;
        if (i >= Ho) {                                                // H odd: the row no window covers
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            st4(dx + off, z);
            st4(dx + off + 4, z);
            continue;
        }
        const float* p = x + off;
        const f32x4 a0 = ld4(p), a1 = ld4(p + 4), b0 = ld4(p + W), b1 = ld4(p + W + 4);
        const f32x4 g = ld4(dy + (plane * Ho + i) * (W >> 1) + 4 * j);
        int k0, k1, k2, k3;
        scan4(a0.x, a0.y, b0.x, b0.y, k0);
        scan4(a0.z, a0.w, b0.z, b0.w, k1);
        scan4(a1.x, a1.y, b1.x, b1.y, k2);
        scan4(a1.z, a1.w, b1.z, b1.w, k3);
        f32x4 t0, t1, u0, u1;
        t0.x = k0 == 0 ? g.x : 0.f; t0.y = k0 == 1 ? g.x : 0.f; u0.x = k0 == 2 ? g.x : 0.f; u0.y = k0 == 3 ? g.x : 0.f;
        t0.z = k1 == 0 ? g.y : 0.f; t0.w = k1 == 1 ? g.y : 0.f; u0.z = k1 == 2 ? g.y : 0.f; u0.w = k1 == 3 ? g.y : 0.f;
        t1.x = k2 == 0 ? g.z : 0.f; t1.y = k2 == 1 ? g.z : 0.f; u1.x = k2 == 2 ? g.z : 0.f; u1.y = k2 == 3 ? g.z : 0.f;
        t1.z = k3 == 0 ? g.w : 0.f; t1.w = k3 == 1 ? g.w : 0.f; u1.z = k3 == 2 ? g.w : 0.f; u1.w = k3 == 3 ? g.w : 0.f;
        float* d = dx + off;
        st4(d, t0);
        st4(d + 4, t1);
        st4(d + W, u0);
        st4(d + W + 4, u1);
    }
}

// ---------------------------------------------------------------- pool, plain path: one lane = one window (any H, W, alignment)
__global__ __launch_bounds__(kThreads) void maxpool_fwd_plain(const float* __restrict__ x, float* __restrict__ y, int64_t total, int H, int W, int Ho, int Wo) {
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < total; q += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(q % Wo);
        const int64_t r = q / Wo;
        const int i = (int)(r % Ho);
        const int64_t plane = r / Ho;
        const float* p = x + (plane * H + 2 * i) * W + 2 * j;
        int k;
        y[q] = scan4(p[0], p[1], p[W], p[W + 1], k);
    }
}

// one lane = one 2x2 cell of the ceil(H/2) x ceil(W/2) cover of dx; cells (partly) outside the pooled extent are the dropped row / column -> zeros
__global__ __launch_bounds__(kThreads) void maxpool_bwd_plain(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int64_t total,
                                                              int H, int W, int Ho, int Wo) {
    const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < total; q += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(q % Wc);
        const int64_t r = q / Wc;
        const int i = (int)(r % Hc);
        const int64_t plane = r / Hc;
        const int64_t off = (plane * H + 2 * i) * W + 2 * j;
        float* d = dx + off;
        if (i < Ho && j < Wo) {
            const float* p = x + off;
            const float g = dy[(plane * Ho + i) * Wo + j];
            int k;
            scan4(p[0], p[1], p[W], p[W + 1], k);
            d[0] = k == 0 ? g : 0.f;
            d[1] = k == 1 ? g : 0.f;
            d[W] = k == 2 ? g : 0.f;
            d[W + 1] = k == 3 ? g : 0.f;
        } else {
            const bool col2 = 2 * j + 1 < W, row2 = 2 * i + 1 < H;
            d[0] = 0.f;
            if (col2) d[1] = 0.f;
            if (row2) {
                d[W] = 0.f;
                if (col2) d[W + 1] = 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------- L1 between G stacked groups and one y
__device__ __forceinline__ float block_sum(float v, float* s_red) {          // fixed order: wave butterfly, then the 4 waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[wave] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// partials[g * gridDim.x + block] = this block's share of sum |x_g - y|.  VEC = 4: m % 4 == 0 and 16-byte aligned bases; VEC = 1: anything.
template <int VEC>
__global__ __launch_bounds__(kThreads) void l1_pair_partial(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ partials, int G,
                                                            int64_t m) {
    __shared__ float s_red[4];
    float acc[kMaxGroups][VEC];
#pragma unroll
    for (int g = 0; g < kMaxGroups; g++)
#pragma unroll
        for (int e = 0; e < VEC; e++) acc[g][e] = 0.f;
    const int64_t units = m / VEC;
    for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += (int64_t)gridDim.x * kThreads) {
        float yv[VEC];
        if (VEC == 4) {
            const f32x4 t = ld4(y + u * 4);
            yv[0] = t.x; yv[1 % VEC] = t.y; yv[2 % VEC] = t.z; yv[3 % VEC] = t.w;
        } else {
            yv[0] = y[u];
        }
#pragma unroll
        for (int g = 0; g < kMaxGroups; g++) {
            if (g < G) {
                const float* xg = x + (int64_t)g * m + u * VEC;
                if (VEC == 4) {
                    const f32x4 t = ld4(xg);
                    acc[g][0] += fabsf(t.x - yv[0]);
                    acc[g][1 % VEC] += fabsf(t.y - yv[1 % VEC]);
                    acc[g][2 % VEC] += fabsf(t.z - yv[2 % VEC]);
                    acc[g][3 % VEC] += fabsf(t.w - yv[3 % VEC]);
                } else {
                    acc[g][0] += fabsf(xg[0] - yv[0]);
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kMaxGroups; g++) {
        if (g < G) {                                                  // (G is uniform over the grid: every lane reaches the barriers)
            float v = acc[g][0];
            if (VEC == 4) v = (acc[g][0] + acc[g][1 % VEC]) + (acc[g][2 % VEC] + acc[g][3 % VEC]);
            v = block_sum(v, s_red);
            if (threadIdx.x == 0) partials[(int64_t)g * gridDim.x + blockIdx.x] = v;
        }
    }
}

// one block per group: the `nb` partials of group g, added in double in a fixed order
__global__ __launch_bounds__(kThreads) void l1_pair_final(const float* __restrict__ partials, float* __restrict__ out, int nb, double scale) {
    __shared__ double s_acc[kThreads];
    const float* p = partials + (int64_t)blockIdx.x * nb;
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += kThreads) v += (double)p[i];
    s_acc[threadIdx.x] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(s_acc[0] * scale);
}

__device__ __forceinline__ float sgn_times(float d, float s) {
    const float sg = d != d ? d : (float)((d > 0.f) - (d < 0.f));     // sgn(0) = 0; a NaN difference stays NaN, as in aten's abs backward
    return sg * s;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void l1_pair_grad(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ s,
                                                         float* __restrict__ dx, int G, int64_t m, float denom) {
    float sc[kMaxGroups];
#pragma unroll
    for (int g = 0; g < kMaxGroups; g++) sc[g] = g < G ? s[g] / denom : 0.f;
    const int64_t units = m / VEC;
    for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += (int64_t)gridDim.x * kThreads) {
        if (VEC == 4) {
            const f32x4 t = ld4(y + u * 4);
#pragma unroll
            for (int g = 0; g < kMaxGroups; g++) {
                if (g < G) {
                    const int64_t o = (int64_t)g * m + u * 4;
                    const f32x4 v = ld4(x + o);
                    f32x4 r;
                    r.x = sgn_times(v.x - t.x, sc[g]);
                    r.y = sgn_times(v.y - t.y, sc[g]);
                    r.z = sgn_times(v.z - t.z, sc[g]);
                    r.w = sgn_times(v.w - t.w, sc[g]);
                    st4(dx + o, r);
                }
            }
        } else {
            const float t = y[u];
#pragma unroll
            for (int g = 0; g < kMaxGroups; g++) {
                if (g < G) {
                    const int64_t o = (int64_t)g * m + u;
                    dx[o] = sgn_times(x[o] - t, sc[g]);
                }
            }
        }
    }
}

inline unsigned stream_grid(int64_t lanes) {
    const int64_t blocks = (lanes + kThreads - 1) / kThreads;
    const int64_t cap = pg::max_stream_blocks();
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

inline bool pool_args_ok(const void* a, const void* b, int64_t planes, int h, int w) { return a && b && planes > 0 && h > 0 && w > 0; }

}  // namespace

PG_EXPORT int pg_vgg_loss_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_maxpool2x2(const float* x, float* y, int64_t planes, int h, int w, void* stream) {
    if (!pool_args_ok(x, y, planes, h, w) || h < 2 || w < 2) return PG_ERR_INVALID_ARG;
    if (planes > (INT64_MAX / 4) / ((int64_t)h * w)) return PG_ERR_TOO_LARGE;
    const int ho = h / 2, wo = w / 2;
    if (w % 8 == 0 && pg::aligned16(x) && pg::aligned16(y)) {
        const int64_t lanes = planes * ho * (w / 8);
        hipLaunchKernelGGL(maxpool_fwd_v4, dim3(stream_grid(lanes)), dim3(kThreads), 0, (hipStream_t)stream, x, y, lanes, h, w, ho);
    } else {
        const int64_t total = planes * ho * wo;
        hipLaunchKernelGGL(maxpool_fwd_plain, dim3(stream_grid(total)), dim3(kThreads), 0, (hipStream_t)stream, x, y, total, h, w, ho, wo);
    }
    return pg::launch_status();
}

PG_EXPORT int pg_maxpool2x2_backward(const float* x, const float* dy, float* dx, int64_t planes, int h, int w, void* stream) {
    if (!pool_args_ok(x, dx, planes, h, w) || !dy || h < 2 || w < 2) return PG_ERR_INVALID_ARG;
    if (planes > (INT64_MAX / 4) / ((int64_t)h * w)) return PG_ERR_TOO_LARGE;
    const int ho = h / 2, wo = w / 2, hc = (h + 1) / 2, wc = (w + 1) / 2;
    if (w % 8 == 0 && pg::aligned16(x) && pg::aligned16(dy) && pg::aligned16(dx)) {
        const int64_t lanes = planes * hc * (w / 8);
        hipLaunchKernelGGL(maxpool_bwd_v4, dim3(stream_grid(lanes)), dim3(kThreads), 0, (hipStream_t)stream, x, dy, dx, lanes, h, w, ho);
    } else {
        const int64_t total = planes * hc * wc;
        hipLaunchKernelGGL(maxpool_bwd_plain, dim3(stream_grid(total)), dim3(kThreads), 0, (hipStream_t)stream, x, dy, dx, total, h, w, ho, wo);
    }
    return pg::launch_status();
}

PG_EXPORT int pg_l1_pair_blocks(int64_t m) {
    if (m <= 0) return 0;
    const int64_t blocks = (m + (int64_t)kThreads * 16 - 1) / ((int64_t)kThreads * 16);      // >= 4 vectors per lane before a second block pays
    return (int)(blocks > PG_L1_PAIR_MAX_BLOCKS ? PG_L1_PAIR_MAX_BLOCKS : blocks);
}

PG_EXPORT int pg_l1_pair_sum(const float* x, const float* y, float* partials, float* out, int groups, int64_t m, double scale, void* stream) {
    if (!x || !y || !partials || !out || m <= 0 || groups < 1) return PG_ERR_INVALID_ARG;
    if (groups > kMaxGroups) return PG_ERR_UNSUPPORTED;
    if (m > INT64_MAX / 8 / groups) return PG_ERR_TOO_LARGE;
    const int nb = pg_l1_pair_blocks(m);
    if (m % 4 == 0 && pg::aligned16(x) && pg::aligned16(y))
        hipLaunchKernelGGL(l1_pair_partial<4>, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, x, y, partials, groups, m);
    else
        hipLaunchKernelGGL(l1_pair_partial<1>, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, x, y, partials, groups, m);
    const int st = pg::launch_status();
    if (st != PG_OK) return st;
    hipLaunchKernelGGL(l1_pair_final, dim3(groups), dim3(kThreads), 0, (hipStream_t)stream, (const float*)partials, out, nb, scale);
    return pg::launch_status();
}

PG_EXPORT int pg_l1_pair_grad(const float* x, const float* y, const float* s, float* dx, int groups, int64_t m, double denom, void* stream) {
    if (!x || !y || !s || !dx || m <= 0 || groups < 1 || !(denom > 0)) return PG_ERR_INVALID_ARG;
    if (groups > kMaxGroups) return PG_ERR_UNSUPPORTED;
    if (m > INT64_MAX / 8 / groups) return PG_ERR_TOO_LARGE;
    if (m % 4 == 0 && pg::aligned16(x) && pg::aligned16(y) && pg::aligned16(dx))
        hipLaunchKernelGGL(l1_pair_grad<4>, dim3(stream_grid(m / 4)), dim3(kThreads), 0, (hipStream_t)stream, x, y, s, dx, groups, m, (float)denom);
    else
        hipLaunchKernelGGL(l1_pair_grad<1>, dim3(stream_grid(m)), dim3(kThreads), 0, (hipStream_t)stream, x, y, s, dx, groups, m, (float)denom);
    return pg::launch_status();
}
