// The paired reconstruction metrics (torch_utils/ops/image_metrics.py) on gfx950: for a table of uint8 image pairs, sad = sum |a - b|, ssd = sum (a - b)^2
// (exact integers) and the mean SSIM of Wang et al. 2004 (11-tap Gaussian window, sigma 1.5, "valid" positions), in ONE pass over the bytes.
//   tile      one workgroup of 256 lanes = kTile x kTile (32 x 32) SSIM positions of one pair, all channels: the (32 + 10)^2 pixels of both images go
//             into LDS once, as planar bytes (row pitch 44 B, so a lane's 14-byte tap span is four dword reads).  Global reads: dwords where the
//             address allows, single bytes at a row's ragged head and tail and on images whose pixel stride is not `channels`; never a byte
//             outside the window.
//   sums      from the tile in LDS.  A tile owns the pixels under its own 32 x 32 positions; the tiles of the last tile row / column own their
//             10-pixel halo too, so every pixel is counted once.  Per lane <= 24 bytes in 32 bits (24 * 255^2 < 2^21), then 64 bits.
//   SSIM      per channel the five moment maps (a, b, a^2, b^2, ab) are filtered along x from the bytes into LDS (42 x 32 floats each) and along y
//             from there; nothing but the per-tile partials reaches memory.  The moments are taken about an origin per tile, channel and image
//             (an integer level near the tile's mean, `tile_origin`): E[x^2] - mu^2 of a near-flat region then cancels small numbers, not 200^2-sized ones; the means get the
//             origin added back (variances and the covariance do not depend on it).
//   order     no atomics: partials[pair][tile] = {sad, ssd, sum of SSIM (double)}, then one wave per pair adds its tiles in a fixed order.  A
//             pair's bits do not depend on which other pairs share the launch.
#include "pg_common.h"
#include <cmath>
#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                     // SSIM positions per tile and direction
constexpr int kTaps = 11;
constexpr int kHalo = kTaps - 1;
constexpr int kIn = kTile + kHalo;            // 42 pixel rows / columns per tile
constexpr int kPitchW = 11;                   // dwords per planar byte row (44 bytes >= 42, and the last strip's 16-byte read ends at byte 44)
constexpr int kPlaneW = kIn * kPitchW;        // dwords per (image, channel) plane
constexpr int kMaxC = 3;
constexpr int kSlots = (kIn * kMaxC + 3 + 3) / 4;   // dword slots covering one ragged 126-byte row at any misalignment

struct Taps { float w[kTaps]; };
struct Partial { unsigned long long sad, ssd; double ssim; };

__device__ __forceinline__ void put_byte(unsigned char* plane0, int C, int j, int rr, unsigned v) {      // byte j of a tile row -> planar LDS
    const int px = C == 3 ? j / 3 : j;
    const int ch = j - px * C;
    plane0[ch * (kPlaneW * 4) + rr * (kPitchW * 4) + px] = (unsigned char)v;
}

// rows y0 .. y0 + ih - 1, columns x0 .. x0 + iw - 1 of one window -> s_img (planar bytes of this image)
template <int C>
__device__ __forceinline__ void load_tile(const unsigned char* __restrict__ base, int64_t row_stride, int pix_stride, int y0, int x0, int ih, int iw,
                                          unsigned char* s_img) {
    if (pix_stride == C) {                                            // a row's bytes are contiguous
        const int nbytes = iw * C;
        for (int it = threadIdx.x; it < ih * kSlots; it += kThreads) {
            const int rr = it / kSlots, slot = it - rr * kSlots;
            const unsigned char* p = base + (int64_t)(y0 + rr) * row_stride + (int64_t)x0 * C;
            const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
            const int j0 = 4 * slot - mis;                            // the slot's first byte, relative to p; p + j0 is dword-aligned
            if (j0 >= nbytes) continue;
            if (j0 >= 0 && j0 + 4 <= nbytes) {
                const unsigned v = *reinterpret_cast<const unsigned*>(p + j0);
#pragma unroll
                for (int k = 0; k < 4; k++) put_byte(s_img, C, j0 + k, rr, (v >> (8 * k)) & 255u);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int j = j0 + k;
                    if (j >= 0 && j < nbytes) put_byte(s_img, C, j, rr, p[j]);
                }
            }
        }
    } else {
        const int per_row = iw * C;
        for (int it = threadIdx.x; it < ih * per_row; it += kThreads) {
            const int rr = it / per_row, j = it - rr * per_row;
            const int px = C == 3 ? j / 3 : j;
            const int ch = j - px * C;
            put_byte(s_img, C, j, rr, base[(int64_t)(y0 + rr) * row_stride + (int64_t)(x0 + px) * pix_stride + ch]);
        }
    }
}

// the origin the moments of one (tile, channel, image) are taken about: an integer level near the tile's mean -- its four corners and, with their
// weight together, its centre.  Any value gives the same SSIM in exact arithmetic; one near the mean keeps E[x^2] and mu^2 small in float32.
__device__ __forceinline__ float tile_origin(const unsigned char* plane, int ih, int iw) {
    const int pitch = kPitchW * 4;
    const int corners = plane[0] + plane[iw - 1] + plane[(ih - 1) * pitch] + plane[(ih - 1) * pitch + iw - 1];
    return (float)((corners + 4 * plane[(ih / 2) * pitch + iw / 2] + 4) >> 3);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int C>
__device__ __forceinline__ void tile_body(const pg_metric_pair& job, int tile, int tiles_x, Partial* out, const Taps& taps, unsigned* s_px, float* s_h,
                                          Partial* s_red) {
    const int t = threadIdx.x;
    const int oh_all = job.h - kHalo, ow_all = job.w - kHalo;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * kTile, x0 = tx * kTile;
    const int oh = min(kTile, oh_all - y0), ow = min(kTile, ow_all - x0);          // this tile's SSIM positions
    const int ih = oh + kHalo, iw = ow + kHalo;                                    // ... and the pixels under them
    const bool last_y = y0 + oh == oh_all, last_x = x0 + ow == ow_all;

    for (int i = t; i < 2 * kMaxC * kPlaneW; i += kThreads) s_px[i] = 0u;          // (the bytes beyond iw / ih are read, never used)
    __syncthreads();
    unsigned char* s_a = reinterpret_cast<unsigned char*>(s_px);
    unsigned char* s_b = reinterpret_cast<unsigned char*>(s_px + kMaxC * kPlaneW);
    load_tile<C>(job.a, job.a_row_stride, job.a_pix_stride, y0, x0, ih, iw, s_a);
    load_tile<C>(job.b, job.b_row_stride, job.b_pix_stride, y0, x0, ih, iw, s_b);
    __syncthreads();

    // ---- integer sums over the pixels this tile owns
    unsigned sad = 0u, ssd = 0u;
    for (int it = t; it < C * ih * kPitchW; it += kThreads) {
        const int ch = it / (ih * kPitchW), rem = it - ch * (ih * kPitchW);
        const int rr = rem / kPitchW, d = rem - rr * kPitchW;
        if (rr >= kTile && !last_y) continue;
        const unsigned va = s_px[ch * kPlaneW + rr * kPitchW + d], vb = s_px[(kMaxC + ch) * kPlaneW + rr * kPitchW + d];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = 4 * d + k;
            if (col < iw && (col < kTile || last_x)) {
                const int df = (int)((va >> (8 * k)) & 255u) - (int)((vb >> (8 * k)) & 255u);
                sad += (unsigned)(df < 0 ? -df : df);
                ssd += (unsigned)(df * df);
            }
        }
    }

    // ---- SSIM, channel by channel
    float ssim_acc = 0.f;
    const float C1 = 6.5025f, C2 = 58.5225f;
    for (int ch = 0; ch < C; ch++) {
        const unsigned* pa = s_px + ch * kPlaneW;
        const unsigned* pb = s_px + (kMaxC + ch) * kPlaneW;
        const float oa = tile_origin(s_a + ch * (kPlaneW * 4), ih, iw), ob = tile_origin(s_b + ch * (kPlaneW * 4), ih, iw);
        // along x: item = (row, strip of 4 positions); 14 bytes of each image -> 4 values of each of the 5 maps
        for (int it = t; it < ih * (kTile / 4); it += kThreads) {
            const int rr = it >> 3, s = it & 7;
            float a[16], b[16];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned va = pa[rr * kPitchW + s + q], vb = pb[rr * kPitchW + s + q];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    a[4 * q + k] = (float)((va >> (8 * k)) & 255u) - oa;
                    b[4 * q + k] = (float)((vb >> (8 * k)) & 255u) - ob;
                }
            }
            float m[5][4];
#pragma unroll
            for (int o = 0; o < 4; o++)
#pragma unroll
                for (int q = 0; q < 5; q++) m[q][o] = 0.f;
#pragma unroll
            for (int i = 0; i < kTaps + 3; i++) {
                const float v0 = a[i], v1 = b[i], v2 = a[i] * a[i], v3 = b[i] * b[i], v4 = a[i] * b[i];
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int k = i - o;
                    if (k >= 0 && k < kTaps) {
                        m[0][o] += taps.w[k] * v0;
                        m[1][o] += taps.w[k] * v1;
                        m[2][o] += taps.w[k] * v2;
                        m[3][o] += taps.w[k] * v3;
                        m[4][o] += taps.w[k] * v4;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 5; q++) {
                float4 v = {m[q][0], m[q][1], m[q][2], m[q][3]};
                *reinterpret_cast<float4*>(s_h + (q * kIn + rr) * kTile + 4 * s) = v;
            }
        }
        __syncthreads();
        // along y: lane = (column, 4 consecutive rows)
        {
            const int col = t & 31, r0 = (t >> 5) * 4;
            float m[5][4];
#pragma unroll
            for (int o = 0; o < 4; o++)
#pragma unroll
                for (int q = 0; q < 5; q++) m[q][o] = 0.f;
            if (r0 < oh && col < ow) {
#pragma unroll
                for (int i = 0; i < kTaps + 3; i++) {
                    if (r0 + i < ih) {
                        float v[5];
#pragma unroll
                        for (int q = 0; q < 5; q++) v[q] = s_h[(q * kIn + r0 + i) * kTile + col];
#pragma unroll
                        for (int o = 0; o < 4; o++) {
                            const int k = i - o;
                            if (k >= 0 && k < kTaps) {
#pragma unroll
                                for (int q = 0; q < 5; q++) m[q][o] += taps.w[k] * v[q];
                            }
                        }
                    }
                }
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    if (r0 + o < oh) {
#pragma clang fp contract(off)                                        // identical images give exactly 1 at every position
                        const float ea = m[0][o], eb = m[1][o];
                        const float mua = ea + oa, mub = eb + ob;
                        const float va = m[2][o] - ea * ea, vb = m[3][o] - eb * eb, cab = m[4][o] - ea * eb;
                        const float num = (2.f * mua * mub + C1) * (2.f * cab + C2);
                        const float den = (mua * mua + mub * mub + C1) * (va + vb + C2);
                        ssim_acc += num / den;
                    }
                }
            }
        }
        __syncthreads();                                              // s_h is rewritten by the next channel
    }

    // ---- block sums in a fixed order: wave butterfly, then the four waves in order
    const unsigned long long w_sad = wave_sum<unsigned long long>(sad), w_ssd = wave_sum<unsigned long long>(ssd);
    const double w_ssim = wave_sum<double>((double)ssim_acc);
    if ((t & 63) == 0) {
        s_red[t >> 6].sad = w_sad;
        s_red[t >> 6].ssd = w_ssd;
        s_red[t >> 6].ssim = w_ssim;
    }
    __syncthreads();
    if (t == 0) {
        Partial p;
        p.sad = (s_red[0].sad + s_red[1].sad) + (s_red[2].sad + s_red[3].sad);
        p.ssd = (s_red[0].ssd + s_red[1].ssd) + (s_red[2].ssd + s_red[3].ssd);
        p.ssim = (s_red[0].ssim + s_red[1].ssim) + (s_red[2].ssim + s_red[3].ssim);
        *out = p;
    }
}

// grid (tiles_max, npairs): block (x, y) = tile x of pair y; pairs with fewer tiles leave their spare blocks idle
__global__ __launch_bounds__(kThreads) void pair_metrics_tiles(const pg_metric_pair* __restrict__ jobs, Partial* __restrict__ partials, int tiles_max, Taps taps) {
    __shared__ unsigned s_px[2 * kMaxC * kPlaneW];
    __shared__ __attribute__((aligned(16))) float s_h[5 * kIn * kTile];
    __shared__ Partial s_red[kThreads / 64];
    const pg_metric_pair job = jobs[blockIdx.y];
    if (job.h <= kHalo || job.w <= kHalo) return;                     // (refused on the host; a table that differs from the host's copy launches nothing wild)
    const int tiles_x = (job.w - kHalo + kTile - 1) / kTile, tiles_y = (job.h - kHalo + kTile - 1) / kTile;
    const int tile = blockIdx.x;
    if (tile >= tiles_x * tiles_y) return;                            // uniform over the block: no lane reaches a barrier
    Partial* out = partials + (int64_t)blockIdx.y * tiles_max + tile;
    if (job.channels == 3)
        tile_body<3>(job, tile, tiles_x, out, taps, s_px, s_h, s_red);
    else
        tile_body<1>(job, tile, tiles_x, out, taps, s_px, s_h, s_red);
}

// one wave per pair: its tiles' partials in a fixed order
__global__ __launch_bounds__(64) void pair_metrics_finish(const pg_metric_pair* __restrict__ jobs, const Partial* __restrict__ partials, int tiles_max,
                                                          long long* __restrict__ sad, long long* __restrict__ ssd, float* __restrict__ ssim) {
    const pg_metric_pair job = jobs[blockIdx.x];
    const int oh = job.h - kHalo, ow = job.w - kHalo;
    int n = oh > 0 && ow > 0 ? ((ow + kTile - 1) / kTile) * ((oh + kTile - 1) / kTile) : 0;
    n = n < tiles_max ? n : tiles_max;
    const Partial* p = partials + (int64_t)blockIdx.x * tiles_max;
    unsigned long long a = 0ull, b = 0ull;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) {
        a += p[i].sad;
        b += p[i].ssd;
        s += p[i].ssim;
    }
    a = wave_sum<unsigned long long>(a);
    b = wave_sum<unsigned long long>(b);
    s = wave_sum<double>(s);
    if (threadIdx.x == 0) {
        sad[blockIdx.x] = (long long)a;
        ssd[blockIdx.x] = (long long)b;
        ssim[blockIdx.x] = n > 0 ? (float)(s / ((double)oh * (double)ow * (double)job.channels)) : 0.f;
    }
}

// argument checks of a host table; tiles_max = the largest tile count of a pair
int check_table(const pg_metric_pair* jobs, int npairs, int* tiles_max) {
    if (!jobs || npairs <= 0) return PG_ERR_INVALID_ARG;
    if (npairs > PG_METRIC_MAX_PAIRS) return PG_ERR_TOO_LARGE;
    int tm = 0;
    for (int j = 0; j < npairs; j++) {
        const pg_metric_pair& q = jobs[j];
        if (!q.a || !q.b || q.h <= kHalo || q.w <= kHalo || (q.channels != 1 && q.channels != 3)) return PG_ERR_INVALID_ARG;
        if (q.a_pix_stride < q.channels || q.b_pix_stride < q.channels || q.a_row_stride < 1 || q.b_row_stride < 1) return PG_ERR_INVALID_ARG;
        if ((int64_t)q.h * q.w * q.channels > INT32_MAX) return PG_ERR_TOO_LARGE;
        if (q.a_row_stride > INT64_MAX / q.h || q.b_row_stride > INT64_MAX / q.h) return PG_ERR_TOO_LARGE;
        const int64_t tiles = (int64_t)((q.w - kHalo + kTile - 1) / kTile) * ((q.h - kHalo + kTile - 1) / kTile);
        if (tiles > INT32_MAX) return PG_ERR_TOO_LARGE;
        if (tiles > tm) tm = (int)tiles;
    }
    *tiles_max = tm;
    return PG_OK;
}

Taps gaussian_taps() {
    double g[kTaps], sum = 0.0;
    for (int k = 0; k < kTaps; k++) {
        const double d = k - kTaps / 2;
        g[k] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    Taps t;
    for (int k = 0; k < kTaps; k++) t.w[k] = (float)(g[k] / sum);
    return t;
}

}  // namespace

PG_EXPORT int pg_image_metrics_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int64_t pg_image_pair_metrics_workspace(const pg_metric_pair* jobs_host, int npairs) {
    int tiles_max = 0;
    const int st = check_table(jobs_host, npairs, &tiles_max);
    if (st != PG_OK) return st;
    return (int64_t)npairs * tiles_max * (int64_t)sizeof(Partial);
}

PG_EXPORT int pg_image_pair_metrics_u8(const pg_metric_pair* jobs_host, const pg_metric_pair* jobs_device, int npairs, void* workspace, int64_t* sad,
                                       int64_t* ssd, float* ssim, void* stream) {
    int tiles_max = 0;
    const int st = check_table(jobs_host, npairs, &tiles_max);
    if (st != PG_OK) return st;
    if (!jobs_device || !workspace || !sad || !ssd || !ssim) return PG_ERR_INVALID_ARG;
    static const Taps taps = gaussian_taps();
    hipLaunchKernelGGL(pair_metrics_tiles, dim3((unsigned)tiles_max, (unsigned)npairs), dim3(kThreads), 0, (hipStream_t)stream, jobs_device,
                       (Partial*)workspace, tiles_max, taps);
    const int ls = pg::launch_status();
    if (ls != PG_OK) return ls;
    hipLaunchKernelGGL(pair_metrics_finish, dim3((unsigned)npairs), dim3(64), 0, (hipStream_t)stream, jobs_device, (const Partial*)workspace, tiles_max,
                       (long long*)sad, (long long*)ssd, ssim);
    return pg::launch_status();
}
