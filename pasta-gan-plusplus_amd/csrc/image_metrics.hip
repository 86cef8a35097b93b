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
// The tile loader, the origin and the filter live in image_metrics_tile.h, shared with region_metrics.hip (the same pass per label region).
#include "image_metrics_tile.h"

namespace {

using namespace pgm;

struct Partial { unsigned long long sad, ssd; double ssim; };

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

    // ---- SSIM, channel by channel (image_metrics_tile.h)
    float ssim_acc = 0.f;
    for (int ch = 0; ch < C; ch++) {
        const float oa = tile_origin(s_a + ch * (kPlaneW * 4), ih, iw), ob = tile_origin(s_b + ch * (kPlaneW * 4), ih, iw);
        ssim_channel(s_px + ch * kPlaneW, s_px + (kMaxC + ch) * kPlaneW, oa, ob, ih, oh, ow, taps, s_h, [&](int, int, float v) { ssim_acc += v; });
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
