// Patch-routing warps of the data loader on gfx950: OpenCV's warpPerspective (8-bit, INTER_LINEAR,
// BORDER_CONSTANT 0) restated bit for bit, batched over jobs, plus the erode-and-paste step of the de-normalisation.
// What it replaces: cv2.warpPerspective / cv2.erode calls of training/dataset.py:2555-2700 (44 warps per sample, single-threaded on
// the DataLoader's main thread in the reference).  Integer/byte work: one thread per destination pixel, coordinates in fp64
// with the evaluation order of OpenCV's WarpPerspectiveInvoker (imgwarp.cpp) -- no fused multiply-adds, round half to even --
// weights 15-bit integers; HBM/L2-bound gather (each destination pixel reads a 2x2 source patch).
#include "pg_common.h"
#include <cstdint>

namespace {

using namespace pg;

constexpr int kInterBits = 5, kTab = 1 << kInterBits;

// Where a destination pixel reads its source: integer tap position (saturated to short, as OpenCV's map) and the four 15-bit bilinear weights.
struct WarpTap {
    int sx, sy, w00, w01, w10, w11;
};

// OpenCV's coordinate evaluation for destination pixel (x, y): block origin term + offset term in fp64, every product and sum rounded on its own (no fused
// multiply-add), round half to even, 5 fractional bits.  Shared by every kernel that warps, so that they all read the same taps.
__device__ __forceinline__ WarpTap warp_tap(const double* __restrict__ m, int x, int y, int block_w) {
    const int xb = (x / block_w) * block_w, x1 = x - xb;                 // OpenCV walks blocks: origin term + offset term
    const double X0 = __dadd_rn(__dadd_rn(__dmul_rn(m[0], (double)xb), __dmul_rn(m[1], (double)y)), m[2]);
    const double Y0 = __dadd_rn(__dadd_rn(__dmul_rn(m[3], (double)xb), __dmul_rn(m[4], (double)y)), m[5]);
    const double W0 = __dadd_rn(__dadd_rn(__dmul_rn(m[6], (double)xb), __dmul_rn(m[7], (double)y)), m[8]);
    double W = __dadd_rn(W0, __dmul_rn(m[6], (double)x1));
    W = W != 0.0 ? __ddiv_rn((double)kTab, W) : 0.0;
    double fX = __dmul_rn(__dadd_rn(X0, __dmul_rn(m[0], (double)x1)), W);
    double fY = __dmul_rn(__dadd_rn(Y0, __dmul_rn(m[3], (double)x1)), W);
    fX = fmax(-2147483648.0, fmin(2147483647.0, fX));
    fY = fmax(-2147483648.0, fmin(2147483647.0, fY));
    const int X = (int)rint(fX), Y = (int)rint(fY);                      // cvRound: round half to even
    WarpTap t;
    t.sx = X >> kInterBits;
    t.sy = Y >> kInterBits;
    t.sx = t.sx < -32768 ? -32768 : (t.sx > 32767 ? 32767 : t.sx);       // saturate_cast<short>
    t.sy = t.sy < -32768 ? -32768 : (t.sy > 32767 ? 32767 : t.sy);
    const int fx = X & (kTab - 1), fy = Y & (kTab - 1);
    t.w00 = (32 - fx) * (32 - fy) * 32, t.w01 = fx * (32 - fy) * 32, t.w10 = (32 - fx) * fy * 32, t.w11 = fx * fy * 32;
    if ((fx | fy) == 0) { t.w00 = 32767; t.w11 = 1; }                    // initInterTab2D: 1.0 saturates, the correction lands on the last tap
    return t;
}

// Channels c0 .. c0 + NC - 1 (NC <= 0: `nc` channels, run-time) of the bilinear sample at `t` from an src_h x src_w x C image; taps outside read 0.
template <int NC>
__device__ __forceinline__ void warp_sample(const uint8_t* __restrict__ s, int src_h, int src_w, int C, const WarpTap& t, int c0, int nc, uint8_t* __restrict__ d) {
    const bool y0 = t.sy >= 0 && t.sy < src_h, y1 = t.sy + 1 >= 0 && t.sy + 1 < src_h;
    const bool x0 = t.sx >= 0 && t.sx < src_w, x1ok = t.sx + 1 >= 0 && t.sx + 1 < src_w;
    const int n = NC > 0 ? NC : nc;
#pragma unroll
    for (int c = c0; c < c0 + n; c++) {
        const int p00 = (y0 && x0) ? s[((int64_t)t.sy * src_w + t.sx) * C + c] : 0;
        const int p01 = (y0 && x1ok) ? s[((int64_t)t.sy * src_w + t.sx + 1) * C + c] : 0;
        const int p10 = (y1 && x0) ? s[((int64_t)(t.sy + 1) * src_w + t.sx) * C + c] : 0;
        const int p11 = (y1 && x1ok) ? s[((int64_t)(t.sy + 1) * src_w + t.sx + 1) * C + c] : 0;
        const int v = (p00 * t.w00 + p01 * t.w01 + p10 * t.w10 + p11 * t.w11 + (1 << 14)) >> 15;
        d[c - c0] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

__global__ __launch_bounds__(256) void warp_perspective_u8_kernel(const pg_warp_job* __restrict__ jobs) {
    const pg_warp_job jb = jobs[blockIdx.y];
    const int npix = jb.dst_h * jb.dst_w;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        const int y = i / jb.dst_w, x = i - y * jb.dst_w;
        const WarpTap t = warp_tap(jb.minv, x, y, jb.block_w);
        warp_sample<0>(jb.src, jb.src_h, jb.src_w, jb.channels, t, 0, jb.channels, jb.dst + (int64_t)i * jb.channels);
    }
}

// The erode of the paste step: cv2.erode(mask, ones(k, k)) with OpenCV's default anchor (k/2, k/2), pixels outside the image ignored
// -> "== 255" iff every in-range tap of the window [y - k/2, y - k/2 + k) x [x - k/2, x - k/2 + k) is 255.  K > 0 fixes the window at compile
// time (8: the upper mode's, dataset.py:2589; 5: the lower and full modes', :1827 / :3345); K = 0 reads it from `k` (1..16).
template <int K>
__device__ __forceinline__ bool eroded_white(const uint8_t* __restrict__ mask, int y, int x, int h, int w, int mc, int k) {
    const int ks = K > 0 ? K : k, a = ks / 2;
    for (int ky = 0; ky < ks; ky++) {
        const int yy = y + ky - a;
        if (yy < 0 || yy >= h) continue;
        for (int kx = 0; kx < ks; kx++) {
            const int xx = x + kx - a;
            if (xx < 0 || xx >= w) continue;
            if (mask[((int64_t)yy * w + xx) * mc] != 255) return false;
        }
    }
    return true;
}

// canvas[p] = (erode_kxk(mask channel 0)[p] == 255) ? patch[p] : canvas[p]      (dataset.py:2624-2630)
template <int K>
__global__ __launch_bounds__(256) void patch_compose_u8_kernel(const uint8_t* __restrict__ patch, const uint8_t* __restrict__ mask, uint8_t* __restrict__ canvas,
                                                               uint8_t* __restrict__ canvas2, int h, int w, int mc, int k) {
    const int npix = h * w;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        const int y = i / w, x = i - y * w;
        if (eroded_white<K>(mask, y, x, h, w, mc, k)) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const uint8_t v = patch[(int64_t)i * 3 + c];
                canvas[(int64_t)i * 3 + c] = v;
                if (canvas2) canvas2[(int64_t)i * 3 + c] = v;
            }
        }
    }
}

// The whole paste sequence of one canvas in one pass (round 6): the reference pastes its parts one after the other, later parts overwriting earlier ones
// (dataset.py:2620-2633), i.e. a pixel ends up with the patch of the LAST part whose eroded mask is set there, or 0.  One job = one canvas (+ the copy that
// skips the sleeve parts); one thread = one pixel, walking the job's parts in order.  Every canvas pixel is written: the canvases need no zero fill.
template <int K>
__global__ __launch_bounds__(256) void patch_compose_ordered_u8_kernel(const pg_compose_job* __restrict__ jobs, int h, int w, int mc, int k) {
    const pg_compose_job* jb = jobs + blockIdx.y;
    const int npix = h * w, nparts = jb->nparts;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        const int y = i / w, x = i - y * w;
        int last = -1, last2 = -1;
        for (int p = 0; p < nparts; p++) {
            const uint8_t* mask = jb->mask[p];
            // (the window's own pixel first: most pixels lie outside a part; it is always in the window, since 0 <= k/2 < k)
            if (mask[(int64_t)i * mc] == 255 && eroded_white<K>(mask, y, x, h, w, mc, k)) {
                last = p;
                if (jb->to_canvas2[p]) last2 = p;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            jb->canvas[(int64_t)i * 3 + c] = last >= 0 ? jb->patch[last][(int64_t)i * 3 + c] : (uint8_t)0;
            if (jb->canvas2) jb->canvas2[(int64_t)i * 3 + c] = last2 >= 0 ? jb->patch[last2][(int64_t)i * 3 + c] : (uint8_t)0;
        }
    }
}

// Fused de-normalisation (the snapshot grid, training/snapshot_grid.py): patches -> canvas without the warped intermediates.  What the three launches
// above leave -- pg_warp_perspective_u8 of every patch and mask to H x W, then patch_compose_ordered_u8_kernel -- byte for byte: the same `warp_tap`, the
// same erode rule.  One workgroup = one kDT x kDT canvas tile of one job.  Per part, in paste order: channel 0 of the warped mask is evaluated over the tile
// plus the erode halo into LDS (once per halo pixel, instead of k * k global reads per pixel), pixels outside the canvas as 255 (= ignored); each lane erodes
// its kDT * kDT / 256 pixels from LDS and remembers the last part whose eroded mask is set.  The three patch channels are warped for that part only.
// LDS: (kDT + 15)^2 = 2209 bytes at most -- no occupancy limit; the tile is 32 so that the halo work stays below half of the tile's own (39^2 / 32^2 = 1.49
// evaluations per pixel at k = 8, against 2.07 for a 16-tile) while a 512 x 512 canvas still gives 256 workgroups per job.
constexpr int kDT = 32, kDHaloMax = kDT + 15;

template <int K>
__global__ __launch_bounds__(256) void patch_denorm_u8_kernel(const pg_denorm_job* __restrict__ jobs, int H, int W, int ph, int pw, int mc, int block_w, int tiles_x) {
    __shared__ uint8_t s_mask[kDHaloMax * kDHaloMax];
    const pg_denorm_job* jb = jobs + blockIdx.y;
    constexpr int ks = K, a = ks / 2, hs = kDT + ks - 1;                  // halo side
    const int ty0 = ((int)blockIdx.x / tiles_x) * kDT, tx0 = ((int)blockIdx.x % tiles_x) * kDT;
    const int lx = threadIdx.x % kDT, ly0 = threadIdx.x / kDT;            // this lane's pixels: (ly0 + 8 j, lx), j = 0..3
    const int nparts = jb->nparts;
    int last[kDT * kDT / 256];
#pragma unroll
    for (int j = 0; j < kDT * kDT / 256; j++) last[j] = -1;
    for (int p = 0; p < nparts; p++) {
        const uint8_t* mask = jb->mask[p];
        const double* m = jb->minv[p];
        int any = 0;
        for (int i = threadIdx.x; i < hs * hs; i += 256) {
            const int hy = i / hs, hx = i - hy * hs;
            const int y = ty0 - a + hy, x = tx0 - a + hx;
            uint8_t v = 255;                                              // outside the canvas: the erode ignores the tap
            if (y >= 0 && y < H && x >= 0 && x < W) {
                warp_sample<1>(mask, ph, pw, mc, warp_tap(m, x, y, block_w), 0, 1, &v);
                any |= v == 255;
            }
            s_mask[i] = v;
        }
        if (__syncthreads_or(any)) {                                      // (most tiles lie outside most parts)
#pragma unroll
            for (int j = 0; j < kDT * kDT / 256; j++) {
                const int ly = ly0 + 8 * j;
                if (s_mask[(ly + a) * hs + lx + a] != 255) continue;      // the window's own pixel first
                int dark = 0;                                             // (branch-free: the window is K * K LDS bytes)
#pragma unroll
                for (int ky = 0; ky < ks; ky++) {
                    const uint8_t* row = s_mask + (ly + ky) * hs + lx;
#pragma unroll
                    for (int kx = 0; kx < ks; kx++) dark |= row[kx] != 255;
                }
                if (!dark) last[j] = p;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < kDT * kDT / 256; j++) {
        const int y = ty0 + ly0 + 8 * j, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        uint8_t v[3] = {0, 0, 0};
        if (last[j] >= 0) warp_sample<3>(jb->patch[last[j]], ph, pw, 3, warp_tap(jb->minv[last[j]], x, y, block_w), 0, 3, v);
        uint8_t* d = jb->canvas + ((int64_t)y * W + x) * 3;
        d[0] = v[0], d[1] = v[1], d[2] = v[2];
    }
}

}  // namespace

PG_EXPORT int pg_patch_routing_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_patch_compose_ordered_u8_k(const pg_compose_job* jobs_device, int njobs, int h, int w, int mask_channels, int ksize, void* stream) {
    if (!jobs_device || njobs <= 0 || h <= 0 || w <= 0 || mask_channels <= 0) return PG_ERR_INVALID_ARG;
    if (ksize < 1 || ksize > 16) return PG_ERR_INVALID_ARG;
    if ((int64_t)h * w > 0x3fffffffLL) return PG_ERR_TOO_LARGE;
    if (njobs > 65535) return PG_ERR_TOO_LARGE;
    int bx = (h * w + 255) / 256;
    if (bx > 1024) bx = 1024;
    const dim3 grid((unsigned)bx, (unsigned)njobs);
    const hipStream_t st = (hipStream_t)stream;
    if (ksize == 8)
        hipLaunchKernelGGL(patch_compose_ordered_u8_kernel<8>, grid, dim3(256), 0, st, jobs_device, h, w, mask_channels, 8);
    else if (ksize == 5)
        hipLaunchKernelGGL(patch_compose_ordered_u8_kernel<5>, grid, dim3(256), 0, st, jobs_device, h, w, mask_channels, 5);
    else
        hipLaunchKernelGGL(patch_compose_ordered_u8_kernel<0>, grid, dim3(256), 0, st, jobs_device, h, w, mask_channels, ksize);
    return pg::launch_status();
}

PG_EXPORT int pg_patch_denorm_u8(const pg_denorm_job* jobs_device, int njobs, int H, int W, int ph, int pw, int mask_channels, int ksize, int block_w,
                                 void* stream) {
    if (!jobs_device || njobs <= 0 || H <= 0 || W <= 0 || ph <= 0 || pw <= 0 || mask_channels <= 0 || block_w <= 0) return PG_ERR_INVALID_ARG;
    if (ksize < 1 || ksize > 16) return PG_ERR_INVALID_ARG;
    if ((int64_t)H * W > 0x3fffffffLL || (int64_t)ph * pw > 0x3fffffffLL) return PG_ERR_TOO_LARGE;
    if (njobs > 65535) return PG_ERR_TOO_LARGE;
    const int tiles_x = (W + kDT - 1) / kDT, tiles_y = (H + kDT - 1) / kDT;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)njobs);
    const hipStream_t st = (hipStream_t)stream;
    // every window size is a compile-time instantiation: the erode loops over LDS unroll, and there is one code path to trust
#define PG_DENORM_CASE(KS) \
    case KS: hipLaunchKernelGGL(patch_denorm_u8_kernel<KS>, grid, dim3(256), 0, st, jobs_device, H, W, ph, pw, mask_channels, block_w, tiles_x); break;
    switch (ksize) {
        PG_DENORM_CASE(1) PG_DENORM_CASE(2) PG_DENORM_CASE(3) PG_DENORM_CASE(4) PG_DENORM_CASE(5) PG_DENORM_CASE(6) PG_DENORM_CASE(7) PG_DENORM_CASE(8)
        PG_DENORM_CASE(9) PG_DENORM_CASE(10) PG_DENORM_CASE(11) PG_DENORM_CASE(12) PG_DENORM_CASE(13) PG_DENORM_CASE(14) PG_DENORM_CASE(15) PG_DENORM_CASE(16)
    }
#undef PG_DENORM_CASE
    return pg::launch_status();
}

PG_EXPORT int pg_patch_compose_ordered_u8(const pg_compose_job* jobs_device, int njobs, int h, int w, int mask_channels, void* stream) {
    return pg_patch_compose_ordered_u8_k(jobs_device, njobs, h, w, mask_channels, 8, stream);
}

PG_EXPORT int pg_warp_perspective_u8(const pg_warp_job* jobs_device, int njobs, int max_dst_pixels, void* stream) {
    if (!jobs_device || njobs <= 0 || max_dst_pixels <= 0) return PG_ERR_INVALID_ARG;
    if (njobs > 65535) return PG_ERR_TOO_LARGE;
    int bx = (max_dst_pixels + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(warp_perspective_u8_kernel, dim3((unsigned)bx, (unsigned)njobs), dim3(256), 0, (hipStream_t)stream, jobs_device);
    return pg::launch_status();
}

PG_EXPORT int pg_patch_compose_u8_k(const uint8_t* patch, const uint8_t* mask, uint8_t* canvas, uint8_t* canvas2, int h, int w, int mask_channels, int ksize,
                                    void* stream) {
    if (!patch || !mask || !canvas || h <= 0 || w <= 0 || mask_channels <= 0) return PG_ERR_INVALID_ARG;
    if (ksize < 1 || ksize > 16) return PG_ERR_INVALID_ARG;
    if ((int64_t)h * w > 0x3fffffffLL) return PG_ERR_TOO_LARGE;
    int bx = (h * w + 255) / 256;
    if (bx > pg::max_stream_blocks()) bx = pg::max_stream_blocks();
    const hipStream_t st = (hipStream_t)stream;
    if (ksize == 8)
        hipLaunchKernelGGL(patch_compose_u8_kernel<8>, dim3((unsigned)bx), dim3(256), 0, st, patch, mask, canvas, canvas2, h, w, mask_channels, 8);
    else if (ksize == 5)
        hipLaunchKernelGGL(patch_compose_u8_kernel<5>, dim3((unsigned)bx), dim3(256), 0, st, patch, mask, canvas, canvas2, h, w, mask_channels, 5);
    else
        hipLaunchKernelGGL(patch_compose_u8_kernel<0>, dim3((unsigned)bx), dim3(256), 0, st, patch, mask, canvas, canvas2, h, w, mask_channels, ksize);
    return pg::launch_status();
}

PG_EXPORT int pg_patch_compose_u8(const uint8_t* patch, const uint8_t* mask, uint8_t* canvas, uint8_t* canvas2, int h, int w, int mask_channels, void* stream) {
    return pg_patch_compose_u8_k(patch, mask, canvas, canvas2, h, w, mask_channels, 8, stream);
}
