// The reconstruction metrics per label region, and the confusion count of two label maps (torch_utils/ops/region_metrics.py), on gfx950.
//
// pg_region_pair_metrics_u8: image_metrics.hip's pass (image_metrics_tile.h: the same tiles, loader, per-tile origins and filter) with a third window,
// the labels, beside the two images.
//   labels    the (32 + 10)^2 label bytes of a tile go into LDS through the same loader (one "channel"), and are replaced in place by the pixel's
//             membership byte: bit r = the label is in region r (a label >= 32 is in none).  Everything below reads that byte.
//   sums      per region n, sad, ssd over the pixels the tile owns (its own 32 x 32, plus the 10-pixel halo on the last tile row / column: every
//             pixel once).  A tile holds <= 42^2 pixels, so each of its sums fits 32 bits (42^2 * 3 * 255^2 < 2^29); 64 bits from the finish on.
//   SSIM      ssim_channel hands every position's value to a sink that adds it to the accumulators of the regions holding the position's centre
//             pixel (row + 5, col + 5 of the tile, always inside it); `positions` counts those centres once, not per channel.
//   order     no atomics: partials[pair][tile][region], then one wave per (pair, region) adds the tiles in a fixed order.  A lane adds its
//             positions in the order image_metrics.hip does, so a region holding every label reproduces that kernel's sum.
//
// pg_label_confusion_u8: one launch; a workgroup counts its pixels into an LDS table of classes^2 bins (a lane walks 8 consecutive pixels and sends
// one LDS atomic per run of equal bins: parsing maps are mostly runs), then adds its non-zero bins to the output with 64-bit integer atomics
// (exact, hence independent of their order).
#include "image_metrics_tile.h"

namespace {

using namespace pgm;

constexpr int kMaxR = PG_REGION_MAX;
constexpr int kRun = 8;                       // consecutive pixels per lane and step of the confusion count
constexpr int kConfBlocksMax = 256;

struct Regions { unsigned set[kMaxR]; int n; };
struct RPartial { unsigned n, positions, sad, ssd; double ssim; };
struct Luts { unsigned w[128]; };             // pred_lut[256], then target_lut[256]

template <int C>
__device__ __forceinline__ void tile_body(const pg_region_pair& job, int tile, int tiles_x, RPartial* out, const Taps& taps, const Regions& regions,
                                          unsigned* s_px, unsigned* s_lab, float* s_h, RPartial* s_red) {
    const int t = threadIdx.x;
    const int R = regions.n;
    const int oh_all = job.h - kHalo, ow_all = job.w - kHalo;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * kTile, x0 = tx * kTile;
    const int oh = min(kTile, oh_all - y0), ow = min(kTile, ow_all - x0);          // this tile's SSIM positions
    const int ih = oh + kHalo, iw = ow + kHalo;                                    // ... and the pixels under them
    const bool last_y = y0 + oh == oh_all, last_x = x0 + ow == ow_all;

    for (int i = t; i < 2 * kMaxC * kPlaneW; i += kThreads) s_px[i] = 0u;          // (the bytes beyond iw / ih are read, never used)
    for (int i = t; i < kPlaneW; i += kThreads) s_lab[i] = 0u;
    __syncthreads();
    unsigned char* s_a = reinterpret_cast<unsigned char*>(s_px);
    unsigned char* s_b = reinterpret_cast<unsigned char*>(s_px + kMaxC * kPlaneW);
    unsigned char* s_m = reinterpret_cast<unsigned char*>(s_lab);
    load_tile<C>(job.a, job.a_row_stride, job.a_pix_stride, y0, x0, ih, iw, s_a);
    load_tile<C>(job.b, job.b_row_stride, job.b_pix_stride, y0, x0, ih, iw, s_b);
    load_tile<1>(job.labels, job.l_row_stride, job.l_pix_stride, y0, x0, ih, iw, s_m);
    __syncthreads();
    for (int i = t; i < kPlaneW; i += kThreads) {                                  // label -> membership byte
        const unsigned v = s_lab[i];
        unsigned o = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned lab = (v >> (8 * k)) & 255u;
            unsigned m = 0u;
#pragma unroll
            for (int r = 0; r < kMaxR; r++) m |= ((regions.set[r] >> (lab & 31u)) & 1u) << r;
            o |= (lab < 32u ? m : 0u) << (8 * k);
        }
        s_lab[i] = o;
    }
    __syncthreads();

    unsigned cn[kMaxR], cpos[kMaxR], csad[kMaxR], cssd[kMaxR];
    float cssim[kMaxR];
#pragma unroll
    for (int r = 0; r < kMaxR; r++) cn[r] = cpos[r] = csad[r] = cssd[r] = 0u, cssim[r] = 0.f;

    // ---- integer sums over the pixels this tile owns
    for (int it = t; it < C * ih * kPitchW; it += kThreads) {
        const int ch = it / (ih * kPitchW), rem = it - ch * (ih * kPitchW);
        const int rr = rem / kPitchW, d = rem - rr * kPitchW;
        if (rr >= kTile && !last_y) continue;
        const unsigned va = s_px[ch * kPlaneW + rr * kPitchW + d], vb = s_px[(kMaxC + ch) * kPlaneW + rr * kPitchW + d];
        const unsigned vm = s_lab[rr * kPitchW + d];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = 4 * d + k;
            if (col < iw && (col < kTile || last_x)) {
                const int df = (int)((va >> (8 * k)) & 255u) - (int)((vb >> (8 * k)) & 255u);
                const unsigned ad = (unsigned)(df < 0 ? -df : df), sq = (unsigned)(df * df);
                const unsigned m = (vm >> (8 * k)) & 255u;
#pragma unroll
                for (int r = 0; r < kMaxR; r++) {
                    if (r < R) {
                        const bool in = (m >> r) & 1u;
                        cn[r] += in && ch == 0 ? 1u : 0u;
                        csad[r] += in ? ad : 0u;
                        cssd[r] += in ? sq : 0u;
                    }
                }
            }
        }
    }

    // ---- SSIM, channel by channel (image_metrics_tile.h): a position belongs to the regions of its centre pixel
    for (int ch = 0; ch < C; ch++) {
        const float oa = tile_origin(s_a + ch * (kPlaneW * 4), ih, iw), ob = tile_origin(s_b + ch * (kPlaneW * 4), ih, iw);
        ssim_channel(s_px + ch * kPlaneW, s_px + (kMaxC + ch) * kPlaneW, oa, ob, ih, oh, ow, taps, s_h, [&](int row, int col, float v) {
            const unsigned m = s_m[(row + kTaps / 2) * (kPitchW * 4) + col + kTaps / 2];
#pragma unroll
            for (int r = 0; r < kMaxR; r++) {
                if (r < R) {
                    const bool in = (m >> r) & 1u;
                    cssim[r] += in ? v : 0.f;
                    cpos[r] += in && ch == 0 ? 1u : 0u;
                }
            }
        });
    }

    // ---- block sums in a fixed order: wave butterfly, then the four waves in order
#pragma unroll
    for (int r = 0; r < kMaxR; r++) {
        if (r < R) {
            const unsigned w_n = wave_sum<unsigned>(cn[r]), w_pos = wave_sum<unsigned>(cpos[r]);
            const unsigned w_sad = wave_sum<unsigned>(csad[r]), w_ssd = wave_sum<unsigned>(cssd[r]);
            const double w_ssim = wave_sum<double>((double)cssim[r]);
            if ((t & 63) == 0) {
                RPartial p;
                p.n = w_n, p.positions = w_pos, p.sad = w_sad, p.ssd = w_ssd, p.ssim = w_ssim;
                s_red[(t >> 6) * kMaxR + r] = p;
            }
        }
    }
    __syncthreads();
    if (t < R) {
        const RPartial p0 = s_red[t], p1 = s_red[kMaxR + t], p2 = s_red[2 * kMaxR + t], p3 = s_red[3 * kMaxR + t];
        RPartial p;
        p.n = (p0.n + p1.n) + (p2.n + p3.n);
        p.positions = (p0.positions + p1.positions) + (p2.positions + p3.positions);
        p.sad = (p0.sad + p1.sad) + (p2.sad + p3.sad);
        p.ssd = (p0.ssd + p1.ssd) + (p2.ssd + p3.ssd);
        p.ssim = (p0.ssim + p1.ssim) + (p2.ssim + p3.ssim);
        out[t] = p;
    }
}

// grid (tiles_max, npairs): block (x, y) = tile x of pair y; pairs with fewer tiles leave their spare blocks idle
__global__ __launch_bounds__(kThreads) void region_metrics_tiles(const pg_region_pair* __restrict__ jobs, RPartial* __restrict__ partials, int tiles_max,
                                                                 Taps taps, Regions regions) {
    __shared__ unsigned s_px[2 * kMaxC * kPlaneW];
    __shared__ unsigned s_lab[kPlaneW];
    __shared__ __attribute__((aligned(16))) float s_h[5 * kIn * kTile];
    __shared__ RPartial s_red[(kThreads / 64) * kMaxR];
    const pg_region_pair job = jobs[blockIdx.y];
    if (job.h <= kHalo || job.w <= kHalo) return;                     // (refused on the host; a table that differs from the host's copy launches nothing wild)
    const int tiles_x = (job.w - kHalo + kTile - 1) / kTile, tiles_y = (job.h - kHalo + kTile - 1) / kTile;
    const int tile = blockIdx.x;
    if (tile >= tiles_x * tiles_y) return;                            // uniform over the block: no lane reaches a barrier
    RPartial* out = partials + ((int64_t)blockIdx.y * tiles_max + tile) * regions.n;
    if (job.channels == 3)
        tile_body<3>(job, tile, tiles_x, out, taps, regions, s_px, s_lab, s_h, s_red);
    else
        tile_body<1>(job, tile, tiles_x, out, taps, regions, s_px, s_lab, s_h, s_red);
}

// grid (npairs, nregions), one wave each: the tiles' partials of that pair and region in a fixed order
__global__ __launch_bounds__(64) void region_metrics_finish(const pg_region_pair* __restrict__ jobs, const RPartial* __restrict__ partials, int tiles_max,
                                                            int npairs, int R, long long* __restrict__ counts, double* __restrict__ ssim_sum) {
    const int j = blockIdx.x, r = blockIdx.y;
    const pg_region_pair job = jobs[j];
    const int oh = job.h - kHalo, ow = job.w - kHalo;
    int n = oh > 0 && ow > 0 ? ((ow + kTile - 1) / kTile) * ((oh + kTile - 1) / kTile) : 0;
    n = n < tiles_max ? n : tiles_max;
    const RPartial* p = partials + (int64_t)j * tiles_max * R + r;
    unsigned long long cn = 0ull, cpos = 0ull, a = 0ull, b = 0ull;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) {
        const RPartial q = p[(int64_t)i * R];
        cn += q.n;
        cpos += q.positions;
        a += q.sad;
        b += q.ssd;
        s += q.ssim;
    }
    cn = wave_sum<unsigned long long>(cn);
    cpos = wave_sum<unsigned long long>(cpos);
    a = wave_sum<unsigned long long>(a);
    b = wave_sum<unsigned long long>(b);
    s = wave_sum<double>(s);
    if (threadIdx.x == 0) {
        const int64_t at = (int64_t)j * R + r, plane = (int64_t)npairs * R;
        counts[at] = (long long)cn;
        counts[plane + at] = (long long)a;
        counts[2 * plane + at] = (long long)b;
        counts[3 * plane + at] = (long long)cpos;
        ssim_sum[at] = s;
    }
}

// argument checks of a host table; tiles_max = the largest tile count of a pair
int check_table(const pg_region_pair* jobs, int npairs, int nregions, int* tiles_max) {
    if (!jobs || npairs <= 0 || nregions < 1 || nregions > kMaxR) return PG_ERR_INVALID_ARG;
    if (npairs > PG_METRIC_MAX_PAIRS) return PG_ERR_TOO_LARGE;
    int tm = 0;
    for (int j = 0; j < npairs; j++) {
        const pg_region_pair& q = jobs[j];
        if (!q.a || !q.b || !q.labels || q.h <= kHalo || q.w <= kHalo || (q.channels != 1 && q.channels != 3)) return PG_ERR_INVALID_ARG;
        if (q.a_pix_stride < q.channels || q.b_pix_stride < q.channels || q.l_pix_stride < 1) return PG_ERR_INVALID_ARG;
        if (q.a_row_stride < 1 || q.b_row_stride < 1 || q.l_row_stride < 1) return PG_ERR_INVALID_ARG;
        if ((int64_t)q.h * q.w * q.channels > INT32_MAX) return PG_ERR_TOO_LARGE;
        if (q.a_row_stride > INT64_MAX / q.h || q.b_row_stride > INT64_MAX / q.h || q.l_row_stride > INT64_MAX / q.h) return PG_ERR_TOO_LARGE;
        const int64_t tiles = (int64_t)((q.w - kHalo + kTile - 1) / kTile) * ((q.h - kHalo + kTile - 1) / kTile);
        if (tiles > INT32_MAX) return PG_ERR_TOO_LARGE;
        if (tiles > tm) tm = (int)tiles;
    }
    *tiles_max = tm;
    return PG_OK;
}

// grid (blocks, npairs): the blocks of a pair share its pixels in steps of kThreads * kRun
__global__ __launch_bounds__(kThreads) void label_confusion(const pg_label_pair* __restrict__ jobs, Luts luts, int K, unsigned long long* __restrict__ out) {
    __shared__ unsigned s_hist[PG_CONFUSION_MAX_CLASSES * PG_CONFUSION_MAX_CLASSES];
    __shared__ unsigned s_lutw[128];
    const int t = threadIdx.x;
    const pg_label_pair job = jobs[blockIdx.y];
    if (job.h < 1 || job.w < 1) return;
    const unsigned npix = (unsigned)job.h * (unsigned)job.w, w = (unsigned)job.w;      // (h * w < 2^31: checked on the host)
    if (blockIdx.x * (unsigned)(kThreads * kRun) >= npix) return;      // uniform over the block
    s_hist[t] = 0u;
    if (t < 128) s_lutw[t] = luts.w[t];
    __syncthreads();
    const unsigned char* s_lut = reinterpret_cast<const unsigned char*>(s_lutw);
    for (unsigned i0 = (blockIdx.x * kThreads + t) * kRun; i0 < npix; i0 += gridDim.x * (unsigned)(kThreads * kRun)) {
        unsigned y = i0 / w, x = i0 - y * w;
        int cur = -1;
        unsigned cnt = 0u;
#pragma unroll
        for (int k = 0; k < kRun; k++) {
            if (i0 + k < npix) {
                const unsigned pc = s_lut[job.pred[(int64_t)y * job.p_row_stride + (int64_t)x * job.p_pix_stride]];
                const unsigned tc = s_lut[256 + job.target[(int64_t)y * job.t_row_stride + (int64_t)x * job.t_pix_stride]];
                const int bin = pc < (unsigned)K && tc < (unsigned)K ? (int)(tc * K + pc) : -1;
                if (bin != cur) {
                    if (cur >= 0) atomicAdd(&s_hist[cur], cnt);
                    cur = bin;
                    cnt = 0u;
                }
                cnt++;
                if (++x == w) x = 0u, y++;
            }
        }
        if (cur >= 0) atomicAdd(&s_hist[cur], cnt);
    }
    __syncthreads();
    if (t < K * K && s_hist[t]) atomicAdd(out + (int64_t)blockIdx.y * K * K + t, (unsigned long long)s_hist[t]);
}

}  // namespace

PG_EXPORT int pg_region_metrics_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int64_t pg_region_pair_metrics_workspace(const pg_region_pair* jobs_host, int npairs, int nregions) {
    int tiles_max = 0;
    const int st = check_table(jobs_host, npairs, nregions, &tiles_max);
    if (st != PG_OK) return st;
    return (int64_t)npairs * tiles_max * nregions * (int64_t)sizeof(RPartial);
}

PG_EXPORT int pg_region_pair_metrics_u8(const pg_region_pair* jobs_host, const pg_region_pair* jobs_device, int npairs, const uint32_t* regions,
                                        int nregions, void* workspace, int64_t* counts, double* ssim_sum, void* stream) {
    int tiles_max = 0;
    const int st = check_table(jobs_host, npairs, nregions, &tiles_max);
    if (st != PG_OK) return st;
    if (!jobs_device || !regions || !workspace || !counts || !ssim_sum) return PG_ERR_INVALID_ARG;
    static const Taps taps = gaussian_taps();
    Regions reg;
    for (int r = 0; r < kMaxR; r++) reg.set[r] = r < nregions ? regions[r] : 0u;
    reg.n = nregions;
    hipLaunchKernelGGL(region_metrics_tiles, dim3((unsigned)tiles_max, (unsigned)npairs), dim3(kThreads), 0, (hipStream_t)stream, jobs_device,
                       (RPartial*)workspace, tiles_max, taps, reg);
    const int ls = pg::launch_status();
    if (ls != PG_OK) return ls;
    hipLaunchKernelGGL(region_metrics_finish, dim3((unsigned)npairs, (unsigned)nregions), dim3(64), 0, (hipStream_t)stream, jobs_device,
                       (const RPartial*)workspace, tiles_max, npairs, nregions, (long long*)counts, ssim_sum);
    return pg::launch_status();
}

PG_EXPORT int pg_label_confusion_u8(const pg_label_pair* jobs_host, const pg_label_pair* jobs_device, int npairs, const unsigned char* pred_lut,
                                    const unsigned char* target_lut, int classes, int64_t* out, void* stream) {
    if (!jobs_host || !jobs_device || !pred_lut || !target_lut || !out || npairs <= 0) return PG_ERR_INVALID_ARG;
    if (classes < 1 || classes > PG_CONFUSION_MAX_CLASSES) return PG_ERR_INVALID_ARG;
    if (npairs > PG_METRIC_MAX_PAIRS) return PG_ERR_TOO_LARGE;
    Luts luts;
    unsigned char* bytes = reinterpret_cast<unsigned char*>(luts.w);
    for (int i = 0; i < 256; i++) {
        if ((pred_lut[i] >= classes && pred_lut[i] != PG_LABEL_IGNORE) || (target_lut[i] >= classes && target_lut[i] != PG_LABEL_IGNORE)) return PG_ERR_INVALID_ARG;
        bytes[i] = pred_lut[i];
        bytes[256 + i] = target_lut[i];
    }
    int64_t npix_max = 0;
    for (int j = 0; j < npairs; j++) {
        const pg_label_pair& q = jobs_host[j];
        if (!q.pred || !q.target || q.h < 1 || q.w < 1 || q.p_pix_stride < 1 || q.t_pix_stride < 1 || q.p_row_stride < 1 || q.t_row_stride < 1) return PG_ERR_INVALID_ARG;
        if ((int64_t)q.h * q.w > INT32_MAX) return PG_ERR_TOO_LARGE;
        if (q.p_row_stride > INT64_MAX / q.h || q.t_row_stride > INT64_MAX / q.h) return PG_ERR_TOO_LARGE;
        if ((int64_t)q.h * q.w > npix_max) npix_max = (int64_t)q.h * q.w;
    }
    const int64_t per_block = (int64_t)kThreads * kRun * 2;            // two steps per block, up to kConfBlocksMax blocks per pair
    int64_t blocks = (npix_max + per_block - 1) / per_block;
    blocks = blocks < 1 ? 1 : (blocks > kConfBlocksMax ? kConfBlocksMax : blocks);
    hipLaunchKernelGGL(label_confusion, dim3((unsigned)blocks, (unsigned)npairs), dim3(kThreads), 0, (hipStream_t)stream, jobs_device, luts, classes,
                       (unsigned long long*)out);
    return pg::launch_status();
}
