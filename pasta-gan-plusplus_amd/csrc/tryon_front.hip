// The try-on loader's pre-routing maps on gfx950 (training/tryon_front.py): what ``TryOnTestSet.unrouted`` (training/dataset.py) builds per pixel, from
// the decoded files and the key-point tables of ``TryOnTestSet.raw``, bit for bit.  Three launches per batch, none of which reads anything back:
//   pg_tryon_front_stats     per-sample label-group counts, first rows and the skin histogram (integer atomics: run-to-run identical)
//   pg_tryon_front_bit_rows  the four arm bands (quadrilateral test, dilated along x) and the canvas mask eroded along x, one bit per pixel
//   pg_tryon_front_compose   resolves every data-dependent decision of ``_host_<part>`` from the statistics, once per workgroup, and writes every map
// The loader's rules: segments, discs and quadrilaterals in float64 in `_Raster`'s operation order (nothing contracted: the pragma below; the discs
// are integer arithmetic); square dilation and the 8 x 8 erosion as a pass along x (bit rows) and a pass along y (compose); images pad with 255,
// everything else with 0.  Only the pose primitives are culled by bounding box (a segment reaches 2.5 pixels, a disc less than 5: the boxes grow by 3 and
// 5); a quadrilateral is tested at every pixel, because a degenerate one (a limb of zero length) covers the whole frame under `_Raster.quad`'s rule.
// PG_TRYON_OUTFIT is PG_TRYON_FULL with the lower garment cut from a second clothes source (lower_src_img / lower_src_parsing): the statistics count that
// source's label groups too, compose reads it through the same padded-frame loads as the clothes source and writes it out padded (lower_clothes).
// Memory-bound streams: one lane = 4 consecutive pixels of a row, the uint8 sides move as dwords (byte loads where W or left is no multiple of 4).
#include "pg_common.h"
#include "pg_stage.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace {

using namespace pg::stage;       // byte_of, load_px4

constexpr int kStats = PG_FRONT_STATS, kPrims = PG_FRONT_PRIMS;
constexpr int kLowerCnt = 784;                           // stats[784..787]: the label-group counts of the lower clothes' parsing (outfit mode)
constexpr int kStatRows = 32;                            // rows per workgroup of the statistics kernel (a multiple of 4: its dwords stay aligned)
constexpr int kBandK[2] = {35, 28};                      // dilation of the upper-arm / fore-arm band (dataset.py BAND_K)
enum { TOPS = 0, DRESSES = 1, PANTS = 2, SKIRT = 3 };    // garment classes, and the label groups {5,7} {6} {9} {12} that start in them

__device__ __forceinline__ int group_of(uint32_t label) {
    return (label == 5u || label == 7u) ? 0 : label == 6u ? 1 : label == 9u ? 2 : label == 12u ? 3 : -1;
}

__host__ __device__ __forceinline__ bool no_canvas(int mode) { return mode == PG_TRYON_FULL || mode == PG_TRYON_OUTFIT; }

// ----------------------------------------------------------------------------------------------------------- statistics
// Grid: x = blocks of kStatRows rows of the W-wide sources, y = sample.  stats was zeroed by the entry point's memset node.
__global__ __launch_bounds__(256) void front_stats_kernel(pg_front_io io, int H, int W) {
    const int n = blockIdx.y;
    __shared__ int s_cnt[8], s_key[8], s_lcnt[4], s_hist[768];
    for (int i = threadIdx.x; i < 768; i += 256) s_hist[i] = 0;
    if (threadIdx.x < 8) { s_cnt[threadIdx.x] = 0; s_key[threadIdx.x] = 0; }
    if (threadIdx.x < 4) s_lcnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t P = (int64_t)H * W;                                        // H % 4 == 0: every sample starts on a dword
    const int y0 = blockIdx.x * kStatRows, y1 = y0 + kStatRows < H ? y0 + kStatRows : H;
    const uint32_t* pp = reinterpret_cast<const uint32_t*>(io.person_parsing + n * P);
    const uint32_t* cp = reinterpret_cast<const uint32_t*>(io.clothes_parsing + n * P);
    const uint32_t* lp4 = io.lower_src_parsing ? reinterpret_cast<const uint32_t*>(io.lower_src_parsing + n * P) : nullptr;      // (uniform)
    const uint8_t* img = io.person_img + n * P * 3;
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, key[8] = {0, 0, 0, 0, 0, 0, 0, 0}, lcnt[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)y0 * W / 4 + threadIdx.x; i < (int64_t)y1 * W / 4; i += 256) {
        const uint32_t pw = __builtin_nontemporal_load(pp + i), cw = __builtin_nontemporal_load(cp + i);
        if (lp4) {                                                           // the lower clothes' label groups: counts only (no rule reads their rows)
            const uint32_t lw = __builtin_nontemporal_load(lp4 + i);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int gl = group_of((lw >> (8 * k)) & 0xffu);
#pragma unroll
                for (int g = 0; g < 4; g++)
                    if (gl == g) lcnt[g]++;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t px = i * 4 + k;
            const int rkey = H - (int)(px / W);                              // larger = higher up; 0 = absent
            const uint32_t lp = (pw >> (8 * k)) & 0xffu, lc = (cw >> (8 * k)) & 0xffu;
            const int gp = group_of(lp), gc = group_of(lc);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                if (gp == g) { cnt[g]++; key[g] = rkey > key[g] ? rkey : key[g]; }
                if (gc == g) { cnt[4 + g]++; key[4 + g] = rkey > key[4 + g] ? rkey : key[4 + g]; }
            }
            if (lp == 10u || lp == 13u) {                                    // neck + face: the skin histogram (zero bytes are not counted)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const uint32_t v = img[px * 3 + c];
                    if (v) atomicAdd(&s_hist[c * 256 + (int)v], 1);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (cnt[j]) atomicAdd(&s_cnt[j], cnt[j]);
        if (key[j]) atomicMax(&s_key[j], key[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (lcnt[j]) atomicAdd(&s_lcnt[j], lcnt[j]);
    __syncthreads();
    int* st = io.stats + (int64_t)n * kStats;
    if (threadIdx.x < 8) {
        if (s_cnt[threadIdx.x]) atomicAdd(st + threadIdx.x, s_cnt[threadIdx.x]);
        if (s_key[threadIdx.x]) atomicMax(st + 8 + threadIdx.x, s_key[threadIdx.x]);
    }
    if (threadIdx.x < 4 && s_lcnt[threadIdx.x]) atomicAdd(st + kLowerCnt + threadIdx.x, s_lcnt[threadIdx.x]);
    for (int i = threadIdx.x; i < 768; i += 256)
        if (s_hist[i]) atomicAdd(st + 16 + i, s_hist[i]);
}

// ----------------------------------------------------------------------------------------------------------- the per-sample decisions
// `_garment_classes` (dataset.py) on the four group counts: map[g] = the class label group g ends in, cls[c] = the pixel count of class c.
__device__ void resolve_classes(const int* cnt, int* map, int* cls) {
    const int nt = cnt[0], nd = cnt[1], np = cnt[2], ns = cnt[3];
    map[0] = TOPS; map[1] = DRESSES; map[2] = PANTS; map[3] = SKIRT;
    int cT = nt, cD = nd, cP, cS;
    if (np > ns) { map[3] = PANTS; cP = np + ns; cS = 0; }                  // pants and skirt are merged into whichever is larger
    else { map[2] = SKIRT; cS = np + ns; cP = 0; }
    if (nd > 0) {
        if (cP > 0) { map[1] = TOPS; cT += nd; cD = 0; }
        else if (nd > nt + cS) {                                            // the dress swallows the top and the skirt
            map[0] = DRESSES;
            for (int g = 2; g < 4; g++)
                if (map[g] == SKIRT) map[g] = DRESSES;
            cD = nd + nt + cS; cT = 0; cS = 0;
        } else {
            if (nt > cS) { map[1] = SKIRT; cS += nd; }
            else { map[1] = TOPS; cT += nd; }
            cD = 0;
        }
    }
    cls[TOPS] = cT; cls[DRESSES] = cD; cls[PANTS] = cP; cls[SKIRT] = cS;
}

struct Resolved {
    int up_src, lo_src;                     // whose parsing and image the upper / lower routing inputs are cut from: 0 person, 1 clothes, 2 lower clothes
    int up_bits, lo_bits, canvas_bits;      // bit g: label group g belongs to the mask (canvas: of the person's parsing)
    int label, bound_start;                 // bound = 255 from row bound_start on (H: nowhere)
};

__device__ __forceinline__ int groups_in(const int* map, int a, int b) {
    int m = 0;
    for (int g = 0; g < 4; g++)
        if (map[g] == a || map[g] == b) m |= 1 << g;
    return m;
}

// `_host_upper` / `_host_lower` / `_host_full` / `_host_outfit`: every ``if`` on a pixel sum, from the statistics.
__device__ void resolve(const int* st, const int* hip, int mode, int H, Resolved& r) {
    int pm[4], pc[4], cm[4], cc[4];
    resolve_classes(st, pm, pc);
    resolve_classes(st + 4, cm, cc);
    int key = 0;                                                            // first row of the person's lower garment (skirt + pants)
    for (int g = 0; g < 4; g++)
        if ((pm[g] == PANTS || pm[g] == SKIRT) && st[8 + g] > key) key = st[8 + g];
    const int ymin = key > 0 ? H - key : -1;
    r.bound_start = H;
    if (mode == PG_TRYON_UPPER) {
        const bool zero = cc[DRESSES] > 0;                                  // a dress replaces the person's lower garment entirely
        r.up_src = 1; r.up_bits = groups_in(cm, TOPS, DRESSES);
        r.lo_src = 0; r.lo_bits = zero ? 0 : groups_in(pm, PANTS, SKIRT);
        r.canvas_bits = r.lo_bits;
        r.label = (!zero && pc[PANTS] > 0) ? 0 : (!zero && pc[SKIRT] > 0) ? 1 : cc[DRESSES] > 0 ? 2 : 1;
        bool has = false;
        int top = 0;
        if (hip[0]) { top = ymin < 0 ? hip[1] : (ymin < hip[1] ? ymin : hip[1]); has = true; }
        else if (ymin >= 0) { top = ymin; has = true; }
        if (has && !zero) r.bound_start = top < 0 ? (H + top > 0 ? H + top : 0) : (top < H ? top : H);       // ``bound[top:]`` as NumPy slices it
    } else if (mode == PG_TRYON_LOWER) {
        const bool zero = pc[DRESSES] > 0;                                  // a person in a dress keeps it
        r.up_src = 0; r.up_bits = groups_in(pm, TOPS, DRESSES);
        r.lo_src = 1; r.lo_bits = zero ? 0 : groups_in(cm, PANTS, SKIRT);
        r.canvas_bits = r.up_bits;
        r.label = (!zero && cc[PANTS] > 0) ? 0 : (!zero && cc[SKIRT] > 0) ? 1 : pc[DRESSES] > 0 ? 2 : 1;
        if (ymin >= 0 && !zero) r.bound_start = ymin;
    } else if (mode == PG_TRYON_OUTFIT) {                                   // `_host_full` with the lower garment's classes from the lower clothes
        int lm[4], lc[4];
        resolve_classes(st + kLowerCnt, lm, lc);
        r.up_src = 1; r.up_bits = groups_in(cm, TOPS, DRESSES);
        r.lo_src = 2; r.lo_bits = groups_in(lm, PANTS, SKIRT);
        r.canvas_bits = 0;
        r.label = lc[PANTS] > 0 ? 0 : lc[SKIRT] > 0 ? 1 : cc[DRESSES] > 0 ? 2 : 1;
    } else {
        r.up_src = r.lo_src = 1;
        r.up_bits = groups_in(cm, TOPS, DRESSES); r.lo_bits = groups_in(cm, PANTS, SKIRT);
        r.canvas_bits = 0;
        r.label = cc[PANTS] > 0 ? 0 : cc[SKIRT] > 0 ? 1 : cc[DRESSES] > 0 ? 2 : 1;
    }
}

// ----------------------------------------------------------------------------------------------------------- bit rows
// Grid: x = blocks of 256 / words rows, y = plane (0..3 the arm bands, 4 the canvas mask), z = sample.  One thread = one 32-pixel word.
__global__ __launch_bounds__(256) void front_bit_rows_kernel(pg_front_io io, int H, int W, int left, int mode, int words) {
    const int n = blockIdx.z, plane = blockIdx.y;
    __shared__ uint32_t s_raw[256];
    __shared__ Resolved s_r;
    if (plane < 4 ? io.band_absent[n * 4 + plane] != 0 : no_canvas(mode)) return;      // (uniform over the workgroup) never read by compose
    const int rows_pb = 256 / words;
    const int lr = threadIdx.x / words, w = threadIdx.x - lr * words;
    const int y = blockIdx.x * rows_pb + lr;
    const bool active = lr < rows_pb && y < H;
    uint32_t raw = 0u;
    if (plane < 4) {
        // `_Raster.quad`: the pixels on the same side of all four edges, the side of the third corner (1.0 when it lies on the first edge)
        double p[8], ex[4], ey[4];
#pragma unroll
        for (int i = 0; i < 8; i++) p[i] = io.bands[((int64_t)n * 4 + plane) * 8 + i];
#pragma unroll
        for (int i = 0; i < 4; i++) { ex[i] = p[2 * ((i + 1) & 3)] - p[2 * i]; ey[i] = p[2 * ((i + 1) & 3) + 1] - p[2 * i + 1]; }
        const double v = ex[0] * (p[5] - p[1]) - ey[0] * (p[4] - p[0]);
        const double sign = v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : v == 0.0 ? 1.0 : v;             // (NaN stays NaN: nothing is inside)
        if (active) {
            const double yd = (double)y;
            for (int j = 0; j < 32; j++) {
                const int x = 32 * w + j;
                if (x >= H) break;
                const double xd = (double)x;
                bool inside = true;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const double cross = ex[i] * (yd - p[2 * i + 1]) - ey[i] * (xd - p[2 * i]);
                    inside = inside && (cross * sign >= 0.0);
                }
                raw |= (inside ? 1u : 0u) << j;
            }
        }
    } else {
        if (threadIdx.x == 0) resolve(io.stats + (int64_t)n * kStats, io.hip_top + n * 2, mode, H, s_r);
        __syncthreads();
        const int bits = s_r.canvas_bits;
        if (active) {
            const uint8_t* row = io.person_parsing + ((int64_t)n * H + y) * W;
            for (int j = 0; j < 32; j++) {
                const int x = 32 * w + j, xs = x - left;
                bool on = x >= H;                                           // taps outside the frame are ignored: they read as set
                if (x < H && xs >= 0 && xs < W) {
                    const int g = group_of(row[xs]);
                    on = g >= 0 && ((bits >> g) & 1);
                }
                raw |= (on ? 1u : 0u) << j;
            }
        }
    }
    s_raw[threadIdx.x] = raw;
    __syncthreads();
    if (!active) return;
    const uint32_t outside = plane < 4 ? 0u : 0xffffffffu;
    const uint32_t prev = w > 0 ? s_raw[threadIdx.x - 1] : outside, next = w + 1 < words ? s_raw[threadIdx.x + 1] : outside;
    uint32_t out = raw;
    if (plane < 4) {                                                        // `_Raster.dilate` along x: k / 2 before, k - 1 - k / 2 after
        const int k = kBandK[plane & 1], lo = k / 2, hi = k - 1 - k / 2;
        for (int d = 1; d <= lo; d++) out |= (raw << d) | (prev >> (32 - d));
        for (int d = 1; d <= hi; d++) out |= (raw >> d) | (next << (32 - d));
    } else {                                                                // `_erode_white` along x: taps -4 .. +3
        for (int d = 1; d <= 4; d++) out &= (raw << d) | (prev >> (32 - d));
        for (int d = 1; d <= 3; d++) out &= (raw >> d) | (next << (32 - d));
    }
    io.bit_rows[(((int64_t)n * 5 + plane) * H + y) * words + w] = out;
}

// ----------------------------------------------------------------------------------------------------------- compose
// `_Raster.segment` (thickness 5) at pixel (px, py) of the W-wide frame, float64 in NumPy's operation order.
__device__ __forceinline__ bool in_segment(int px, int py, int x0, int y0, int x1, int y1) {
    const double d0 = (double)((int64_t)x1 - x0), d1 = (double)((int64_t)y1 - y0);
    const double ln = d0 * d0 + d1 * d1;
    double t = 0.0;
    if (ln != 0.0) {
        t = ((double)((int64_t)px - x0) * d0 + (double)((int64_t)py - y0) * d1) / ln;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double ex = (double)px - ((double)x0 + t * d0), ey = (double)py - ((double)y0 + t * d1);
    return ex * ex + ey * ey <= 6.25;
}

__device__ __forceinline__ bool in_disc(int px, int py, int x0, int y0) {
    const int64_t dx = (int64_t)px - x0, dy = (int64_t)py - y0;
    return dx * dx + dy * dy < 25;
}

// 4 pixels x C bytes of a W-wide source row at source column xs (the frame's column minus left); columns outside the source read as `fill`.
template <int C>
__device__ __forceinline__ void load_src4(const uint8_t* __restrict__ row, int xs, int W, uint32_t fill, bool fast, uint32_t (&w)[C]) {
    if (fast && xs >= 0 && xs + 4 <= W) {                                   // left % 4 == 0 and W % 4 == 0: whole aligned dwords
        load_px4<C>(row + (int64_t)xs * C, w);
        return;
    }
#pragma unroll
    for (int i = 0; i < C; i++) w[i] = fill * 0x01010101u;
    if (xs + 3 < 0 || xs >= W) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (xs + k < 0 || xs + k >= W) continue;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int i = k * C + c, sh = (i & 3) * 8;
            w[i >> 2] = (w[i >> 2] & ~(0xffu << sh)) | ((uint32_t)row[(int64_t)(xs + k) * C + c] << sh);
        }
    }
}

// The 12-byte mask of 4 RGB pixels: 0xff in the three bytes of every pixel that is on.
__device__ __forceinline__ void rgb_mask(const bool (&on)[4], uint32_t (&m)[3]) {
    m[0] = (on[0] ? 0x00ffffffu : 0u) | (on[1] ? 0xff000000u : 0u);
    m[1] = (on[1] ? 0x0000ffffu : 0u) | (on[2] ? 0xffff0000u : 0u);
    m[2] = (on[2] ? 0x000000ffu : 0u) | (on[3] ? 0xffffff00u : 0u);
}

__device__ __forceinline__ void store3(uint8_t* __restrict__ p, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t* d = reinterpret_cast<uint32_t*>(p);
    __builtin_nontemporal_store(a, d);
    __builtin_nontemporal_store(b, d + 1);
    __builtin_nontemporal_store(c, d + 2);
}

// Grid: x = blocks of 256 lanes x 4 pixels over the H x H frame, y = sample.
__global__ __launch_bounds__(256) void front_compose_kernel(pg_front_io io, int H, int W, int left, int mode, int words, int fast) {
    const int n = blockIdx.y;
    __shared__ Resolved s_r;
    __shared__ int s_prim[kPrims][8];
    __shared__ int s_nprim;
    __shared__ int s_absent[4];
    __shared__ int s_med[3][3];                                             // per channel: count, the two middle bytes
    const int* st = io.stats + (int64_t)n * kStats;
    const int64_t q0 = (int64_t)blockIdx.x * 256;
    const int wy0 = (int)(q0 * 4 / H);
    int wy1 = (int)(((q0 + 255) * 4 + 3) / H);
    wy1 = wy1 < H ? wy1 : H - 1;

    if (threadIdx.x == 0) resolve(st, io.hip_top + n * 2, mode, H, s_r);
    if (threadIdx.x < 4) s_absent[threadIdx.x] = io.band_absent[n * 4 + threadIdx.x];
    if (threadIdx.x < 64) {                                                 // wave 0: the pose primitives that can reach this workgroup's rows, in order
        int row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool keep = false;
        if ((int)threadIdx.x < kPrims) {
#pragma unroll
            for (int i = 0; i < 8; i++) row[i] = io.pose_prims[((int64_t)n * kPrims + threadIdx.x) * 8 + i];
            if (row[0] == 1) {
                const int64_t lo = (row[2] < row[4] ? row[2] : row[4]) - 3LL, hi = (row[2] > row[4] ? row[2] : row[4]) + 3LL;
                keep = hi >= wy0 && lo <= wy1;
            } else if (row[0] == 2) {
                keep = (int64_t)row[2] + 5 >= wy0 && (int64_t)row[2] - 5 <= wy1;
            }
        }
        const unsigned long long kept = __ballot(keep);
        if (keep) {
            const int at = __popcll(kept & ((1ull << threadIdx.x) - 1ull));
#pragma unroll
            for (int i = 0; i < 8; i++) s_prim[at][i] = row[i];
        }
        if (threadIdx.x == 0) s_nprim = __popcll(kept);
    }
    if (blockIdx.x == 0 && threadIdx.x < 192) {                             // waves 0..2: the skin median of one channel each, from its histogram
        const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
        int bin[4], sum = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int b = 4 * lane + i;
            bin[i] = b ? st[16 + c * 256 + b] : 0;
            sum += bin[i];
        }
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const int total = __shfl(incl, 63, 64);
        const int k1 = (total - 1) / 2, k2 = total / 2;                     // the middle of the sorted bytes (k1 == k2 for an odd count)
        int before = incl - sum;
        if (lane == 0) s_med[c][0] = total;
        if (total > 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (before <= k1 && k1 < before + bin[i]) s_med[c][1] = 4 * lane + i;
                if (before <= k2 && k2 < before + bin[i]) s_med[c][2] = 4 * lane + i;
                before += bin[i];
            }
        }
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (threadIdx.x < 3) {
            const double m = (double)(s_med[threadIdx.x][1] + s_med[threadIdx.x][2]) / 2.0;      // .0 or .5: exact in float32
            io.skin[n * 3 + threadIdx.x] = s_med[threadIdx.x][0] > 0 ? (float)m : __builtin_nanf("");
        }
        if (threadIdx.x == 3) io.label[n] = s_r.label;
    }

    const int64_t q = q0 + threadIdx.x;
    if (q * 4 >= (int64_t)H * H) return;
    const int y = (int)(q * 4 / H), x = (int)(q * 4 - (int64_t)y * H);      // H % 4 == 0: the 4 pixels lie in one row
    const int xs = x - left;
    const int64_t src_row = ((int64_t)n * H + y) * W;
    const int64_t px = ((int64_t)n * H + y) * H + x;                        // first pixel in the batch of frames
    const Resolved r = s_r;

    uint32_t pi[3], ci[3], pp[1], cp[1];
    load_src4<3>(io.person_img + src_row * 3, xs, W, 255u, fast, pi);
    load_src4<3>(io.clothes_img + src_row * 3, xs, W, 255u, fast, ci);
    load_src4<1>(io.person_parsing + src_row, xs, W, 0u, fast, pp);
    load_src4<1>(io.clothes_parsing + src_row, xs, W, 0u, fast, cp);
    store3(io.image + px * 3, pi[0], pi[1], pi[2]);
    store3(io.clothes + px * 3, ci[0], ci[1], ci[2]);
    uint32_t li[3] = {0u, 0u, 0u}, lp[1] = {0u};                            // the lower clothes (outfit mode; uniform over the grid)
    if (mode == PG_TRYON_OUTFIT) {
        load_src4<3>(io.lower_src_img + src_row * 3, xs, W, 255u, fast, li);
        load_src4<1>(io.lower_src_parsing + src_row, xs, W, 0u, fast, lp);
        store3(io.lower_clothes + px * 3, li[0], li[1], li[2]);
    }

    // the routing inputs: garment masks from the resolved classes, the images under them
    bool up_on[4], lo_on[4], can_on[4];
    bool any_canvas = false, any_hand = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int gp = group_of(byte_of(pp, k)), gc = group_of(byte_of(cp, k));
        const int gu = r.up_src ? gc : gp, gl = r.lo_src == 2 ? group_of(byte_of(lp, k)) : r.lo_src ? gc : gp;
        up_on[k] = gu >= 0 && ((r.up_bits >> gu) & 1);
        lo_on[k] = gl >= 0 && ((r.lo_bits >> gl) & 1);
        can_on[k] = gp >= 0 && ((r.canvas_bits >> gp) & 1);
        any_canvas = any_canvas || can_on[k];
        const uint32_t lp = byte_of(pp, k);
        any_hand = any_hand || lp == 14u || lp == 15u;
    }
    uint32_t m[3];
    rgb_mask(up_on, m);
    store3(io.upper_mask + px * 3, m[0], m[1], m[2]);
    store3(io.upper_img + px * 3, (r.up_src ? ci[0] : pi[0]) & m[0], (r.up_src ? ci[1] : pi[1]) & m[1], (r.up_src ? ci[2] : pi[2]) & m[2]);
    rgb_mask(lo_on, m);
    store3(io.lower_mask + px * 3, m[0], m[1], m[2]);
    if (r.lo_src == 2) store3(io.lower_img + px * 3, li[0] & m[0], li[1] & m[1], li[2] & m[2]);
    else store3(io.lower_img + px * 3, (r.lo_src ? ci[0] : pi[0]) & m[0], (r.lo_src ? ci[1] : pi[1]) & m[1], (r.lo_src ? ci[2] : pi[2]) & m[2]);

    // canvas: the person's own garment under its mask eroded 8 x 8 -- the pass along y over the x-eroded bit rows (taps -4 .. +3, in the frame)
    const int word = x >> 5, sh = x & 31;                                   // x % 4 == 0: the 4 bits lie in one word
    if (io.canvas) {
        uint32_t e = 0u;
        if (any_canvas) {
            const uint32_t* rows = io.bit_rows + (((int64_t)n * 5 + 4) * H) * words + word;
            e = 0xffffffffu;
            const int ya = y - 4 > 0 ? y - 4 : 0, yb = y + 3 < H - 1 ? y + 3 : H - 1;
            for (int yy = ya; yy <= yb; yy++) e &= rows[(int64_t)yy * words];
            e >>= sh;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) can_on[k] = (e >> k) & 1u;
        rgb_mask(can_on, m);
        store3(io.canvas + px * 3, pi[0] & m[0], pi[1] & m[1], pi[2] & m[2]);
    }

    // retain mask: shoes + head, and the hand labels minus the two arm bands (the pass along y of their dilation)
    uint32_t band[4] = {0u, 0u, 0u, 0u};                                    // bit k: pixel k lies in the dilated band
    if (any_hand) {
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (s_absent[b]) { band[b] = 0xfu; continue; }
            const int kk = kBandK[b & 1], lo = kk / 2, hi = kk - 1 - kk / 2;
            const uint32_t* rows = io.bit_rows + (((int64_t)n * 5 + b) * H) * words + word;
            const int ya = y - lo > 0 ? y - lo : 0, yb = y + hi < H - 1 ? y + hi : H - 1;
            uint32_t o = 0u;
            for (int yy = ya; yy <= yb; yy++) o |= rows[(int64_t)yy * words];
            band[b] = (o >> sh) & 0xfu;
        }
    }
    uint32_t retain = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t lp = byte_of(pp, k);
        bool on = lp == 18u || lp == 19u || lp == 1u || lp == 2u || lp == 4u || lp == 13u;
        if (lp == 14u) on = !(((band[0] | band[1]) >> k) & 1u);
        if (lp == 15u) on = !(((band[2] | band[3]) >> k) & 1u);
        retain |= (on ? 1u : 0u) << (8 * k);
    }
    __builtin_nontemporal_store(retain, reinterpret_cast<uint32_t*>(io.retain_mask + px));

    if (io.sleeve) {
        uint32_t gp[1], s = 0u;
        load_src4<1>(io.garment_parsing + src_row, xs, W, 0u, fast, gp);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t g = byte_of(gp, k);
            s |= ((g == 10u || g == 11u) ? 1u : 0u) << (8 * k);
        }
        __builtin_nontemporal_store(s, reinterpret_cast<uint32_t*>(io.sleeve + px));
    }

    // pose map: drawn in the W-wide frame, later primitives over earlier ones, then padded with 0
    uint32_t po[3] = {0u, 0u, 0u};
    if (xs + 3 >= 0 && xs < W) {
        const int np = s_nprim;
        for (int i = 0; i < np; i++) {
            const int kind = s_prim[i][0], x0 = s_prim[i][1], y0 = s_prim[i][2], x1 = s_prim[i][3], y1 = s_prim[i][4];
            const int64_t reach = kind == 1 ? 3 : 5;
            const int64_t xa = (kind == 1 && x1 < x0 ? x1 : x0) - reach, xb = (kind == 1 && x1 > x0 ? x1 : x0) + reach;
            const int64_t ya = (kind == 1 && y1 < y0 ? y1 : y0) - reach, yb = (kind == 1 && y1 > y0 ? y1 : y0) + reach;
            if (y < ya || y > yb || xs + 3 < xa || xs > xb) continue;
            const uint32_t colour = (uint32_t)s_prim[i][5] | ((uint32_t)s_prim[i][6] << 8) | ((uint32_t)s_prim[i][7] << 16);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int xp = xs + k;
                if (xp < 0 || xp >= W) continue;
                if (kind == 1 ? in_segment(xp, y, x0, y0, x1, y1) : in_disc(xp, y, x0, y0)) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const int j = 3 * k + c, s2 = (j & 3) * 8;
                        po[j >> 2] = (po[j >> 2] & ~(0xffu << s2)) | (((colour >> (8 * c)) & 0xffu) << s2);
                    }
                }
            }
        }
    }
    store3(io.pose + px * 3, po[0], po[1], po[2]);

    if (x == 0) io.bound[(int64_t)n * H + y] = y >= r.bound_start ? 255 : 0;
}

int check_common(const pg_front_io* io, int n, int H, int W) {
    if (!io || n <= 0 || H <= 0 || W <= 0) return PG_ERR_INVALID_ARG;
    if (!io->person_img || !io->clothes_img || !io->person_parsing || !io->clothes_parsing || !io->stats) return PG_ERR_INVALID_ARG;
    if (W > H) return PG_ERR_INVALID_ARG;
    if (H % 4 || H > 4096) return PG_ERR_UNSUPPORTED;
    const void* al[] = {io->person_img, io->clothes_img, io->person_parsing, io->clothes_parsing, io->garment_parsing, io->stats, io->lower_src_img,
                        io->lower_src_parsing};
    for (const void* p : al)
        if (reinterpret_cast<uintptr_t>(p) & 3u) return PG_ERR_UNSUPPORTED;
    if (n > 65535) return PG_ERR_TOO_LARGE;
    return PG_OK;
}

int check_maps(const pg_front_io* io, int n, int H, int W, int left, int mode) {
    const int rc = check_common(io, n, H, W);
    if (rc != PG_OK) return rc;
    if (mode != PG_TRYON_UPPER && mode != PG_TRYON_LOWER && mode != PG_TRYON_FULL && mode != PG_TRYON_OUTFIT) return PG_ERR_INVALID_ARG;
    if (mode == PG_TRYON_OUTFIT && (!io->lower_src_img || !io->lower_src_parsing)) return PG_ERR_INVALID_ARG;
    if (left < 0 || left + W > H) return PG_ERR_INVALID_ARG;
    if (!io->bands || !io->band_absent || !io->hip_top || !io->bit_rows) return PG_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(io->bands) & 7u) || (reinterpret_cast<uintptr_t>(io->band_absent) & 3u) ||
        (reinterpret_cast<uintptr_t>(io->hip_top) & 3u) || (reinterpret_cast<uintptr_t>(io->bit_rows) & 3u))
        return PG_ERR_UNSUPPORTED;
    return PG_OK;
}

}  // namespace

PG_EXPORT int pg_tryon_front_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_tryon_front_stats(const pg_front_io* io, int n, int H, int W, void* stream) {
    const int rc = check_common(io, n, H, W);
    if (rc != PG_OK) return rc;
    const hipError_t e = hipMemsetAsync(io->stats, 0, (size_t)n * kStats * sizeof(int), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(front_stats_kernel, dim3((unsigned)((H + kStatRows - 1) / kStatRows), (unsigned)n), dim3(256), 0, (hipStream_t)stream, *io, H, W);
    return pg::launch_status();
}

PG_EXPORT int pg_tryon_front_bit_rows(const pg_front_io* io, int n, int H, int W, int left, int mode, void* stream) {
    const int rc = check_maps(io, n, H, W, left, mode);
    if (rc != PG_OK) return rc;
    const int words = (H + 31) / 32, rows_pb = 256 / words;
    hipLaunchKernelGGL(front_bit_rows_kernel, dim3((unsigned)((H + rows_pb - 1) / rows_pb), 5u, (unsigned)n), dim3(256), 0, (hipStream_t)stream, *io, H, W,
                       left, mode, words);
    return pg::launch_status();
}

PG_EXPORT int pg_tryon_front_compose(const pg_front_io* io, int n, int H, int W, int left, int mode, void* stream) {
    const int rc = check_maps(io, n, H, W, left, mode);
    if (rc != PG_OK) return rc;
    const void* out[] = {io->upper_img, io->lower_img, io->upper_mask, io->lower_mask, io->image, io->clothes, io->pose, io->retain_mask, io->bound,
                         io->skin, io->label, io->pose_prims};
    for (const void* p : out)
        if (!p) return PG_ERR_INVALID_ARG;
    if ((io->sleeve != nullptr) != (io->garment_parsing != nullptr)) return PG_ERR_INVALID_ARG;
    if ((io->canvas != nullptr) != !no_canvas(mode)) return PG_ERR_INVALID_ARG;
    if ((io->lower_clothes != nullptr) != (mode == PG_TRYON_OUTFIT)) return PG_ERR_INVALID_ARG;
    const void* al[] = {io->upper_img, io->lower_img, io->upper_mask, io->lower_mask, io->sleeve, io->image, io->clothes, io->pose, io->retain_mask,
                        io->canvas, io->skin, io->label, io->pose_prims, io->lower_clothes};
    for (const void* p : al)
        if (reinterpret_cast<uintptr_t>(p) & 3u) return PG_ERR_UNSUPPORTED;
    const int words = (H + 31) / 32, fast = (left % 4 == 0 && W % 4 == 0) ? 1 : 0;
    const int64_t quads = (int64_t)H * H / 4;
    hipLaunchKernelGGL(front_compose_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, *io, H, W, left, mode,
                       words, fast);
    return pg::launch_status();
}
