// ADA discriminator augmentation (training/augment.py): the geometric warp of AugmentPipe and its adjoint, and the per-sample colour transform.
//
// Warp = reflect-pad by a per-sample-derived margin -> 2x upsample with the 12-tap sym6 filter -> per-sample affine bilinear grid_sample
// (align_corners=False, zeros outside) -> [the 2x downsample stays a pg_upfirdn2d call].  The margins (int32[4]) and the 2x3 sampling matrices are read
// on the device: the padded, upsampled image is never materialised; each output sample evaluates it at its bilinear footprint (7 padded rows x 7 padded
// columns, the union of the two corners' 6-tap polyphase windows -- bilinear weights and filter taps are both separable).
//
// Coordinates.  With G = G_inv of sample n (the pre-padding 3x3 matrix of augment.py:194-260) the reference's matrix chain
// (augment.py:286-296) maps output sample (ox, oy) of the [2(H+6), 2(W+6)] grid to the up-sampled, padded image at
//     ix = 2 (G00 x3 + G01 y3 + G02) + 2 mx0 + W - 1,   x3 = (ox + 1) / 2 - (W + 6) / 2      (and likewise iy with row 1, my0, H)
// which is evaluated here in double precision (the reference composes five float32 matrix products).
//
// Adjoint: gather over the output samples whose bilinear footprint covers each point of the up-sampled padded domain (the bounding box of the inverse-mapped
// square (u-1, u+1)^2, every candidate re-tested with the forward's own arithmetic), written to a worst-case-sized [2(3H-2), 2(3W-2)] plane (margins are
// clamped to <= W-1 / H-1); then one pass folds the polyphase upsample's adjoint and the reflection back onto [H, W].  No atomics: bit-identical per call.
#include "pg_common.h"

namespace {

constexpr int kTaps = 12;         // sym6
constexpr int kPad = kTaps / 4;   // Hz_pad of augment.py:276 (3)
constexpr int kCh = 4;            // channels per thread

struct Margins { int x0, y0, x1, y1; };

__device__ inline Margins load_margins(const int* m, int h, int w) {
    // the host clamps them to [0, W-1] / [0, H-1] already (augment.py:281-282); clamped again so that no value of the tensor can address outside x
    Margins r;
    r.x0 = min(max(m[0], 0), w - 1); r.y0 = min(max(m[1], 0), h - 1);
    r.x1 = min(max(m[2], 0), w - 1); r.y1 = min(max(m[3], 0), h - 1);
    return r;
}

// output sample -> up-sampled padded image coordinates
__device__ inline void map_point(const float* G, int ox, int oy, int h, int w, const Margins& m, double& ix, double& iy) {
    const double x3 = 0.5 * (ox + 1) - 0.5 * (w + 2 * kPad);
    const double y3 = 0.5 * (oy + 1) - 0.5 * (h + 2 * kPad);
    ix = 2.0 * ((double)G[0] * x3 + (double)G[1] * y3 + (double)G[2]) + 2.0 * m.x0 + (w - 1);
    iy = 2.0 * ((double)G[3] * x3 + (double)G[4] * y3 + (double)G[5]) + 2.0 * m.y0 + (h - 1);
}

// torch reflect padding of one index (single bounce: the margin is at most n-1), clamped for safety
__device__ inline int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// Bilinear x polyphase weights of one axis: `k` = 7 padded indices starting at `j0`; w[t] = 0 where the padded index is outside [0, np) or the bilinear
// corner outside [0, 2 np).  `idx[t]` = source index in [0, n) after reflection (0 where the weight is 0).  False if the coordinate is not finite / far out.
__device__ inline bool axis_weights(double c, int n, int m0, int np, const float* f, float wt[7], int idx[7]) {
    const int nu = 2 * np;
    if (!(c > -2.0 && c < (double)nu + 1.0)) return false;       // also rejects NaN: no corner can be inside
    const double fl = floor(c);
    const int u0 = (int)fl;
    const float t = (float)(c - fl);
    const float wa = (u0 >= 0 && u0 < nu) ? 1.0f - t : 0.0f;     // corner u0
    const float wb = (u0 + 1 >= 0 && u0 + 1 < nu) ? t : 0.0f;    // corner u0 + 1
    const int j0 = (u0 - 5) >> 1;                                 // floor((u0 - 5) / 2): first padded index under the two windows
#pragma unroll
    for (int q = 0; q < 7; q++) {
        const int j = j0 + q;
        const int ka = 5 + u0 - 2 * j, kb = ka + 1;               // upfirdn2d(up=2, pad 6/5, true convolution): y[u] = 2 sum_j x[j] f[5 + u - 2j]
        float v = 0.0f;
        if (ka >= 0 && ka < kTaps) v += wa * f[ka];
        if (kb >= 0 && kb < kTaps) v += wb * f[kb];
        const bool in = j >= 0 && j < np;
        wt[q] = in ? 2.0f * v : 0.0f;
        idx[q] = in ? reflect(j - m0, n) : 0;
    }
    return true;
}

__global__ void warp_forward(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ g_inv, const int* __restrict__ margins,
                             const float* __restrict__ filt, int C, int h, int w) {
    const int Wo = 2 * (w + 2 * kPad), Ho = 2 * (h + 2 * kPad);
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= Wo * Ho) return;
    const int chunks = (C + kCh - 1) / kCh;
    const int n = blockIdx.y / chunks, c0 = (blockIdx.y % chunks) * kCh;
    const int ox = pix % Wo, oy = pix / Wo;
    float f[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; k++) f[k] = filt[k];
    const Margins m = load_margins(margins, h, w);
    double ix, iy;
    map_point(g_inv + 9 * n, ox, oy, h, w, m, ix, iy);
    float wx[7], wy[7];
    int cx[7], cy[7];
    float acc[kCh] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (axis_weights(ix, w, m.x0, w + m.x0 + m.x1, f, wx, cx) && axis_weights(iy, h, m.y0, h + m.y0 + m.y1, f, wy, cy)) {
        for (int a = 0; a < 7; a++) {
            if (wy[a] == 0.0f) continue;
#pragma unroll
            for (int k = 0; k < kCh; k++) {
                if (c0 + k >= C) break;
                const float* row = x + (((int64_t)n * C + c0 + k) * h + cy[a]) * w;
                float s = 0.0f;
#pragma unroll
                for (int b = 0; b < 7; b++) s += wx[b] * row[cx[b]];
                acc[k] += wy[a] * s;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kCh; k++) {
        if (c0 + k >= C) break;
        y[(((int64_t)n * C + c0 + k) * Ho + oy) * Wo + ox] = acc[k];
    }
}

// adjoint, step 1: grid_sample's adjoint into the up-sampled padded domain (only its live [Hi, Wi] corner of the worst-case plane is written)
__global__ void warp_adjoint_gather(const float* __restrict__ dy, float* __restrict__ buf, const float* __restrict__ g_inv, const int* __restrict__ margins,
                                    int C, int h, int w) {
    const int Wo = 2 * (w + 2 * kPad), Ho = 2 * (h + 2 * kPad);
    const int Wmax = 2 * (3 * w - 2), Hmax = 2 * (3 * h - 2);
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= Wmax * Hmax) return;
    const int chunks = (C + kCh - 1) / kCh;
    const int n = blockIdx.y / chunks, c0 = (blockIdx.y % chunks) * kCh;
    const int ux = pix % Wmax, uy = pix / Wmax;
    const Margins m = load_margins(margins, h, w);
    const int Wi = 2 * (w + m.x0 + m.x1), Hi = 2 * (h + m.y0 + m.y1);
    if (ux >= Wi || uy >= Hi) return;
    const float* G = g_inv + 9 * n;
    // ix = A (ox + 1, oy + 1) + K  ->  (ox + 1, oy + 1) = A^-1 ((ix, iy) - K); the square (ux-1, ux+1) x (uy-1, uy+1) maps to a parallelogram
    const double a00 = G[0], a01 = G[1], a10 = G[3], a11 = G[4];
    // map_point written as ix = G00 (ox + 1) + G01 (oy + 1) + Kx (x3 = (ox + 1) / 2 - (W + 6) / 2), likewise iy
    const double Kx = -(w + 2 * kPad) * a00 - (h + 2 * kPad) * a01 + 2.0 * (double)G[2] + 2.0 * m.x0 + (w - 1);
    const double Ky = -(w + 2 * kPad) * a10 - (h + 2 * kPad) * a11 + 2.0 * (double)G[5] + 2.0 * m.y0 + (h - 1);
    const double det = a00 * a11 - a01 * a10;
    float acc[kCh] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (det != 0.0 && isfinite(det) && isfinite(Kx) && isfinite(Ky)) {
        const double i00 = a11 / det, i01 = -a01 / det, i10 = -a10 / det, i11 = a00 / det;
        double lo_x = 1e300, hi_x = -1e300, lo_y = 1e300, hi_y = -1e300;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double px = (q & 1 ? ux + 1.0 : ux - 1.0) - Kx, py = (q & 2 ? uy + 1.0 : uy - 1.0) - Ky;
            const double ax = i00 * px + i01 * py - 1.0, ay = i10 * px + i11 * py - 1.0;     // = (ox, oy)
            lo_x = fmin(lo_x, ax); hi_x = fmax(hi_x, ax); lo_y = fmin(lo_y, ay); hi_y = fmax(hi_y, ay);
        }
        // one sample of slack on every side against rounding; every candidate is re-tested below with the forward's arithmetic
        // (clamped in double before the conversion: an extreme matrix must not produce an out-of-range int)
        const int x_lo = (int)fmin(fmax(floor(lo_x) - 1.0, 0.0), (double)Wo), x_hi = (int)fmax(fmin(ceil(hi_x) + 1.0, (double)(Wo - 1)), -1.0);
        const int y_lo = (int)fmin(fmax(floor(lo_y) - 1.0, 0.0), (double)Ho), y_hi = (int)fmax(fmin(ceil(hi_y) + 1.0, (double)(Ho - 1)), -1.0);
        for (int oy = y_lo; oy <= y_hi; oy++) {
            for (int ox = x_lo; ox <= x_hi; ox++) {
                double ix, iy;
                map_point(G, ox, oy, h, w, m, ix, iy);
                const double fx = floor(ix), fy = floor(iy);
                float wgt_x, wgt_y;
                if (fx == (double)ux) wgt_x = 1.0f - (float)(ix - fx);
                else if (fx + 1.0 == (double)ux) wgt_x = (float)(ix - fx);
                else continue;
                if (fy == (double)uy) wgt_y = 1.0f - (float)(iy - fy);
                else if (fy + 1.0 == (double)uy) wgt_y = (float)(iy - fy);
                else continue;
                const float wgt = wgt_x * wgt_y;
#pragma unroll
                for (int k = 0; k < kCh; k++) {
                    if (c0 + k >= C) break;
                    acc[k] += wgt * dy[(((int64_t)n * C + c0 + k) * Ho + oy) * Wo + ox];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kCh; k++) {
        if (c0 + k >= C) break;
        buf[(((int64_t)n * C + c0 + k) * Hmax + uy) * Wmax + ux] = acc[k];
    }
}

// the padded indices that reflect onto source index i (at most three): itself, its mirror in the leading margin, its mirror in the trailing margin
__device__ inline int preimages(int i, int n, int m0, int m1, int j[3]) {
    int k = 0;
    j[k++] = i + m0;
    if (i >= 1 && i <= m0) j[k++] = m0 - i;
    if (i <= n - 2 && n - 1 - i <= m1) j[k++] = m0 + 2 * (n - 1) - i;
    return k;
}

// adjoint, step 2: the polyphase upsample's adjoint (12 taps per axis from each padded index) plus the reflection fold onto [H, W]
__global__ void warp_adjoint_fold(const float* __restrict__ buf, float* __restrict__ dx, const int* __restrict__ margins, const float* __restrict__ filt,
                                  int C, int h, int w) {
    const int Wmax = 2 * (3 * w - 2), Hmax = 2 * (3 * h - 2);
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= w * h) return;
    const int nc = blockIdx.y;
    const int x = pix % w, y = pix / w;
    float f[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; k++) f[k] = filt[k];
    const Margins m = load_margins(margins, h, w);
    const int Wi = 2 * (w + m.x0 + m.x1), Hi = 2 * (h + m.y0 + m.y1);
    int jx[3], jy[3];
    const int nx = preimages(x, w, m.x0, m.x1, jx), ny = preimages(y, h, m.y0, m.y1, jy);
    const float* plane = buf + (int64_t)nc * Hmax * Wmax;
    float acc = 0.0f;
    for (int a = 0; a < ny; a++) {
        for (int ky = 0; ky < kTaps; ky++) {
            const int uy = 2 * jy[a] - 5 + ky;
            if (uy < 0 || uy >= Hi) continue;
            const float* row = plane + (int64_t)uy * Wmax;
            float s = 0.0f;
            for (int b = 0; b < nx; b++) {
                const int u0 = 2 * jx[b] - 5;
#pragma unroll
                for (int kx = 0; kx < kTaps; kx++) {
                    const int ux = u0 + kx;
                    if (ux >= 0 && ux < Wi) s += f[kx] * row[ux];
                }
            }
            acc += f[ky] * s;
        }
    }
    dx[(int64_t)nc * h * w + pix] = 4.0f * acc;
}

// mode 0: y[c] = sum_k M[c][k] x[k] + M[c][C];  mode 1 (transpose): y[c] = sum_k M[k][c] x[k];  mode 2 (linear part): y[c] = sum_k M[c][k] x[k]
// M = [N, C, C + 1], C in {1, 3}.  Modes 1 and 2 are each other's adjoint: the backward of mode 0 is mode 1, the backward of mode 1 is mode 2.
template <int C>
__global__ void color_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mat, int hw, int mode) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= hw) return;
    const int n = blockIdx.y;
    const float* M = mat + n * C * (C + 1);
    float v[C];
#pragma unroll
    for (int k = 0; k < C; k++) v[k] = x[((int64_t)n * C + k) * hw + pix];
#pragma unroll
    for (int c = 0; c < C; c++) {
        float s = mode == 0 ? M[c * (C + 1) + C] : 0.0f;
#pragma unroll
        for (int k = 0; k < C; k++) s += (mode == 1 ? M[k * (C + 1) + c] : M[c * (C + 1) + k]) * v[k];
        y[((int64_t)n * C + c) * hw + pix] = s;
    }
}

// ---------------------------------------------------------------------------- late stages: imgfilter, noise, cutout (augment.py:372-431)
//
// One launch: a workgroup owns a kLateTH x kLateTW tile of one (sample, channel) plane.  It stages the tile with a kLateP-pixel halo in LDS (forward: the
// reflect-padded source, gathered; adjoint: the masked gradient, zero outside the image), runs the row pass into a second LDS array (every staged row, tile
// columns) and the column pass from there into registers; noise and cutout are the epilogue.  The padded image, the row-pass result and any workspace never
// reach global memory.  A sample's taps are uniform over the workgroup: they are read once per thread at a uniform address (scalar registers), centred in
// kLateTaps slots (zero beyond ntaps), so both passes unroll over compile-time tap indices; a copy in LDS serves the adjoint's edge terms.
// Pitches (107, 65 dwords) are odd: the row pass walks lanes down a column of the staged tile, the column pass across a row of the row-pass result.
//
// Adjoint of the reflect-padded correlation, per axis (p = taps / 2; dy = 0 outside [0, H)):
//     dx[i] = sum_k t[k] ( dy[i-k+p] + [1 <= i <= p] dy[-i-k+p] + [H-1-p <= i <= H-2] dy[2(H-1)-i-k+p] )
// The first term is the forward pass with the taps reversed; the two mirror terms are evaluated only by the outputs next to an edge, and every source they
// name lies in [i-p, i+p] clipped to the image, i.e. inside the staged halo.  A gather: no atomics, bit-identical per call.

constexpr int kLateTaps = 43;                 // Hz_fbank.shape[1]: the largest filter the kernel is built for
constexpr int kLateP = kLateTaps / 2;         // 21
constexpr int kLateTH = 32, kLateTW = 64;     // output tile
constexpr int kLateSH = kLateTH + 2 * kLateP; // 74 staged rows
constexpr int kLateSW = kLateTW + 2 * kLateP; // 106 staged columns
constexpr int kLateSPitch = kLateSW + 1;      // 107
constexpr int kLateMPitch = kLateTW + 1;      // 65
constexpr int kLateR = 8;                     // outputs per thread and pass (a sliding window of kLateR + 2 kLateP inputs)
constexpr int kLateThreads = 256;

// cutout mask of one pixel in the reference's float32 arithmetic (augment.py:427-430): 1 outside the box, 0 inside
__device__ inline float late_mask(const float* cut, int xi, int yi, int h, int w) {
#pragma clang fp contract(off)
    const bool mx = fabsf(((float)xi + 0.5f) / (float)w - cut[0]) >= cut[2] / 2.0f;
    const bool my = fabsf(((float)yi + 0.5f) / (float)h - cut[1]) >= cut[3] / 2.0f;
    return (mx || my) ? 1.0f : 0.0f;
}

// v -> M (v + noise sigma): the product is rounded before the sum (torch's `images + randn * sigma`), the mask multiplies by 0 or 1
__device__ inline float late_epilogue(float v, const float* noise, int64_t at, float sigma, const float* cut, int xi, int yi, int h, int w) {
#pragma clang fp contract(off)
    if (noise) {
        const float t = noise[at] * sigma;
        v = v + t;
    }
    if (cut) v = v * late_mask(cut, xi, yi, h, w);
    return v;
}

// without a filter: mode 0: y = M (x + noise sigma); modes 1, 2: y = M x.  One thread = kVec consecutive pixels of a row (kVec = 4: 16-byte loads and
// stores, taken when w % 4 == 0 and the pointers are 16-byte aligned; else 1); `noise` / `sigma` arrive null where the mode ignores them.
template <int kVec>
__global__ void late_pointwise(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ noise, const float* __restrict__ sigma,
                               const float* __restrict__ cut, int C, int h, int w) {
    typedef pg::vec_t<float, kVec> vec;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= h * w / kVec) return;
    const int n = blockIdx.y / C, pix = q * kVec;
    const int64_t at = (int64_t)blockIdx.y * h * w + pix;
    const int xi = pix % w, yi = pix / w;
    const float* cutn = cut ? cut + 4 * n : nullptr;
    const float sg = noise ? sigma[n] : 0.0f;
    vec v = *reinterpret_cast<const vec*>(x + at), nz;
    if (noise) nz = *reinterpret_cast<const vec*>(noise + at);
#pragma unroll
    for (int k = 0; k < kVec; k++) {
#pragma clang fp contract(off)
        float r = v.v[k];
        if (noise) {
            const float t = nz.v[k] * sg;
            r = r + t;
        }
        if (cutn) r = r * late_mask(cutn, xi + k, yi, h, w);
        v.v[k] = r;
    }
    *reinterpret_cast<vec*>(y + at) = v;
}

// One mirror term of the adjoint along an axis of length `n`: sum_k T[k] src[idx(k)], idx(k) = base - k, over the k whose idx lies in the image and in the
// staged range [origin, origin + staged) (`src` = staged element 0, `stride` dwords apart).  A rolled loop: only the outputs next to an edge come here.
__device__ inline float late_mirror(const float* T, const float* src, int stride, int base, int n, int origin, int staged) {
    const int klo = max(0, base - min(n, origin + staged) + 1), khi = min(kLateTaps - 1, base - max(0, origin));
    float s = 0.0f;
#pragma unroll 1
    for (int k = klo; k <= khi; k++) s += T[k] * src[(base - k - origin) * stride];
    return s;
}

template <bool kAdj>
__global__ __launch_bounds__(kLateThreads) void late_filter(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ taps, int ntaps,
                                                            const float* __restrict__ noise, const float* __restrict__ sigma,
                                                            const float* __restrict__ cut, int C, int h, int w, int tiles_x) {
    __shared__ float S[kLateSH * kLateSPitch];
    __shared__ float Mid[kLateSH * kLateMPitch];
    __shared__ float T[kLateTaps];
    const int tid = threadIdx.x;
    const int n = blockIdx.y / C;
    const int x0 = (blockIdx.x % tiles_x) * kLateTW, y0 = (blockIdx.x / tiles_x) * kLateTH;
    const int p = ntaps / 2, shift = kLateP - p;
    const float* plane = x + (int64_t)blockIdx.y * h * w;
    const float* cutn = cut ? cut + 4 * n : nullptr;

    // taps, centred in kLateTaps slots; the adjoint's main term runs the forward loop with the taps reversed
    float t[kLateTaps];
#pragma unroll
    for (int k = 0; k < kLateTaps; k++) {
        const int q = (kAdj ? kLateTaps - 1 - k : k) - shift;
        t[k] = (q >= 0 && q < ntaps) ? taps[n * ntaps + q] : 0.0f;
    }
    if (tid < kLateTaps) {
        const int q = tid - shift;
        T[tid] = (q >= 0 && q < ntaps) ? taps[n * ntaps + q] : 0.0f;      // unreversed, for the mirror terms
    }

    // stage the tile and its halo
    for (int e = tid; e < kLateSH * kLateSW; e += kLateThreads) {
        const int r = e / kLateSW, c = e % kLateSW;
        const int gy = y0 - kLateP + r, gx = x0 - kLateP + c;
        float v = 0.0f;
        if (kAdj) {
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
                v = plane[(int64_t)gy * w + gx];
                if (cutn) v = v * late_mask(cutn, gx, gy, h, w);
            }
        } else if (gy >= -p && gy < h + p && gx >= -p && gx < w + p) {   // further out only zero taps look: keep 0 x inf out of the sums
            v = plane[(int64_t)reflect(gy, h) * w + reflect(gx, w)];
        }
        S[r * kLateSPitch + c] = v;
    }
    __syncthreads();

    // row pass: every staged row, tile columns; one thread = kLateR consecutive columns of one row, lanes down the rows
    for (int task = tid; task < kLateSH * (kLateTW / kLateR); task += kLateThreads) {
        const int r = task % kLateSH, c0 = (task / kLateSH) * kLateR;
        const float* row = S + r * kLateSPitch;
        float acc[kLateR];
#pragma unroll
        for (int j = 0; j < kLateR; j++) acc[j] = 0.0f;
#pragma unroll
        for (int i = 0; i < kLateR + 2 * kLateP; i++) {
            const float v = row[c0 + i];
#pragma unroll
            for (int j = 0; j < kLateR; j++)
                if (i - j >= 0 && i - j < kLateTaps) acc[j] += t[i - j] * v;
        }
        if (kAdj) {
#pragma unroll
            for (int j = 0; j < kLateR; j++) {
                const int gx = x0 + c0 + j;
                if (gx >= w) continue;
                if (gx >= 1 && gx <= kLateP) acc[j] += late_mirror(T, row, 1, kLateP - gx, w, x0 - kLateP, kLateSW);
                if (gx >= w - 1 - kLateP && gx <= w - 2) acc[j] += late_mirror(T, row, 1, 2 * (w - 1) - gx + kLateP, w, x0 - kLateP, kLateSW);
            }
        }
#pragma unroll
        for (int j = 0; j < kLateR; j++) Mid[r * kLateMPitch + c0 + j] = acc[j];
    }
    __syncthreads();

    // column pass: one thread = kLateR consecutive rows of one column, lanes across the columns
    {
        const int c = tid % kLateTW, r0 = (tid / kLateTW) * kLateR;
        const float* col = Mid + c;
        float acc[kLateR];
#pragma unroll
        for (int j = 0; j < kLateR; j++) acc[j] = 0.0f;
#pragma unroll
        for (int i = 0; i < kLateR + 2 * kLateP; i++) {
            const float v = col[(r0 + i) * kLateMPitch];
#pragma unroll
            for (int j = 0; j < kLateR; j++)
                if (i - j >= 0 && i - j < kLateTaps) acc[j] += t[i - j] * v;
        }
        const int gx = x0 + c;
        if (gx >= w) return;
        const float sg = (!kAdj && noise) ? sigma[n] : 0.0f;
#pragma unroll
        for (int j = 0; j < kLateR; j++) {
            const int gy = y0 + r0 + j;
            if (gy >= h) continue;
            float v = acc[j];
            if (kAdj) {
                if (gy >= 1 && gy <= kLateP) v += late_mirror(T, col, kLateMPitch, kLateP - gy, h, y0 - kLateP, kLateSH);
                if (gy >= h - 1 - kLateP && gy <= h - 2) v += late_mirror(T, col, kLateMPitch, 2 * (h - 1) - gy + kLateP, h, y0 - kLateP, kLateSH);
            } else {
                const int64_t at = ((int64_t)blockIdx.y * h + gy) * w + gx;
                v = late_epilogue(v, noise, at, sg, cutn, gx, gy, h, w);
            }
            y[((int64_t)blockIdx.y * h + gy) * w + gx] = v;
        }
    }
}

bool warp_args_ok(int n, int c, int h, int w) {
    return n > 0 && c > 0 && h >= 2 && w >= 2 && n <= 65535 && (int64_t)n * ((c + kCh - 1) / kCh) <= 65535 && (int64_t)n * c <= 65535;
}

bool warp_size_ok(int h, int w) {     // 32-bit pixel indices within one plane of the worst-case workspace
    return h < (1 << 14) && w < (1 << 14) && (int64_t)(2 * (3 * h - 2)) * (2 * (3 * w - 2)) < 0x7fffffffLL;
}

}  // namespace

PG_EXPORT int pg_augment_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_augment_warp(const float* x, float* y, const float* g_inv, const int* margins, const float* f, int n, int c, int h, int w, void* stream) {
    if (!x || !y || !g_inv || !margins || !f) return PG_ERR_INVALID_ARG;
    if (!warp_args_ok(n, c, h, w)) return PG_ERR_INVALID_ARG;
    if (!warp_size_ok(h, w)) return PG_ERR_TOO_LARGE;
    const int pix = 4 * (w + 2 * kPad) * (h + 2 * kPad);
    const dim3 grid((pix + 255) / 256, n * ((c + kCh - 1) / kCh));
    hipLaunchKernelGGL(warp_forward, grid, dim3(256), 0, (hipStream_t)stream, x, y, g_inv, margins, f, c, h, w);
    return pg::launch_status();
}

PG_EXPORT int pg_augment_warp_adjoint(const float* dy, float* workspace, float* dx, const float* g_inv, const int* margins, const float* f,
                                      int n, int c, int h, int w, void* stream) {
    if (!dy || !workspace || !dx || !g_inv || !margins || !f) return PG_ERR_INVALID_ARG;
    if (!warp_args_ok(n, c, h, w)) return PG_ERR_INVALID_ARG;
    if (!warp_size_ok(h, w)) return PG_ERR_TOO_LARGE;
    hipStream_t s = (hipStream_t)stream;
    const int plane = (2 * (3 * h - 2)) * (2 * (3 * w - 2));
    hipLaunchKernelGGL(warp_adjoint_gather, dim3((plane + 255) / 256, n * ((c + kCh - 1) / kCh)), dim3(256), 0, s, dy, workspace, g_inv, margins, c, h, w);
    int st = pg::launch_status();
    if (st != PG_OK) return st;
    hipLaunchKernelGGL(warp_adjoint_fold, dim3((h * w + 255) / 256, n * c), dim3(256), 0, s, workspace, dx, margins, f, c, h, w);
    return pg::launch_status();
}

PG_EXPORT int pg_augment_color(const float* x, float* y, const float* mat, int n, int c, int hw, int mode, void* stream) {
    if (!x || !y || !mat || n <= 0 || hw <= 0 || n > 65535 || mode < 0 || mode > 2) return PG_ERR_INVALID_ARG;
    if (c != 1 && c != 3) return PG_ERR_UNSUPPORTED;
    const dim3 grid((hw + 255) / 256, n);
    if (c == 3) hipLaunchKernelGGL(color_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, x, y, mat, hw, mode);
    else hipLaunchKernelGGL(color_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, y, mat, hw, mode);
    return pg::launch_status();
}

PG_EXPORT int pg_augment_late(const float* x, float* y, const float* taps, int ntaps, const float* noise, const float* sigma, const float* cut,
                              int n, int c, int h, int w, int mode, void* stream) {
    if (!x || !y || n <= 0 || c <= 0 || h <= 0 || w <= 0 || mode < 0 || mode > 2 || (noise == nullptr) != (sigma == nullptr)) return PG_ERR_INVALID_ARG;
    if ((int64_t)n * c > 65535) return PG_ERR_INVALID_ARG;
    if ((int64_t)h * w >= 0x7fffffffLL) return PG_ERR_TOO_LARGE;
    hipStream_t s = (hipStream_t)stream;
    if (!taps) {
        const float* nz = mode == 0 ? noise : nullptr;
        const float* sg = mode == 0 ? sigma : nullptr;
        if (w % 4 == 0 && pg::aligned16(x) && pg::aligned16(y) && (!nz || pg::aligned16(nz)))
            hipLaunchKernelGGL(late_pointwise<4>, dim3((h * w / 4 + 255) / 256, n * c), dim3(256), 0, s, x, y, nz, sg, cut, c, h, w);
        else
            hipLaunchKernelGGL(late_pointwise<1>, dim3((h * w + 255) / 256, n * c), dim3(256), 0, s, x, y, nz, sg, cut, c, h, w);
        return pg::launch_status();
    }
    if (ntaps <= 0) return PG_ERR_INVALID_ARG;
    if (ntaps % 2 == 0 || ntaps > kLateTaps || h <= ntaps / 2 || w <= ntaps / 2) return PG_ERR_UNSUPPORTED;
    const int tiles_x = (w + kLateTW - 1) / kLateTW, tiles_y = (h + kLateTH - 1) / kLateTH;
    if ((int64_t)tiles_x * tiles_y > 0x7fffffffLL) return PG_ERR_TOO_LARGE;
    const dim3 grid(tiles_x * tiles_y, n * c);
    if (mode == 2)
        hipLaunchKernelGGL(late_filter<true>, grid, dim3(kLateThreads), 0, s, x, y, taps, ntaps, nullptr, nullptr, cut, c, h, w, tiles_x);
    else
        hipLaunchKernelGGL(late_filter<false>, grid, dim3(kLateThreads), 0, s, x, y, taps, ntaps, mode == 0 ? noise : nullptr, mode == 0 ? sigma : nullptr,
                           cut, c, h, w, tiles_x);
    return pg::launch_status();
}
