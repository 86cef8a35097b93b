// The tile machinery shared by image_metrics.hip and region_metrics.hip: one workgroup of 256 lanes = kTile x kTile (32 x 32) SSIM positions of one
// uint8 image pair, whose (32 + 10)^2 pixels sit in LDS as planar bytes (row pitch 44 B, so a lane's 14-byte tap span is four dword reads).
//   load_tile     global window -> planar LDS bytes: dwords where the address allows, single bytes at a row's ragged head and tail and on images whose
//                 pixel stride is not `channels`; never a byte outside the window.
//   tile_origin   the integer level the moments of one (tile, channel, image) are taken about.
//   ssim_channel  the five moment maps (a, b, a^2, b^2, ab) of one channel filtered along x from the bytes into LDS (42 x 32 floats each) and along y
//                 from there; the SSIM value of every position of the tile goes to a caller's sink (a plain sum, or sums per label region).
#pragma once
#include "pg_common.h"
#include <cmath>
#include <cstdint>

namespace pgm {

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

// One channel of one tile (ih x iw pixels under oh x ow positions; planes pa / pb, origins oa / ob): sink(row, col, value) receives the SSIM value
// of position (row, col) of the tile, each position once, a lane's positions in row order.  `s_h`: 5 * kIn * kTile floats, 16-byte aligned.
// Every lane of the workgroup must call it (two barriers); s_h may be rewritten on return.
template <typename Sink>
__device__ __forceinline__ void ssim_channel(const unsigned* pa, const unsigned* pb, float oa, float ob, int ih, int oh, int ow, const Taps& taps,
                                             float* s_h, Sink&& sink) {
    const int t = threadIdx.x;
    const float C1 = 6.5025f, C2 = 58.5225f;
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
                    sink(r0 + o, col, num / den);
                }
            }
        }
    }
    __syncthreads();                                                  // s_h is rewritten by the next channel
}

inline Taps gaussian_taps() {
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

}  // namespace pgm
