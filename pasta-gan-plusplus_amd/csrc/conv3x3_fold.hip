// Folded tail of the texture block (fp32 stack): the block ends with x = conv1(h') + skip(s') -- a bias-free 3x3 and a bias-free 1x1 over SPADE outputs that
// already carry their pre-activation -- and the only reader of x is the modulated 1x1 ToRGB head (demodulate=False, 3 outputs).  Per sample that is ONE linear
// map of (h', s') with 3 x 64 x 9 + 3 x 64 weights (composed by pg_conv1x1_fold_prep, conv1x1_fold.hip, in float64), so x need not exist:
//     r[n,o,y,x] = clamp( sum_{c,ky,kx} xa[n,c,y+ky-1,x+kx-1] * w[n,o,9c+3ky+kx] + sum_c xb[n,c,y,x] * w[n,o,9C+c] + bias[n,o] ) (+ skip[n,o,y,x]).
// Zero padding stays exact: neither folded layer has a bias, so zero samples of xa map to zero.
//   * a thread owns 4 adjacent pixels x 4 rows (16 x Cout sums in registers), a wave 256 columns x 4 rows, a workgroup four waves stacked: 16 rows.  Per channel
//     a wave loads the 6 rows of xa its 4 output rows touch and 4 rows of xb, 16 bytes per lane; the halo rows between the waves of a workgroup are re-read
//     from cache, so HBM sees each row of xa 18 / 16 times;
//   * the +-1 column neighbours come from the adjacent lane (one DPP move each); only lanes 0 and 63 load an extra sample, in ONE 4-byte request per row whose
//     other lanes are out of range;
//   * every load is a buffer load over ONE channel plane: rows above / below the image, columns beyond it and the unused lanes of the edge request fall outside
//     the descriptor's range and read as zero -- no branch, no select;
//   * the 10 x Cout weights of a channel are wave-uniform: scalar loads, consumed as the scalar operand of the FMAs;
//   * the next channel's 16 requests are issued before the current channel's 160 x Cout FMAs (two register sets, loop unrolled by two);
//   * a channel's 10 products per output are summed apart and added to the running sum once, so the long summation chain has C links.
// 4 * 2C bytes read + 4 * Cout written (+ 4 * Cout skip image) per pixel against 10 * C * Cout FMAs: HBM-bound while the FMAs issue at about half rate.
#include "pg_common.h"

namespace {
typedef float f32x4s __attribute__((ext_vector_type(4)));
typedef unsigned u32x4s __attribute__((ext_vector_type(4)));

constexpr int F3_ROWS = 4;                  // output rows per wave
constexpr int F3_WAVES = 4;                 // waves per workgroup, stacked vertically
constexpr int F3_COLS = 256;                // columns per wave
constexpr int F3_OOB = 0x40000000;          // a byte offset beyond every plane the entry point accepts (<= 2^29 bytes), also after adding or subtracting a row offset
constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138;     // lane l reads lane l + 1 / lane l - 1; a lane without that neighbour keeps `old`

template <int CTRL> __device__ __forceinline__ float dpp_or(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

struct F3Planes {          // one channel's samples of a wave: 6 rows of xa (+ the sample left of lane 0 / right of lane 63 in `e`), 4 rows of xb
    f32x4s a[F3_ROWS + 2];
    float e[F3_ROWS + 2];
    f32x4s b[F3_ROWS];
};

template <int CO>
__global__ __launch_bounds__(256, 2) void conv3x3_fold_head_kernel(const float* __restrict__ xa, const float* __restrict__ xb, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, const float* __restrict__ skip, float* __restrict__ y,
                                                                   int C, int H, int W, float clamp) {
    const int n = blockIdx.z;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int r0 = ((int)blockIdx.y * F3_WAVES + wave) * F3_ROWS;            // first output row of this wave
    if (r0 >= H) return;                                                     // wave-uniform; the kernel has no barrier
    const int col = (int)blockIdx.x * F3_COLS + lane * 4;
    const bool colok = col < W;                                              // W % 4 == 0: all four pixels or none
    const int plane_bytes = H * W * 4;
    // byte offsets inside a channel plane; whatever lies outside the image lies outside [0, plane_bytes) as an unsigned offset
    const int off_col = colok ? col * 4 : F3_OOB;
    const int off_edge = lane == 0 ? (col > 0 && colok ? (col - 1) * 4 : F3_OOB) : (lane == 63 && col + 4 < W ? (col + 4) * 4 : F3_OOB);
    int off_a[F3_ROWS + 2], off_e[F3_ROWS + 2];
#pragma unroll
    for (int j = 0; j < F3_ROWS + 2; j++) {
        const int r = r0 - 1 + j;
        const int ro = r >= 0 && r < H ? r * W * 4 : F3_OOB;                 // (r0 + 4 may lie more than a row below the image: no product that could wrap)
        off_a[j] = ro + off_col;
        off_e[j] = ro + off_edge;
    }
    const float* pa = xa + (int64_t)n * C * H * W;
    const float* pb = xb + (int64_t)n * C * H * W;
    const float* wn = w + (int64_t)n * CO * 10 * C;
    const int64_t HW = (int64_t)H * W;

    auto load = [&](int c, F3Planes& p) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pa + c * HW), 0, plane_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pb + c * HW), 0, plane_bytes, 0x00020000);
#pragma unroll
        for (int j = 0; j < F3_ROWS + 2; j++) p.a[j] = __builtin_bit_cast(f32x4s, __builtin_amdgcn_raw_buffer_load_b128(ra, off_a[j], 0, 0));
#pragma unroll
        for (int j = 0; j < F3_ROWS; j++) p.b[j] = __builtin_bit_cast(f32x4s, __builtin_amdgcn_raw_buffer_load_b128(rb, off_a[j + 1], 0, 0));
#pragma unroll
        for (int j = 0; j < F3_ROWS + 2; j++) p.e[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, off_e[j], 0, 0));
    };

    float acc[CO][F3_ROWS][4];
#pragma unroll
    for (int o = 0; o < CO; o++)
#pragma unroll
        for (int t = 0; t < F3_ROWS; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) acc[o][t][q] = 0.f;

    auto mac = [&](int c, const F3Planes& p) __attribute__((always_inline)) {
        float w3[CO][9], w1[CO];             // wave-uniform: scalar registers
#pragma unroll
        for (int o = 0; o < CO; o++) {
#pragma unroll
            for (int k = 0; k < 9; k++) w3[o][k] = wn[o * 10 * C + c * 9 + k];
            w1[o] = wn[o * 10 * C + 9 * C + c];
        }
        float v[F3_ROWS + 2][6];                                            // input row r0 - 1 + j with its left and right neighbour columns
#pragma unroll
        for (int j = 0; j < F3_ROWS + 2; j++) {
            v[j][0] = dpp_or<DPP_WAVE_SHR1>(p.e[j], p.a[j][3]);              // lane 0 keeps its own edge sample
            v[j][1] = p.a[j][0]; v[j][2] = p.a[j][1]; v[j][3] = p.a[j][2]; v[j][4] = p.a[j][3];
            v[j][5] = dpp_or<DPP_WAVE_SHL1>(p.e[j], p.a[j][0]);              // lane 63 likewise
        }
        // a channel's 10 products are summed on their own and added to the running sums once: the long chain has C links, not 10 C (its roundings are the
        // ones at the magnitude of the result)
#pragma unroll
        for (int t = 0; t < F3_ROWS; t++) {
            float part[CO][4];
#pragma unroll
            for (int o = 0; o < CO; o++)
#pragma unroll
                for (int q = 0; q < 4; q++) part[o][q] = p.b[t][q] * w1[o];
#pragma unroll
            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++)
#pragma unroll
                    for (int o = 0; o < CO; o++)
#pragma unroll
                        for (int q = 0; q < 4; q++) part[o][q] = __builtin_fmaf(v[t + ky][q + kx], w3[o][3 * ky + kx], part[o][q]);
#pragma unroll
            for (int o = 0; o < CO; o++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[o][t][q] += part[o][q];
        }
    };

    F3Planes pA, pB;
    load(0, pA);
    int c = 0;
    for (; c + 1 < C; c += 2) {
        load(c + 1, pB);
        __builtin_amdgcn_sched_barrier(0);
        mac(c, pA);
        if (c + 2 < C) load(c + 2, pA);
        __builtin_amdgcn_sched_barrier(0);
        mac(c + 1, pB);
    }
    if (c < C) mac(c, pA);

    if (!colok) return;
    const float cl = pg::clamp_bound(clamp);
#pragma unroll
    for (int o = 0; o < CO; o++) {
        const float bo = bias[n * CO + o];
#pragma unroll
        for (int t = 0; t < F3_ROWS; t++) {
            if (r0 + t < H) {
                const int64_t at = (((int64_t)n * CO + o) * H + (r0 + t)) * W + col;
                f32x4s r;
#pragma unroll
                for (int q = 0; q < 4; q++) r[q] = fminf(fmaxf(acc[o][t][q] + bo, -cl), cl);
                if (skip) r += *(const f32x4s*)(skip + at);
                *(f32x4s*)(y + at) = r;
            }
        }
    }
}
}  // namespace

PG_EXPORT int pg_conv3x3_fold_head(const float* xa, const float* xb, const float* w, const float* bias, const float* skip, float* y,
                                   int N, int C, int H, int W, int Cout, float clamp, void* stream) {
    if (!xa || !xb || !w || !bias || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Cout <= 0) return PG_ERR_INVALID_ARG;
    if (Cout > 4 || W % 4 != 0 || !pg::aligned16(xa) || !pg::aligned16(xb) || !pg::aligned16(y) || (skip && !pg::aligned16(skip))) return PG_ERR_UNSUPPORTED;
    if ((int64_t)H * W * 4 > (int64_t)1 << 29 || (int64_t)C * 10 * Cout > (int64_t)1 << 24) return PG_ERR_UNSUPPORTED;      // plane offsets are 32-bit, see F3_OOB
    const int64_t by = ((int64_t)H + F3_WAVES * F3_ROWS - 1) / (F3_WAVES * F3_ROWS);
    if (N > 65535 || by > 65535) return PG_ERR_TOO_LARGE;
    const dim3 grid((unsigned)((W + F3_COLS - 1) / F3_COLS), (unsigned)by, (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
#define PG_FOLD3(P) case P: hipLaunchKernelGGL((conv3x3_fold_head_kernel<P>), grid, dim3(64 * F3_WAVES), 0, s, xa, xb, w, bias, skip, y, C, H, W, clamp); break;
    switch (Cout) { PG_FOLD3(1) PG_FOLD3(2) PG_FOLD3(3) PG_FOLD3(4) }
#undef PG_FOLD3
    return pg::launch_status();
}
