// The fp32 stride-2 3x3 convolution with padding 0 -- what follows the FIR pass of every `down = 2` 3x3 layer (conv2d_resample.py:119-122 -> conv2d_gradfix.conv2d,
// stride 2; ResBlock.conv0 and Conv2dLayer, networks.py:170-179) -- with its multiplies on the bf16 matrix pipe, in the three-term arithmetic of bf16x3.h.  Input [N, Cin, 2 OH + 1, 2 OW + 1] (any H, W >= 3: OH = (H - 3) / 2 + 1), output [N, Cout, OH, OW].
//
// The tile is what makes it pay.  An input sample of a stride-2 layer meets 9/4 taps per cout, not 9, so a staged and split 16-channel chunk has to meet MANY
// couts before the producers' round (stage, split, one barrier: ~2.7 k cycles whatever it feeds) hides behind the matrix pipe: here all 128 couts of a cout group.
//
//   * workgroup = 8 waves = ONE per CU: four producer waves and four multiplying waves (one of each per SIMD).  Tile = 4 x 16 outputs x 128 couts; multiplying wave
//     w = couts 32 w .. 32 w + 31 x the 64 outputs = two accumulators (output rows {0, 1} and {2, 3}; D column = 16 (row & 1) + column).  K chunk = 16 channels = one
//     MFMA K.  Per chunk a wave issues 9 taps x 6 plane products x 2 accumulators = 108 MFMAs, the workgroup 432.  The five small product
//     classes (smallest first) sum in an accumulator of their own that joins the result in the epilogue, and the leading products a0 b0 of a chunk in one that
//     starts at zero and joins the tile's sum by a VALU addition per chunk (see the K loop for the measurements that asked for it).
//   * input: the 9 x 33 halo of the tile.  Rows are 2 OW + 1 floats long, so no row is 16-byte aligned: a producer wave requests, per (halo row, channel), the ten
//     ALIGNED 16-byte words that cover the row's 33 samples (LDS-DMA, range-checked buffer loads) and applies the row's misalignment -- (first element index) & 3,
//     from the image's 16-byte-aligned base -- when it reads the samples back for the split.  Wave pw stages and splits halo rows pw, pw + 4 (and 8 for wave 0):
//     it depends on no other wave's requests.
//   * planes: [buffer 2][plane 3][k-half 2][halo row 9][column parity 2][17] x 16 B (8 channels of one pixel = the B operand of one MFMA lane); even and odd halo
//     columns apart, so the 16 lanes of an output row read 16 consecutive records for every tap (kx = 0 / 2: even records c / c + 1, kx = 1: odd record c).
//   * weights: never in LDS.  The stream is [cout group][chunk][m-block 4][tap 9][plane 3][k-half 2][32 couts][8 channels] bf16, so a wave's A fragment is one
//     contiguous, coalesced kilobyte.  A wave holds the 27 fragments of the current chunk in registers and, tap by tap, reloads each with the NEXT chunk's as soon as
//     its last MFMA has issued: a whole chunk (~3.5 k cycles) of lead on an L2-resident stream (442 KB at 64 -> 128), no weight barrier, no weight LDS traffic.
//   * one s_barrier per chunk.  Barrier g: the producers have completed planes[g & 1] of chunk g, the multiplying waves have finished chunk g - 1 (its buffer is free
//     for chunk g + 1).  The next chunk's rows are requested before a producer goes to the barrier.  No flags, no polling.
//   * epilogue: the stages ResBlock.conv0 / Conv2dLayer use on this geometry -- per-cout bias, linear | relu | lrelu, gain, clamp -- in pg_conv2d_forward's order.
//   * tile stream: persistent, conv2d_kernel.h's XCD-aware order, cout group fastest (the workgroups of an XCD share input rows in its L2).
//   * Cout > 128: further cout groups over the same staging code; the stream is zero-padded to whole groups (a wave whose 32 couts lie beyond
//     Cout multiplies zeros beside the waves that do not, and stores nothing).
//
//
// LDS map (83 328 bytes of dynamic LDS, one workgroup per CU):
//        0 .. 23 551   raw halo words: producer wave 0 [3 rows][16 channels][10 words] padded to 512 words, waves 1-3 [2 rows][16][10] = 320 words each
//   23 552 .. 82 303   planes [2 buffers][3 planes][2 k-halves][306 records] x 16 B (one buffer 29 376 bytes)
//   82 304 .. 83 327   bias [2 tiles][128] float32
// gfx950 compile (hipcc -O3 -Rpass-analysis=kernel-resource-usage): conv2d_s2x3 243 VGPRs, 0 AGPRs, 88 SGPRs, scratch 0 bytes per lane, ZERO spills (VGPR and
// SGPR), occupancy 2 waves per SIMD = the one 8-wave workgroup.  Of the 243: 108 hold the chunk's weights, 96 the three
// accumulator pairs, 24 the B ring.
#pragma once
#include "conv2d_kernel.h"
#include "bf16x3_pack.h"

#ifndef SX_EXP
#define SX_EXP 0         // dev ablations (results wrong by design; tools/s2x3_variants.py): 1 no MFMAs, 2 no operand split, 4 no halo loads, 8 no weight loads, 16 no output stores, 32 cycle stamps of wave 0 into y
#endif

namespace pgconv {

constexpr int SX_KC = 16;
constexpr int SX_TH = 4, SX_TW = 16;                                 // output tile
constexpr int SX_IH = 9, SX_IW = 33;                                 // its halo
constexpr int SX_RW = 10;                                            // 16-byte words staged per (halo row, channel): 40 floats cover 33 samples at any misalignment 0..3
constexpr int SX_RAW = (512 + 3 * 320) * 4;                          // floats: the four producer waves' regions [row of the wave][channel 16][10 words], wave 0's padded to whole requests
constexpr int SX_PR = 34;                                            // records per halo row: 17 even columns, then 17 odd (16 used)
constexpr int SX_NPIX = SX_IH * SX_PR;                               // 306
constexpr int SX_PLB = SX_NPIX * 32;                                 // bytes of one plane: [k-half][record] x 16 B
constexpr int SX_GROUP = 128;                                        // couts per tile
constexpr int SX_FRAG = 64 * 16;                                     // bytes of one A fragment
constexpr int SX_WSLAB = 27 * SX_FRAG;                               // one (group, chunk, m-block): [tap 9][plane 3] fragments
constexpr size_t SX_LDS = (size_t)SX_RAW * 4 + 2 * 3 * (size_t)SX_PLB + 2 * SX_GROUP * 4;      // 23 552 + 58 752 + 1 024 = 83 328 bytes

struct S2x3Params {
    const float* x; float* y; const unsigned char* wx3; const float* bias;
    int N, Cin, H, W, Cout, OH, OW;
    int tilesX, tilesY, groups, total_tiles;
    int64_t ys[4];
    int act; float alpha, gain, clamp;
};

__global__ __launch_bounds__(512, 1) void conv2d_s2x3(S2x3Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sx_smem[];
    float* raw = (float*)sx_smem;
    unsigned char* planes = sx_smem + SX_RAW * 4;                      // [2 buffers][3 planes][2 k-halves][306 records] x 16 B
    float* bias_s = (float*)(planes + 2 * 3 * SX_PLB);                 // [2 tiles][128]: staged by producer wave 0

    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    const unsigned smem_b = __builtin_amdgcn_readfirstlane(lds_offset((const float*)sx_smem));
    const int HW = p.H * p.W;
    const int nchunks = p.Cin / SX_KC;
    const int total = p.total_tiles;
    const int q8 = total >> 3, r8 = total & 7;
    const int my_tiles = (total - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int my_chunks = my_tiles * nchunks;

    auto decode = [&](int tile, int& n, int& oy0, int& ox0, int& grp) __attribute__((always_inline)) {
        const int xcd = tile & 7;
        int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (tile >> 3);
        grp = L % p.groups; L /= p.groups;
        const int tx = L % p.tilesX; L /= p.tilesX;
        const int ty = L % p.tilesY;
        n = L / p.tilesY;
        oy0 = ty * SX_TH; ox0 = tx * SX_TW;
    };
    // an image's samples are addressed from the 16-byte-aligned address at or below its first one; `delta` = the first sample's index from there (0..3)
    auto image_base = [&](int n, int& delta) __attribute__((always_inline)) {
        const uint64_t b = (uint64_t)(uintptr_t)(p.x + (int64_t)n * p.Cin * HW);
        delta = (int)((b & 15u) >> 2);
        return b & ~(uint64_t)15;
    };

    if (wave >= 4) {
        // ------------------------------------------------------------ producer waves.  Round g: wait for the own rows of chunk g (requested at the end of round g - 1), split
        // them into planes[g & 1], request the rows of chunk g + 1 (they travel while this wave sits at the barrier), barrier.
        const int pw = wave - 4;
        const int nrows = pw == 0 ? 3 : 2;
        const int nreq = pw == 0 ? 8 : 5;                              // 16-byte requests per lane and chunk: 480 (padded to 512) or 320 words
        const int reg_w = pw == 0 ? 0 : 512 + (pw - 1) * 320;          // first word of this wave's region
        unsigned xoff[8];
        i32x4 xrsrc;
        int c_tile = blockIdx.x, c_chunk = 0;                          // the chunk being REQUESTED
        int s_tile = blockIdx.x, s_chunk = 0, s_sb = 0, s_grp = 0, s_par = 0;      // the chunk being SPLIT; s_sb = (delta + gy0 * W) & 3 of its tile
        const int w3 = p.W & 3, hw3 = HW & 3;
        auto request_rows = [&]() __attribute__((always_inline)) {
            if (c_chunk == 0) {
                int n, oy0, ox0, grp, delta;
                decode(c_tile, n, oy0, ox0, grp);
                const uint64_t base = image_base(n, delta);
                const int gx0 = 2 * ox0;
                const int ncols = p.W - gx0 < SX_IW ? p.W - gx0 : SX_IW;       // samples of a halo row inside the image
                int ll = lane;
                asm volatile("" : "+v"(ll));
#pragma unroll
                for (int i = 0; i < 8; i++) {                          // (row of the wave, channel, word of the row)
                    const int f = i * 64 + ll;
                    const int ri = f / 160, rem = f % 160;
                    const int c = rem / SX_RW, wd = rem % SX_RW;
                    const int row = ri == 0 ? pw : (ri == 1 ? pw + 4 : 8);
                    const int gy = 2 * oy0 + row;
                    const int e0 = delta + c * HW + gy * p.W + gx0;    // index of the row's first sample from the aligned base (< 2^29: checked by the launcher)
                    // a word is requested when it holds a sample of the image's row: nothing beyond the 16-byte word that holds the image's last sample is touched
                    const bool ok = ri < nrows && gy < p.H && 4 * wd < (e0 & 3) + ncols;
                    xoff[i] = ok ? (unsigned)((e0 & ~3) + 4 * wd) * 4u : 0x80000000u;
                }
                xrsrc[0] = (int)(unsigned)base;
                xrsrc[1] = (int)(unsigned)(base >> 32) & 0xffff;
                xrsrc[2] = (p.Cin * HW + 4) * 4;
                xrsrc[3] = 0x00020000;
            }
            i32x4 rs;                                                  // (the descriptor is carried across the chunk loop: back onto the scalar unit for the DMA's operand)
#pragma unroll
            for (int i = 0; i < 4; i++) rs[i] = __builtin_amdgcn_readfirstlane(xrsrc[i]);
            const unsigned xs_b = smem_b + (unsigned)reg_w * 16u;
            const int soff = c_chunk * SX_KC * HW * 4;                 // (a multiple of 64 bytes: the words stay aligned)
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (i < nreq && !(SX_EXP & 4)) dma_dwordx4_buf(rs, xs_b + 1024u * i, xoff[i], soff);
            if (++c_chunk == nchunks) { c_chunk = 0; c_tile += gridDim.x; }
        };
        auto split_rows = [&](int g) __attribute__((always_inline)) {
            if (s_chunk == 0) {
                int n, oy0, ox0, delta;
                decode(s_tile, n, oy0, ox0, s_grp);
                image_base(n, delta);
                s_sb = (delta + ((2 * oy0) & 3) * w3) & 3;
            }
            if (pw == 0 && s_chunk + 1 == nchunks) {
                // the tile's 128 bias values for the multiplying waves' epilogue: published by this round's barrier, read after the next one; two buffers, as the
                // epilogue of a two-chunk tile runs beside the round that stages its successor's.  (Nothing of this wave is in flight here: ld_opaque's wait is its own.)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int co = s_grp * SX_GROUP + 64 * h + lane;
                    bias_s[s_par * SX_GROUP + 64 * h + lane] = (p.bias && co < p.Cout) ? ld_opaque(p.bias + co) : 0.f;
                }
            }
            unsigned char* pl_b = planes + (size_t)(g & 1) * 3 * SX_PLB;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int task = lane + 64 * i;                        // (row of the wave, k-half, column): 66 per row
                if (task < nrows * 66) {
                    const int ri = task / 66, rem = task - ri * 66;
                    const int kh = rem >= SX_IW ? 1 : 0, col = rem - SX_IW * kh;
                    const int row = ri == 0 ? pw : (ri == 1 ? pw + 4 : 8);
                    const int sh_row = s_sb + (row & 3) * w3;          // + channel * HW: the misalignment of (row, channel), mod 4
                    const float* rp = raw + (reg_w + ri * 160 + (8 * kh) * SX_RW) * 4 + col;
                    x3_u32x4 pl[3];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        // channel 8 kh + 2 j (+ 1) of the chunk; 16 HW = 0 mod 4, so the chunk does not enter
                        const int ca = 8 * kh + 2 * j, cb = ca + 1;
                        const float va = rp[ca % 8 * 40 + ((sh_row + ca * hw3) & 3)], vb = rp[cb % 8 * 40 + ((sh_row + cb * hw3) & 3)];
                        unsigned p0, p1, p2;
                        if (SX_EXP & 2) { p0 = __float_as_uint(va); p1 = __float_as_uint(vb); p2 = p0; }
                        else x3_split_pair(va, vb, p0, p1, p2);
                        pl[0][j] = p0; pl[1][j] = p1; pl[2][j] = p2;
                    }
                    unsigned char* dst = pl_b + (size_t)(kh * SX_NPIX + row * SX_PR + (col & 1) * 17 + (col >> 1)) * 16;
                    *(x3_u32x4*)(dst) = pl[0];
                    *(x3_u32x4*)(dst + SX_PLB) = pl[1];
                    *(x3_u32x4*)(dst + 2 * SX_PLB) = pl[2];
                }
            }
            if (++s_chunk == nchunks) { s_chunk = 0; s_tile += gridDim.x; s_par ^= 1; }
        };
        // Barriers: s_barrier counts all eight waves; every wave executes my_chunks + 1 of them.
        request_rows();                                                // chunk 0
        for (int g = 0; g < my_chunks; g++) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the rows of chunk g are home (nothing younger is in flight)
            split_rows(g);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // the raw rows have been read (their region may be overwritten), the planes written
            if (g + 1 < my_chunks) request_rows();                     // the 8 / 5 row requests stay in flight across the barrier
            asm volatile("s_barrier" ::: "memory");
        }
        asm volatile("s_barrier" ::: "memory");                       // barrier my_chunks: nothing left to produce
        return;
    }

    // ---------------------------------------------------------------- multiplying waves
    const int half = lane >> 5, l31 = lane & 31;
    const int orow = l31 >> 4, ocol = l31 & 15;                        // this lane's D column: output row (of the accumulator's two) and column
    f32x16 acc[2], accs[2];                                            // per accumulator tile: the sum of the leading products a0 b0 (joined chunk by chunk), and the five small product classes
    x3_u32x4 A[9][3];                                                  // the current chunk's weights [tap][plane]; reloaded tap by tap with the next chunk's
    auto wslab = [&](int grp, int chunk) __attribute__((always_inline)) {
        return p.wx3 + (((int64_t)grp * nchunks + chunk) * 4 + wave) * (int64_t)SX_WSLAB + lane * 16;
    };
    int tile = blockIdx.x, par = 0;
    int e_n, e_oy0, e_ox0, e_grp;
    decode(tile, e_n, e_oy0, e_ox0, e_grp);
    {
        const unsigned char* w0 = wslab(e_grp, 0);
#pragma unroll
        for (int t = 0; t < 9; t++)
#pragma unroll
            for (int pl = 0; pl < 3; pl++) A[t][pl] = (SX_EXP & 8) ? (x3_u32x4){0u, 0u, 0u, 0u} : *(const x3_u32x4*)(w0 + (t * 3 + pl) * SX_FRAG);
        // the first chunk's weights are home before the loops: whatever order the loads above were issued in, the waits inside the chunk loop then count the
        // loop's own reloads only (a load still pending at the loop's entry makes every round wait for the count of the worst entry order)
        __builtin_amdgcn_s_waitcnt(0x0f70);                            // vmcnt(0)
#pragma unroll
        for (int t = 0; t < 9; t++)
#pragma unroll
            for (int pl = 0; pl < 3; pl++) asm volatile("" : "+v"(A[t][pl]));
    }
    unsigned long long st_mm = 0, st_bar = 0, st_ep = 0, st_t0 = 0, st_rounds = 0;      // (SX_EXP & 32: cycle totals of this wave)
    const float gain = p.gain;
    const float cl = clamp_bound(p.clamp);
    const float slope = act_slope(p.act, p.alpha);
    const int cs_ = (int)p.ys[1], rs_ = (int)p.ys[2], xs_ = (int)p.ys[3];
    asm volatile("s_barrier" ::: "memory");                           // barrier 0: the producers have made chunk 0
    for (int ti = 0, g = 0; ti < my_tiles; ti++, par ^= 1) {
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int k = 0; k < 16; k++) acc[a][k] = accs[a][k] = 0.f;
        // the next tile, for the weights that follow this tile's last chunk
        int nx_n = e_n, nx_oy0 = e_oy0, nx_ox0 = e_ox0, nx_grp = e_grp;
        if (ti + 1 < my_tiles) decode(tile + (int)gridDim.x, nx_n, nx_oy0, nx_ox0, nx_grp);
        for (int k = 0; k < nchunks; k++, g++) {
            const int wb = g & 1;
            if (SX_EXP & 32) st_t0 = __builtin_amdgcn_s_memtime();
            const unsigned char* wn = k + 1 < nchunks ? wslab(e_grp, k + 1) : wslab(nx_grp, 0);
            {
                const unsigned char* bb = planes + (size_t)wb * 3 * SX_PLB + (size_t)(half * SX_NPIX + 2 * orow * SX_PR + ocol) * 16;
                // tap (ky, kx) of accumulator a reads halo row 4 a + 2 orow + ky, halo column 2 ocol + kx = record (kx & 1) * 17 + ocol + (kx >> 1) of that row
                auto b_frag = [&](int t, int a, int pl) __attribute__((always_inline)) {
                    const int ky = t / 3, kx = t % 3;
                    return *(const x3_u32x4*)(bb + (size_t)pl * SX_PLB + (size_t)((4 * a + ky) * SX_PR + (kx & 1) * 17 + (kx >> 1)) * 16);
                };
                // B ring of two slots of one accumulator's three planes: slot (2 t + a) & 1 = a, requested six MFMAs (one accumulator's share of a tap) ahead
                x3_u32x4 B[2][3];
                f32x16 accp[2];                                        // this chunk's leading products
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int k = 0; k < 16; k++) accp[a][k] = 0.f;
#pragma unroll
                for (int pl = 0; pl < 3; pl++) B[0][pl] = b_frag(0, 0, pl);
#pragma unroll
                for (int t = 0; t < 9; t++) {
#pragma unroll
                    for (int a = 0; a < 2; a++) {
                        if (a == 0 || t + 1 < 9) {
#pragma unroll
                            for (int pl = 0; pl < 3; pl++) B[a ^ 1][pl] = a == 0 ? b_frag(t, 1, pl) : b_frag(t + 1, 0, pl);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int pr = 0; pr < 6; pr++) {
                            // The five small classes (at most 2^-8 of the leading product) meet in their own accumulator, where their roundings are 2^-8 of what
                            // they would be beside the leading sum.  The leading products of a chunk meet in a third one that starts at zero and joins the
                            // tile's sum by one VALU addition per chunk: the MFMA's accumulation is less exact than a rounded addition (measured: with everything
                            // in one accumulator 1.7 - 3.6 x the fp32 kernel's error against float64, leading and small apart 2.5 x at 128 channels; the bar is 2 x).
                            f32x16& dacc = pr == 5 ? accp[a] : accs[a];
                            if (!(SX_EXP & 1) || A[t][X3_PA[pr]][0] == 0x12345678u)
                                dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3_bf16x8, A[t][X3_PA[pr]]), __builtin_bit_cast(x3_bf16x8, B[a][X3_PB[pr]]), dacc, 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    // this tap's fragments have issued their last MFMA of the chunk: the next chunk's take their place
                    if (!(SX_EXP & 8)) {
#pragma unroll
                        for (int pl = 0; pl < 3; pl++) A[t][pl] = *(const x3_u32x4*)(wn + (t * 3 + pl) * SX_FRAG);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int k = 0; k < 16; k++) acc[a][k] += accp[a][k];
            }
            if (SX_EXP & 32) { const unsigned long long t1 = __builtin_amdgcn_s_memtime(); st_mm += t1 - st_t0; st_t0 = t1; }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // barrier g + 1: chunk g + 1 is complete; this chunk's planes are free
            if (SX_EXP & 32) { st_bar += __builtin_amdgcn_s_memtime() - st_t0; st_rounds++; }
        }

        // ---- epilogue: D column = lane & 31 = (output row & 1, column), D row = (k & 3) + 8 (k >> 2) + 4 half = cout of the wave's 32.  The stores go out from inline
        // asm through a buffer descriptor (conv2d_stem7x3.h): a store the compiler can see is counted by its vmcnt waits, and with loads and stores both pending it
        // waits for vmcnt(0) at the next chunk's first tap -- for the weight loads issued a moment before.
        if (SX_EXP & 32) st_t0 = __builtin_amdgcn_s_memtime();
        {
            int ll;                                                    // (the lane's coordinates made again: kept live across the chunk loop they cost registers it needs)
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ll));
            const int half = ll >> 5, orow = (ll >> 4) & 1, ocol = ll & 15;
            const int ox = e_ox0 + ocol;
            const int co0 = e_grp * SX_GROUP + 32 * wave + 4 * half;
            i32x4 yrsrc;
            {
                const uint64_t base = (uint64_t)(uintptr_t)(p.y + (int64_t)e_n * p.ys[0]);
                yrsrc[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)base);
                yrsrc[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32) & 0xffff);
                yrsrc[2] = 0x7ffffffc;
                yrsrc[3] = 0x00020000;
            }
            const float* bs = bias_s + par * SX_GROUP + 32 * wave + 4 * half;
#pragma unroll
            for (int kq = 0; kq < 4; kq++) {
                const f32x4 b4 = *(const f32x4*)(bs + 8 * kq);
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    const int oy = e_oy0 + 2 * a + orow;
                    const bool ok = oy < p.OH && ox < p.OW;
                    const unsigned o0 = (unsigned)((co0 + 8 * kq) * cs_ + oy * rs_ + ox * xs_) * 4u;       // (bytes inside one image of y: below 2^31, checked by the launcher)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        float v = (acc[a][4 * kq + j] + accs[a][4 * kq + j]) + b4[j];
                        v = v > 0.f ? v : v * slope;
                        v = clamp_tail(v * gain, cl);
                        const unsigned off = (ok && co0 + 8 * kq + j < p.Cout && (!(SX_EXP & 16) || v == 12345.678f)) ? o0 + (unsigned)(j * cs_) * 4u : 0x80000000u;      // out of range: dropped
                        asm volatile("buffer_store_dword %0, %1, %2, 0 offen" :: "v"(v), "v"(off), "s"(yrsrc) : "memory");
                    }
                }
            }
        }
        if (SX_EXP & 32) st_ep += __builtin_amdgcn_s_memtime() - st_t0;
        tile += gridDim.x;
        e_n = nx_n; e_oy0 = nx_oy0; e_ox0 = nx_ox0; e_grp = nx_grp;
    }
    if (SX_EXP & 32) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (blockIdx.x == 0 && lane == 0) {
            unsigned long long* o = (unsigned long long*)p.y + wave * 4;
            o[0] = st_mm; o[1] = st_bar; o[2] = st_ep; o[3] = st_rounds;
        }
    }
}

// The weight stream of this kernel for x3_pack_kernel: [cout group][chunk][m-block 4][tap 9][plane 3][k-half 2][32 couts][8 channels], zero-padded to whole groups
struct X3PackS2 {
    static constexpr int PLANE = 512;
    static int cout_padded(int Cout) { return (Cout + SX_GROUP - 1) / SX_GROUP * SX_GROUP; }
    static __device__ __forceinline__ int64_t dst(int co, int tap, int ci, int nchunks) {
        const int grp = co >> 7, mb = (co >> 5) & 3, m = co & 31, chunk = ci >> 4, kh = (ci >> 3) & 1, j = ci & 7;
        return ((((((int64_t)grp * nchunks + chunk) * 4 + mb) * 9 + tap) * 3) * 2 + kh) * 256 + m * 8 + j;
    }
};

inline int64_t s2x3_packed_bytes(int Cout, int Cin) { return (int64_t)((Cout + SX_GROUP - 1) / SX_GROUP) * (Cin / SX_KC) * 4 * SX_WSLAB; }

inline bool s2x3_serves(const S2x3Params& p) {
    return p.H >= 3 && p.W >= 3 && p.Cin % SX_KC == 0 && p.Cin >= 2 * SX_KC && (((uintptr_t)p.x) & 3) == 0 &&
           ((int64_t)p.Cin * p.H * p.W + 4) * 4 < 0x7fffffffLL;                       // one image through a 32-bit buffer descriptor
}

inline int launch_s2x3(S2x3Params p, hipStream_t s) {
    if (!s2x3_serves(p) || !p.wx3) return PG_ERR_UNSUPPORTED;
    p.OH = (p.H - 3) / 2 + 1; p.OW = (p.W - 3) / 2 + 1;
    p.tilesX = (p.OW + SX_TW - 1) / SX_TW;
    p.tilesY = (p.OH + SX_TH - 1) / SX_TH;
    p.groups = (p.Cout + SX_GROUP - 1) / SX_GROUP;
    const int64_t tiles = (int64_t)p.N * p.tilesX * p.tilesY * p.groups;
    if (tiles > 0x7fffffffLL) return PG_ERR_TOO_LARGE;
    if (((int64_t)(p.groups * SX_GROUP) * p.ys[1] + (int64_t)p.OH * p.ys[2] + (int64_t)p.OW * p.ys[3]) * 4 >= 0x7fffffffLL) return PG_ERR_UNSUPPORTED;      // 32-bit byte offsets inside one image of y
    if (p.ys[1] < 0 || p.ys[2] < 0 || p.ys[3] < 0) return PG_ERR_UNSUPPORTED;
    p.total_tiles = (int)tiles;
    const int64_t blocks = tiles < (int64_t)num_cu() ? tiles : (int64_t)num_cu();
    static PerDeviceOnce once;
    const hipError_t e = once.run([] { return hipFuncSetAttribute((const void*)conv2d_s2x3, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(conv2d_s2x3, dim3((unsigned)blocks), dim3(512), SX_LDS, s, p);
    return launch_status();
}

}  // namespace pgconv
