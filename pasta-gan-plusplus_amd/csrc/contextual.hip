// The contextual loss (training/contextual_loss.py, torch_utils/ops/contextual_ops.py) on gfx950: the per-sample P x P affinity between all feature
// positions of two images, streamed -- no P x P element is ever written to memory.  float32.  For one sample, x, y = [C, P] features, h the bandwidth:
//   mu_p = mean_c y[c,p];  x' = x - mu, y' = y - mu;  xn_p = x'_p / (|x'_p| + eps), yn likewise            (pg_cx_prepare, eps = 2.220446049250313e-16)
//   d_ij = 1 - xn_i . yn_j;  m_i = min_j d_ij (lowest j on ties: jmin_i);  e_i = m_i + 1e-3
//   w_ij = exp((1 - d_ij / e_i) / h);  S_i = sum_j w_ij;  a_i = max_j w_ij / S_i
//   CX = (1/P) sum_i a_i;  loss = -log CX                                                                   (pg_cx_forward)
// w falls strictly with d for e > 0, so the arg-max of A_i. IS jmin_i and d at it IS m_i: the second sweep keeps no arg-max of its own, and a_i is
// exp((1 - m_i / e_i) / h) / S_i, evaluated by the expression that made the w of the sweep (the same bits).
// Backward (pg_cx_backward), with g_i = -gout / (P CX), D_i = sum_j w_ij d_ij / S_i, V_i = sum_j (w_ij / S_i) yn_j:
//   dxn_i = (g a / (h e)) (yn_jmin - V_i) - (g a (m - D) / (h e^2)) yn_jmin
// At a well-matched row A_i. is nearly one-hot and both differences cancel to ~ 1e-5 of their terms, which float32 cannot afford.  So the sums leave
// jmin out: the forward keeps S'_i = sum_{j != jmin} w_ij (S = S' + w_jmin) and T'_i = sum_j w_ij (d_ij - m_i), the backward accumulates
// U'_i = sum_{j != jmin} w_ij yn_j, and  yn_jmin - V = (S' yn_jmin - U') / S,  m - D = -T' / S  hold without a cancellation.
// pg_cx_prepare_backward then maps dxn to dx (y and mu are constants):  dx_p = (dxn_p - xn_p (xn_p . dxn_p) (r + eps) / r) / (r + eps), r = |x'_p|,
// and a zero row where r == 0.
//
// Layout: pg_cx_prepare writes xn / yn position-major, [sample][P][Cp] with Cp = C rounded up to 32 and the padding zero, so that both GEMM operands are
// K-contiguous (its reductions over C run in double).  One workgroup (4 waves) owns 64 rows i of one sample and sweeps all of yn in tiles of 128
// columns; K runs in chunks of 32 through LDS on v_mfma_f32_32x32x2_f32 (exact float32 products, one chain per chunk, the chunk sums added in double;
// wave w owns columns 32 w .. 32 w + 31 of the tile and both 32-row halves).  Row statistics stay in the MFMA C layout per lane over the whole sweep
// and are folded across lanes and waves once per sweep, in a fixed order: no atomics, bit-identical run to run.  The backward's second GEMM takes the
// weight tile from the C layout through LDS as its A operand and yn straight from memory as B; wave w owns the 32-channel tiles w, w + 4, ... of a
// slice of up to 512 channels (128 accumulators per lane); wider features run one slice per grid.z, recomputing d.
// Every offset is 64-bit.  Every element of every output is written.  Nothing is read to the host.
#include "pg_common.h"
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int BM = 64;                   // rows i per workgroup
constexpr int BN = 128;                  // columns j per tile
constexpr int KC = 32;                   // channels per LDS chunk == the channel padding (PG_CX_CHANNEL_PAD)
constexpr int LDK = KC + 2;              // LDS row stride of the operand chunks: 34 i + k + (lane >> 5) hits 64 distinct banks
constexpr int LDW = BN + 2;              // LDS row stride of the weight tile, same argument
constexpr float kEps = 2.220446049250313e-16f;
constexpr float kMinOffset = 1e-3f;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ---------------------------------------------------------------- prepare: NCHW -> centred, normalised, position-major
// grid (ceil(P / 256), S + N): block row q < S is sample q of x, q >= S sample q - S of y.  One lane = one position.
__global__ __launch_bounds__(kThreads) void cx_prepare(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ xn,
                                                       float* __restrict__ yn, float* __restrict__ rx, int S, int N, int C, int Cp, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int q = blockIdx.y;
    const bool isx = q < S;
    const int sy = isx ? q % N : q - S;
    const float* yb = y + (int64_t)sy * C * P + p;
    const float* src = isx ? x + (int64_t)q * C * P + p : yb;
    float* dst = (isx ? xn + (int64_t)q * P * Cp : yn + (int64_t)sy * P * Cp) + p * Cp;
    // the two reductions over C in double: the mean and the norm are then correctly rounded float32 values, and a row's d carries no common error of
    // ~ 1e-7 for 1 / (h e) to amplify
    double sum = 0.0;
    for (int c = 0; c < C; c++) sum += (double)yb[(int64_t)c * P];
    const float mu = (float)(sum / (double)C);
    double ss = 0.0;
    for (int c = 0; c < C; c++) {
        const double v = (double)(src[(int64_t)c * P] - mu);
        ss += v * v;
    }
    const float r = (float)sqrt(ss);
    const float den = r + kEps;
    for (int c = 0; c < Cp; c += 4) {
        f32x4 o;
        o.x = c + 0 < C ? (src[(int64_t)(c + 0) * P] - mu) / den : 0.f;
        o.y = c + 1 < C ? (src[(int64_t)(c + 1) * P] - mu) / den : 0.f;
        o.z = c + 2 < C ? (src[(int64_t)(c + 2) * P] - mu) / den : 0.f;
        o.w = c + 3 < C ? (src[(int64_t)(c + 3) * P] - mu) / den : 0.f;
        *reinterpret_cast<f32x4*>(dst + c) = o;
    }
    if (isx) rx[(int64_t)q * P + p] = r;
}

// grid (ceil(P / 256), S).  dx[s][c][p] from dxn / xn [s][p][Cp] and r = rx[s][p]
__global__ __launch_bounds__(kThreads) void cx_prepare_bwd(const float* __restrict__ dxn, const float* __restrict__ xn, const float* __restrict__ rx,
                                                           float* __restrict__ dx, int C, int Cp, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int s = blockIdx.y;
    const float* g = dxn + ((int64_t)s * P + p) * Cp;
    const float* u = xn + ((int64_t)s * P + p) * Cp;
    float* o = dx + (int64_t)s * C * P + p;
    const float r = rx[(int64_t)s * P + p];
    if (!(r > 0.f) && r == r) {                                       // x' == 0: the normalisation is constant there (a NaN norm takes the other branch)
        for (int c = 0; c < C; c++) o[(int64_t)c * P] = 0.f;
        return;
    }
    float dot = 0.f;
    for (int c = 0; c < Cp; c += 4) {
        const f32x4 a = ld4(g + c), b = ld4(u + c);
        dot += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
    }
    const float den = r + kEps;
    const float k = dot * (den / r);
    for (int c = 0; c < Cp; c += 4) {
        const f32x4 a = ld4(g + c), b = ld4(u + c);
        if (c + 0 < C) o[(int64_t)(c + 0) * P] = (a.x - b.x * k) / den;
        if (c + 1 < C) o[(int64_t)(c + 1) * P] = (a.y - b.y * k) / den;
        if (c + 2 < C) o[(int64_t)(c + 2) * P] = (a.z - b.z * k) / den;
        if (c + 3 < C) o[(int64_t)(c + 3) * P] = (a.w - b.w * k) / den;
    }
}

// ---------------------------------------------------------------- one 64 x 128 tile of xn . yn^T
struct Stage {
    f32x4 xv[2], yv[4];
};

// lane t moves channels 4 (t & 7) .. + 3 of rows (t >> 3) + 32 u; rows past P read as zeros
__device__ __forceinline__ void load_chunk(Stage& st, const float* __restrict__ xs, const float* __restrict__ ys, int64_t i0, int64_t j0, int64_t P, int Cp,
                                           int kc) {
    const int k4 = (threadIdx.x & 7) * 4, r = threadIdx.x >> 3;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int64_t row = i0 + r + 32 * u;
        st.xv[u] = row < P ? ld4(xs + row * Cp + kc + k4) : z;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t row = j0 + r + 32 * u;
        st.yv[u] = row < P ? ld4(ys + row * Cp + kc + k4) : z;
    }
}

__device__ __forceinline__ void store_chunk(const Stage& st, float* Xs, float* Ys) {
    const int k4 = (threadIdx.x & 7) * 4, r = threadIdx.x >> 3;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        f32x2* d = reinterpret_cast<f32x2*>(Xs + (r + 32 * u) * LDK + k4);
        d[0] = f32x2{st.xv[u].x, st.xv[u].y};
        d[1] = f32x2{st.xv[u].z, st.xv[u].w};
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        f32x2* d = reinterpret_cast<f32x2*>(Ys + (r + 32 * u) * LDK + k4);
        d[0] = f32x2{st.yv[u].x, st.yv[u].y};
        d[1] = f32x2{st.yv[u].z, st.yv[u].w};
    }
}

// acc[rt][k] = d = 1 - sum_c xn[i0 + row][c] yn[j0 + 32 wave + (lane & 31)][c], row = 32 rt + (k & 3) + 8 (k >> 2) + 4 (lane >> 5).  Called by all 256
// lanes.  Each chunk of 32 channels is an exact-float32 MFMA chain of its own (partial sums of ~ 1/16 of the whole, so its rounding is ~ 1e-8); the chunk
// sums are added in double and d is rounded once: a single float32 chain over C = 512 wanders by ~ 8e-7, which 1 / (h e) ~ 600 at a well-matched row turns
// into 5e-4 of w and, through the cancellation in yn_jmin - V, into 2e-3 of the gradient.
__device__ __forceinline__ void dist_tile(f32x16 (&acc)[2], const float* __restrict__ xs, const float* __restrict__ ys, int64_t i0, int64_t j0, int64_t P,
                                         int Cp, float* Xs, float* Ys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    double tot[2][16];
#pragma unroll
    for (int k = 0; k < 16; k++) tot[0][k] = tot[1][k] = 0.0;
    Stage st;
    load_chunk(st, xs, ys, i0, j0, P, Cp, 0);
    const float* pa0 = Xs + l31 * LDK + half;
    const float* pa1 = Xs + (32 + l31) * LDK + half;
    const float* pb = Ys + (wave * 32 + l31) * LDK + half;
    for (int kc = 0; kc < Cp; kc += KC) {
        __syncthreads();                                              // every wave is done with the previous chunk (and the caller's use of LDS)
        store_chunk(st, Xs, Ys);
        __syncthreads();
        if (kc + KC < Cp) load_chunk(st, xs, ys, i0, j0, P, Cp, kc + KC);
#pragma unroll
        for (int k = 0; k < 16; k++) acc[0][k] = acc[1][k] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            const float b = pb[kk];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa0[kk], b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa1[kk], b, acc[1], 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            tot[0][k] += (double)acc[0][k];
            tot[1][k] += (double)acc[1][k];
        }
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        acc[0][k] = (float)(1.0 - tot[0][k]);
        acc[1][k] = (float)(1.0 - tot[1][k]);
    }
}

__device__ __forceinline__ int slot_row(int rt, int k, int half) { return 32 * rt + (k & 3) + 8 * (k >> 2) + 4 * half; }

__device__ __forceinline__ float weight_of(float d, float inv_e, float inv_h) { return expf((1.f - d * inv_e) * inv_h); }

// ---------------------------------------------------------------- forward: two sweeps
// grid (ceil(P / 64), S)
__global__ __launch_bounds__(kThreads) void cx_forward(const float* __restrict__ xn, const float* __restrict__ yn, float* __restrict__ m_out,
                                                       int* __restrict__ j_out, float* __restrict__ s_out, float* __restrict__ t_out,
                                                       float* __restrict__ a_out, int N, int Cp, int64_t P, float inv_h) {
    __shared__ float Xs[BM * LDK], Ys[BN * LDK];
    __shared__ float red_a[4][BM], red_b[4][BM];
    __shared__ int red_j[4][BM];
    __shared__ float row_m[BM];
    __shared__ int row_jmin[BM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int s = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * BM;
    const float* xs = xn + (int64_t)s * P * Cp;
    const float* ys = yn + (int64_t)(s % N) * P * Cp;
    f32x16 acc[2];

    // sweep 1: the row minimum of d and where it is
    {
        float mn[2][16];
        int jm[2][16];
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int k = 0; k < 16; k++) { mn[rt][k] = INFINITY; jm[rt][k] = 0; }
        for (int64_t j0 = 0; j0 < P; j0 += BN) {
            dist_tile(acc, xs, ys, i0, j0, P, Cp, Xs, Ys);
            const int64_t j = j0 + wave * 32 + l31;
            if (j < P) {
#pragma unroll
                for (int rt = 0; rt < 2; rt++)
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const float d = acc[rt][k];
                        if (d < mn[rt][k]) { mn[rt][k] = d; jm[rt][k] = (int)j; }      // j rises: the first of equal values stays
                    }
            }
        }
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int k = 0; k < 16; k++) {
                float v = mn[rt][k];
                int jv = jm[rt][k];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(v, o, 64);
                    const int oj = __shfl_xor(jv, o, 64);
                    if (ov < v || (ov == v && oj < jv)) { v = ov; jv = oj; }
                }
                if (l31 == 0) {
                    const int row = slot_row(rt, k, half);
                    red_a[wave][row] = v;
                    red_j[wave][row] = jv;
                }
            }
        __syncthreads();
        if (threadIdx.x < BM) {
            float v = red_a[0][threadIdx.x];
            int jv = red_j[0][threadIdx.x];
            for (int w = 1; w < 4; w++) {
                const float ov = red_a[w][threadIdx.x];
                const int oj = red_j[w][threadIdx.x];
                if (ov < v || (ov == v && oj < jv)) { v = ov; jv = oj; }
            }
            row_m[threadIdx.x] = v;
            row_jmin[threadIdx.x] = jv;
            const int64_t i = i0 + threadIdx.x;
            if (i < P) {
                m_out[(int64_t)s * P + i] = v;
                j_out[(int64_t)s * P + i] = jv;
            }
        }
        __syncthreads();
    }

    // sweep 2: S' = the sum of w over j != jmin, T' = sum w (d - m) (its term at jmin is an exact zero)
    float inv_e[2][16], sw[2][16], tw[2][16];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int k = 0; k < 16; k++) {
            inv_e[rt][k] = 1.f / (row_m[slot_row(rt, k, half)] + kMinOffset);
            sw[rt][k] = tw[rt][k] = 0.f;
        }
    for (int64_t j0 = 0; j0 < P; j0 += BN) {
        dist_tile(acc, xs, ys, i0, j0, P, Cp, Xs, Ys);
        const int64_t j = j0 + wave * 32 + l31;
        if (j < P) {
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int row = slot_row(rt, k, half);
                    const float d = acc[rt][k];
                    const float w = weight_of(d, inv_e[rt][k], inv_h);
                    sw[rt][k] += (int)j == row_jmin[row] ? 0.f : w;
                    tw[rt][k] += w * (d - row_m[row]);
                }
        }
    }
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int k = 0; k < 16; k++) {
            float a = sw[rt][k], b = tw[rt][k];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                a += __shfl_xor(a, o, 64);
                b += __shfl_xor(b, o, 64);
            }
            if (l31 == 0) {
                const int row = slot_row(rt, k, half);
                red_a[wave][row] = a;
                red_b[wave][row] = b;
            }
        }
    __syncthreads();
    if (threadIdx.x < BM) {
        const int64_t i = i0 + threadIdx.x;
        if (i < P) {
            const int r = threadIdx.x;
            const float others = (red_a[0][r] + red_a[1][r]) + (red_a[2][r] + red_a[3][r]);
            const float tsum = (red_b[0][r] + red_b[1][r]) + (red_b[2][r] + red_b[3][r]);
            const float m = row_m[r];
            const float wmax = weight_of(m, 1.f / (m + kMinOffset), inv_h);
            s_out[(int64_t)s * P + i] = others;
            t_out[(int64_t)s * P + i] = tsum;
            a_out[(int64_t)s * P + i] = wmax / (others + wmax);
        }
    }
}

// one block per sample: CX = mean_i a_i in double, in a fixed order; loss = -log CX
__global__ __launch_bounds__(kThreads) void cx_finish(const float* __restrict__ a, float* __restrict__ cx, float* __restrict__ loss, int64_t P) {
    __shared__ double s_acc[kThreads];
    const float* p = a + (int64_t)blockIdx.x * P;
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < P; i += kThreads) v += (double)p[i];
    s_acc[threadIdx.x] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double c = s_acc[0] / (double)P;
        cx[blockIdx.x] = (float)c;
        loss[blockIdx.x] = (float)-log(c);
    }
}

// ---------------------------------------------------------------- backward: one sweep, two GEMMs
// grid (ceil(P / 64), S, channel slices of NT * 128).  Wave w owns the 32-channel tiles slice + 32 (4 t + w), t < NT.
template <int NT>
__global__ __launch_bounds__(kThreads) void cx_backward(const float* __restrict__ xn, const float* __restrict__ yn, const float* __restrict__ m_in,
                                                        const int* __restrict__ j_in, const float* __restrict__ s_in, const float* __restrict__ t_in,
                                                        const float* __restrict__ a_in, const float* __restrict__ cx, const float* __restrict__ gout,
                                                        float* __restrict__ dxn, int N, int Cp, int64_t P, float inv_h) {
    __shared__ float Xs[BM * LDK], Ys[BN * LDK];
    __shared__ float Ws[BM * LDW];
    __shared__ float row_inv_e[BM], row_c1[BM], row_c2[BM];
    __shared__ int row_j[BM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int s = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * BM;
    const int cslice = blockIdx.z * (NT * 128);
    const float* xs = xn + (int64_t)s * P * Cp;
    const float* ys = yn + (int64_t)(s % N) * P * Cp;

    if (threadIdx.x < BM) {
        const int64_t i = i0 + threadIdx.x;
        float ie = 1.f, c1 = 0.f, c2 = 0.f;
        int jm = 0;
        if (i < P) {
            const int64_t o = (int64_t)s * P + i;
            const float m = m_in[o], others = s_in[o], ai = a_in[o];
            ie = 1.f / (m + kMinOffset);
            const float ssum = others + weight_of(m, ie, inv_h);      // S, by the forward's own expression
            const float g = -gout[s] / ((float)P * cx[s]);
            const float alpha = g * ai * inv_h * ie;
            const float beta = -g * ai * (t_in[o] / ssum) * inv_h * ie * ie;      // m - D = -T' / S
            c1 = alpha * (others / ssum) - beta;                      // yn_jmin - V = (S' yn_jmin - U') / S
            c2 = -alpha / ssum;
            jm = j_in[o];
        }
        row_inv_e[threadIdx.x] = ie;
        row_c1[threadIdx.x] = c1;
        row_c2[threadIdx.x] = c2;
        row_j[threadIdx.x] = jm;
    }
    __syncthreads();
    float inv_e[2][16];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int k = 0; k < 16; k++) inv_e[rt][k] = row_inv_e[slot_row(rt, k, half)];

    f32x16 vacc[NT][2];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int k = 0; k < 16; k++) vacc[t][0][k] = vacc[t][1][k] = 0.f;
    f32x16 acc[2];
    const float* wa0 = Ws + l31 * LDW + half;
    const float* wa1 = Ws + (32 + l31) * LDW + half;

    for (int64_t j0 = 0; j0 < P; j0 += BN) {
        dist_tile(acc, xs, ys, i0, j0, P, Cp, Xs, Ys);
        const int64_t jc = j0 + wave * 32 + l31;
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int row = slot_row(rt, k, half);
                Ws[row * LDW + wave * 32 + l31] = jc < P && (int)jc != row_j[row] ? weight_of(acc[rt][k], inv_e[rt][k], inv_h) : 0.f;
            }
        __syncthreads();                                              // (the next dist_tile's first barrier separates these reads from the next tile's writes)
#pragma unroll 4
        for (int kk = 0; kk < BN; kk += 2) {
            const int64_t j = j0 + kk + half;
            const float a0 = wa0[kk], a1 = wa1[kk];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const int c0 = cslice + 32 * (4 * t + wave);
                if (c0 < Cp) {
                    const float b = j < P ? ys[j * Cp + c0 + l31] : 0.f;
                    vacc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, vacc[t][0], 0, 0, 0);
                    vacc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, vacc[t][1], 0, 0, 0);
                }
            }
        }
    }

#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int c0 = cslice + 32 * (4 * t + wave);
        if (c0 >= Cp) continue;
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int row = slot_row(rt, k, half);
                const int64_t i = i0 + row;
                if (i < P) {
                    const float yj = ys[(int64_t)row_j[row] * Cp + c0 + l31];
                    dxn[((int64_t)s * P + i) * Cp + c0 + l31] = row_c1[row] * yj + row_c2[row] * vacc[t][rt][k];
                }
            }
    }
}

inline int padded(int c) { return (c + KC - 1) / KC * KC; }

inline int shape_status(int S, int N, int C, int64_t P) {
    if (S < 1 || N < 1 || C < 1 || P < 1 || S % N != 0) return PG_ERR_INVALID_ARG;
    if (S / N > PG_CX_MAX_GROUPS) return PG_ERR_UNSUPPORTED;
    if (C > INT32_MAX - KC || P > INT32_MAX - BN || (int64_t)S + N > 65535) return PG_ERR_TOO_LARGE;       // jmin is 32-bit; samples ride on grid.y
    if ((int64_t)S + N > (INT64_MAX / 8) / P / padded(C)) return PG_ERR_TOO_LARGE;
    return PG_OK;
}

}  // namespace

PG_EXPORT int pg_contextual_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_cx_padded_channels(int channels) { return channels < 1 || channels > INT32_MAX - KC ? 0 : padded(channels); }

PG_EXPORT int pg_cx_prepare(const float* x, const float* y, float* xn, float* yn, float* rx, int samples, int n, int channels, int64_t positions,
                            void* stream) {
    if (!x || !y || !xn || !yn || !rx) return PG_ERR_INVALID_ARG;
    const int st = shape_status(samples, n, channels, positions);
    if (st != PG_OK) return st;
    if (!pg::aligned16(xn) || !pg::aligned16(yn)) return PG_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((positions + kThreads - 1) / kThreads), (unsigned)(samples + n));
    hipLaunchKernelGGL(cx_prepare, grid, dim3(kThreads), 0, (hipStream_t)stream, x, y, xn, yn, rx, samples, n, channels, padded(channels), positions);
    return pg::launch_status();
}

PG_EXPORT int pg_cx_prepare_backward(const float* dxn, const float* xn, const float* rx, float* dx, int samples, int channels, int64_t positions,
                                     void* stream) {
    if (!dxn || !xn || !rx || !dx) return PG_ERR_INVALID_ARG;
    const int st = shape_status(samples, samples, channels, positions);
    if (st != PG_OK) return st;
    if (!pg::aligned16(xn) || !pg::aligned16(dxn)) return PG_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((positions + kThreads - 1) / kThreads), (unsigned)samples);
    hipLaunchKernelGGL(cx_prepare_bwd, grid, dim3(kThreads), 0, (hipStream_t)stream, dxn, xn, rx, dx, channels, padded(channels), positions);
    return pg::launch_status();
}

PG_EXPORT int pg_cx_forward(const float* xn, const float* yn, float* row_min, int* row_argmin, float* row_others, float* row_wd, float* row_a, float* cx,
                            float* loss, int samples, int n, int channels, int64_t positions, double h, void* stream) {
    if (!xn || !yn || !row_min || !row_argmin || !row_others || !row_wd || !row_a || !cx || !loss || !(h > 0)) return PG_ERR_INVALID_ARG;
    const int st = shape_status(samples, n, channels, positions);
    if (st != PG_OK) return st;
    if (!pg::aligned16(xn) || !pg::aligned16(yn)) return PG_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((positions + BM - 1) / BM), (unsigned)samples);
    hipLaunchKernelGGL(cx_forward, grid, dim3(kThreads), 0, (hipStream_t)stream, xn, yn, row_min, row_argmin, row_others, row_wd, row_a, n, padded(channels),
                       positions, (float)(1.0 / h));
    const int ls = pg::launch_status();
    if (ls != PG_OK) return ls;
    hipLaunchKernelGGL(cx_finish, dim3((unsigned)samples), dim3(kThreads), 0, (hipStream_t)stream, (const float*)row_a, cx, loss, positions);
    return pg::launch_status();
}

PG_EXPORT int pg_cx_backward(const float* xn, const float* yn, const float* row_min, const int* row_argmin, const float* row_others, const float* row_wd,
                             const float* row_a, const float* cx, const float* gout, float* dxn, int samples, int n, int channels, int64_t positions,
                             double h, void* stream) {
    if (!xn || !yn || !row_min || !row_argmin || !row_others || !row_wd || !row_a || !cx || !gout || !dxn || !(h > 0)) return PG_ERR_INVALID_ARG;
    const int st = shape_status(samples, n, channels, positions);
    if (st != PG_OK) return st;
    if (!pg::aligned16(xn) || !pg::aligned16(yn)) return PG_ERR_UNSUPPORTED;
    const int cp = padded(channels), tiles = cp / 32;
    const int nt = tiles >= 16 ? 4 : (tiles + 3) / 4;                 // 32-channel tiles per wave: 1..4
    const int slices = (tiles + 4 * nt - 1) / (4 * nt);
    if (slices > 65535) return PG_ERR_TOO_LARGE;
    const dim3 grid((unsigned)((positions + BM - 1) / BM), (unsigned)samples, (unsigned)slices);
    const float inv_h = (float)(1.0 / h);
#define PG_CX_BWD(NT_)                                                                                                                                   \
    hipLaunchKernelGGL(cx_backward<NT_>, grid, dim3(kThreads), 0, (hipStream_t)stream, xn, yn, row_min, row_argmin, row_others, row_wd, row_a, cx, gout, dxn, n, \
                       cp, positions, inv_h)
    switch (nt) {
        case 1: PG_CX_BWD(1); break;
        case 2: PG_CX_BWD(2); break;
        case 3: PG_CX_BWD(3); break;
        default: PG_CX_BWD(4); break;
    }
#undef PG_CX_BWD
    return pg::launch_status();
}
