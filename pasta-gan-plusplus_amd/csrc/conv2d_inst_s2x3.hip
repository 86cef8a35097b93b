// The stride-2 3x3 convolution on the bf16 matrix pipe: instantiation + C ABI (own translation unit: see conv2d_kernel.h on build time).
#include "conv2d_s2x3.h"

/* conv2d(x [N, Cin, H, W], w [Cout, Cin, 3, 3], stride 2, padding 0) -> y [N, Cout, (H - 3) / 2 + 1, (W - 3) / 2 + 1] with the fused bias / activation / gain /
 * clamp of pg_conv2d_forward (networks.py:170-179 around conv2d_resample.py:119-122), in the three-term bf16 arithmetic of csrc/bf16x3.h (unguarded split: an
 * infinite operand yields NaN where the fp32 kernel yields +-inf): float32-class results (csrc/conv2d_s2x3.h).  `packed_x3` = pg_conv2d_s2x3_pack_weight of `packed` (= pg_conv2d_pack_weight of the OIHW 3x3 kernel),
 * pg_conv2d_s2x3_packed_size(Cout, Cin) BYTES, once per weight version.  Serves Cin % 16 == 0, Cin >= 32, H, W >= 3; x is read in whole 16-byte words: nothing
 * outside the 16-byte-aligned span that holds x is touched.  Fusion stages other than bias / act in {linear, relu, lrelu} / gain / clamp (a residual, a
 * modulation, SPADE, a second source, noise, statistics) are declined with PG_ERR_UNSUPPORTED before any launch: callers then use pg_conv2d_forward. */
PG_EXPORT int64_t pg_conv2d_s2x3_packed_size(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0 || Cin % 16 != 0) return 0;
    return pgconv::s2x3_packed_bytes(Cout, Cin);
}

PG_EXPORT int pg_conv2d_s2x3_pack_weight(const float* packed, void* packed_x3, int Cout, int Cin, void* stream) {
    if (!packed || !packed_x3 || Cout <= 0 || Cin <= 0 || (((uintptr_t)packed_x3) & 15) != 0) return PG_ERR_INVALID_ARG;
    if (Cin % 16 != 0) return PG_ERR_UNSUPPORTED;
    return pgconv::launch_x3_pack<pgconv::X3PackS2>(packed, packed_x3, Cout, Cin, (hipStream_t)stream);
}

PG_EXPORT int pg_conv2d_s2x3_forward(const float* x, const void* packed_x3, float* y, int N, int Cin, int H, int W, int Cout, const int64_t ystride[4],
                                     const pg_conv2d_fusion* fusion, void* stream) {
    if (!x || !packed_x3 || !y || !ystride || N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return PG_ERR_INVALID_ARG;
    if ((((uintptr_t)x) & 3) != 0 || (((uintptr_t)packed_x3) & 15) != 0) return PG_ERR_INVALID_ARG;
    pgconv::S2x3Params p;
    p.x = x; p.y = y; p.wx3 = (const unsigned char*)packed_x3; p.bias = nullptr;
    p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    for (int i = 0; i < 4; i++) p.ys[i] = ystride[i];
    p.act = PG_ACT_LINEAR; p.alpha = 0.f; p.gain = 1.f; p.clamp = -1.f;
    if (fusion) {
        const pg_conv2d_fusion& f = *fusion;
        if (f.in_scale || f.in_bias || (f.in_act != 0 && f.in_act != PG_ACT_LINEAR) || f.in_clamp >= 0.f || (f.in_gain != 0.f && f.in_gain != 1.f) || f.out_scale || f.noise || f.residual ||
            f.spade_x || f.spade_mean || f.spade_rstd || f.x2 || f.stats_partial)
            return PG_ERR_UNSUPPORTED;
        const int act = f.act == 0 ? PG_ACT_LINEAR : f.act;
        if (act != PG_ACT_LINEAR && act != PG_ACT_RELU && act != PG_ACT_LRELU) return PG_ERR_UNSUPPORTED;
        p.bias = f.bias; p.act = act; p.alpha = f.alpha; p.gain = f.gain == 0.f ? 1.f : f.gain; p.clamp = f.clamp;
    }
    return pgconv::launch_s2x3(p, (hipStream_t)stream);
}
