/*
 * pasta_gan_ops.h -- C ABI of the MI355X (gfx950) kernels behind PASTA-GAN++'s
 * generator-synthesis operator API.
 *
 * These shared libraries export the symbols below (one per reference "plugin", plus the loader's patch routing, the augment pipe, the try-on staging,
 * the training loop's data fetch and the reconstruction metrics):
 *   bias_act_plugin.so      pg_bias_act
 *   upfirdn2d_plugin.so     pg_upfirdn2d, pg_upfirdn2d_bias_act, pg_upfirdn2d_with_odd_samples
 *   conv2d_plugin.so        fp32: pg_conv2d_{packed_size,pack_weight,forward,splitk_plan,forward_splitk}, pg_conv2d_winograd_*,
 *                           pg_conv2d_up2_{forward,splitk_plan,forward_splitk}, pg_conv1x1_small, pg_conv1x1_fold_{prep,heads}, pg_conv3x3_fold_head, pg_conv3x3_cin1, pg_conv2d_wgrad{_plan,}, pg_split3_bf16_cl;
 *                           16-bit: pg_conv2d16_{packed_size,pack_weight,pack_weight_grouped,forward,splitk_plan,forward_splitk,up2_fused,wgrad,wgrad_plan,wgrad_x3}, pg_adam_flat_{chunk,step},
 *                           pg_conv1x1_small16;  glue: pg_modconv_{dcoefs,w2,prep}, pg_instance_norm_stats, pg_spade_*
 *   patch_routing_plugin.so pg_warp_perspective_u8, pg_patch_compose_u8[_k], pg_patch_compose_ordered_u8[_k]
 *   augment_plugin.so       pg_augment_warp, pg_augment_warp_adjoint, pg_augment_color, pg_augment_late
 *   tryon_plugin.so         pg_tryon_row_extent_u8, pg_tryon_inputs, pg_tryon_triptych_u8, pg_tryon_panels_u8
 *   train_fetch_plugin.so   pg_train_fetch
 *   tryon_front_plugin.so   pg_tryon_front_stats, pg_tryon_front_bit_rows, pg_tryon_front_compose
 *   vgg_loss_plugin.so      pg_maxpool2x2, pg_maxpool2x2_backward, pg_l1_pair_blocks, pg_l1_pair_sum, pg_l1_pair_grad
 *   image_metrics_plugin.so pg_image_pair_metrics_workspace, pg_image_pair_metrics_u8
 *   region_metrics_plugin.so pg_region_pair_metrics_workspace, pg_region_pair_metrics_u8, pg_label_confusion_u8
 *   contextual_plugin.so    pg_cx_padded_channels, pg_cx_prepare, pg_cx_prepare_backward, pg_cx_forward, pg_cx_backward
 * plus pg_<plugin>_abi_version() in each.  They are what the reference's L1
 * Python ops bind in place of its pybind plugins (see INTEGRATION.md for the
 * ctypes stub a maintainer adds to the reference tree).
 *
 * Conventions (all entry points)
 *   - plain pointers to DEVICE memory + sizes; no torch types; never throws.
 *   - asynchronous: work is enqueued on `stream` (a hipStream_t passed as void*;
 *     NULL = the null stream); no allocation, no synchronisation inside.
 *   - return 0 on success; a negative PG_ERR_* for rejected arguments (nothing
 *     was launched); a positive hipError_t if the launch itself failed.
 *   - strides are in ELEMENTS, not bytes.
 */
#ifndef PASTA_GAN_OPS_H
#define PASTA_GAN_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 22

enum pg_dtype { PG_F32 = 0, PG_F16 = 1, PG_BF16 = 2, PG_F64 = 3 };

enum pg_error {
    PG_OK = 0,
    PG_ERR_INVALID_ARG = -1,   /* NULL pointer, non-positive size, bad enum     */
    PG_ERR_UNSUPPORTED = -2,   /* valid request the kernels do not cover         */
    PG_ERR_TOO_LARGE = -3      /* index range exceeds the kernel's 32-bit maths  */
};

/* Activation indices: identical to the reference's cuda_idx (bias_act.py:23-33). */
enum pg_act {
    PG_ACT_LINEAR = 1, PG_ACT_RELU = 2, PG_ACT_LRELU = 3, PG_ACT_TANH = 4, PG_ACT_SIGMOID = 5,
    PG_ACT_ELU = 6, PG_ACT_SELU = 7, PG_ACT_SOFTPLUS = 8, PG_ACT_SWISH = 9
};

/* ------------------------------------------------------------------------
 * bias_act  -- replaces bias_act_plugin.bias_act (torch_utils/ops/bias_act.cpp:32-90,
 * kernel bias_act.cu:23-147).
 *
 *   grad == 0:  y = clamp(act(x + b[(i / stepB) % sizeB]) * gain)
 *   grad == 1:  x holds dy;          y = dy * act'(.) * gain, zeroed where |yref| >= clamp
 *   grad == 2:  x holds d_dx, `dy` the first-order upstream gradient; second derivative
 *   xref / yref: forward input / output as the activation's backward needs them
 *   (bias_act.py:23-33 column `ref`); NULL where the reference passes an empty tensor.
 *   All tensors share x's dense layout; `b` has sizeB contiguous elements of x's dtype.
 *   clamp < 0 disables clamping.
 */
int pg_bias_act(const void* x, const void* b, const void* xref, const void* yref, const void* dy, void* y,
                int dtype, int64_t sizeX, int sizeB, int64_t stepB,
                int grad, int act, float alpha, float gain, float clamp, void* stream);
int pg_bias_act_abi_version(void);

/* First-derivative form with the bias gradient gathered in the same pass (training route): dx as grad == 1 above (NULL: not stored),
 * db[c] = dx summed over every element of channel c, written in the tensors' dtype.  Replaces the pair "plugin call + dx.sum(...)" of
 * BiasActCuda.backward (torch_utils/ops/bias_act.py:176-186).  Covered: float32 / float16 / bfloat16; act linear, relu, lrelu (the
 * derivatives that need only yref); layouts [outer][sizeB][stepB] with stepB a multiple of 16 bytes, or stepB == 1 with sizeB / (16 bytes)
 * dividing 256.  `workspace`: at least pg_bias_act_grad_bias_workspace(...) bytes of device memory (0 = layout not covered); the sum is a
 * fixed-order fold of per-workgroup partials -- bit-identical from run to run.  PG_ERR_UNSUPPORTED: not covered / unaligned. */
int64_t pg_bias_act_grad_bias_workspace(int dtype, int64_t sizeX, int sizeB, int64_t stepB);
int pg_bias_act_grad_bias(const void* dy, const void* yref, void* dx, void* db, void* workspace, int64_t workspace_bytes,
                          int dtype, int64_t sizeX, int sizeB, int64_t stepB,
                          int act, float alpha, float gain, float clamp, void* stream);

/* ------------------------------------------------------------------------
 * upfirdn2d -- replaces upfirdn2d_plugin.upfirdn2d (torch_utils/ops/upfirdn2d.cpp:16-94,
 * kernels upfirdn2d.cu:29-200).
 *
 *   y[n,c,oy,ox] = gain * sum_{ky,kx} g[ky,kx] * xs[oy*downy + ky - pady0, ox*downx + kx - padx0]
 *   xs = x zero-stuffed by (upx, upy), zero outside; g = f flipped in both axes unless `flip`.
 *   outW = (inW*upx + padx0 + padx1 - fw + downx) / downx is computed by the CALLER
 *   (upfirdn2d.cpp:32-33) and passed in; x/y strides are (n, c, h, w) in elements, any layout;
 *   f is float32 [fh, fw] with its own strides.
 */
int pg_upfirdn2d(const void* x, const float* f, void* y, int dtype,
                 int N, int C, int inH, int inW, const int64_t xstride[4],
                 int fh, int fw, const int64_t fstride[2],
                 int outH, int outW, const int64_t ystride[4],
                 int upx, int upy, int downx, int downy, int padx0, int pady0,
                 int flip, float gain, void* stream);
/* Round 6 -- pg_upfirdn2d (no resampling) that also writes the odd rows and columns of its output as a dense tensor: y_odd[n, c, j, i] = y[n, c, 2 j + 1, 2 i + 1],
 * [N, C, (outH - 1) / 2, (outW - 1) / 2].  A ResBlock with down = 2 filters its input twice (conv2d_resample.py:119-122 with padding 2 in front of the strided 3x3
 * convolution, :107-110 with padding 1 and every second sample in front of the 1x1 skip convolution): the second result is exactly these samples of the first.
 * float32, dense NCHW, the tiled kernel's filter sizes; anything else PG_ERR_UNSUPPORTED (callers then make the two pg_upfirdn2d calls). */
int pg_upfirdn2d_with_odd_samples(const void* x, const float* f, void* y, float* y_odd, int dtype,
                                  int N, int C, int inH, int inW, const int64_t xstride[4],
                                  int fh, int fw, const int64_t fstride[2],
                                  int outH, int outW, const int64_t ystride[4],
                                  int padx0, int pady0, int flip, float gain, void* stream);
/* Which kernel the last launch of this library went to: 1 = the 16-byte blur kernel (upfirdn2d_blur4), 2 = a tiled specialisation, 3 = a channels-last kernel,
 * 4 = the generic kernel, 0 = none / declined.  For tests that assert a route; not synchronised with other host threads. */
int pg_upfirdn2d_last_route(void);
/* upfirdn2d followed, in the same pass, by the tail of a SynthesisLayer: v = fir(x) * gain + noise * noise_gain + bias[c];
 * y = clamp(act(v) * act_gain) with act in {linear, relu, lrelu}.  float32, dense NCHW, the filter sizes / factors of the
 * tiled kernel only (PG_ERR_UNSUPPORTED otherwise -- callers then run pg_upfirdn2d and pg_bias_act separately). */
typedef struct pg_fir_epilogue {
    const float* noise;         /* [outH, outW] (noise_batch_stride 0) or [N, outH, outW]; NULL = none */
    int64_t      noise_batch_stride;
    float        noise_gain;
    const float* bias;          /* [C]; NULL = none */
    int          act;           /* pg_act */
    float        alpha;
    float        act_gain;      /* 0 => 1 */
    float        clamp;         /* < 0 = off */
} pg_fir_epilogue;
int pg_upfirdn2d_bias_act(const void* x, const float* f, void* y, int dtype,
                          int N, int C, int inH, int inW, const int64_t xstride[4],
                          int fh, int fw, const int64_t fstride[2],
                          int outH, int outW, const int64_t ystride[4],
                          int upx, int upy, int downx, int downy, int padx0, int pady0,
                          int flip, float gain, const pg_fir_epilogue* epilogue, void* stream);
int pg_upfirdn2d_abi_version(void);

/* ------------------------------------------------------------------------
 * conv2d (new: the reference has no native conv; its arithmetic is cuDNN's behind
 * conv2d_gradfix.py:35-43 / conv2d_resample.py:29-54).  fp32 NCHW implicit GEMM on
 * v_mfma_f32_32x32x2_f32 with fused prologue/epilogue.
 *
 * Weight packing: OIHW [Cout, Cin, KH, KW] -> the kernel's [CinP][KH*KW][CoutP] layout
 * (CinP = Cin rounded up to 16, CoutP = Cout rounded up to 32, zero filled), scaled by
 * `scale` (the layers' runtime weight_gain, networks.py:171) and optionally flipped in
 * both spatial axes (flip_weight=False in conv2d_resample.py:34-35) or transposed
 * O<->I (the conv_transpose2d weight view, conv2d_resample.py:127).
 * pg_conv2d_packed_size returns the number of floats the packed buffer needs.
 */
int64_t pg_conv2d_packed_size(int Cout, int Cin, int KH, int KW);
int pg_conv2d_pack_weight(const float* w, float* packed, int Cout, int Cin, int KH, int KW,
                          float scale, int flip_hw, int transpose_oi, void* stream);

/* Optional fused stages of pg_conv2d_forward; every pointer may be NULL (= stage off). */
typedef struct pg_conv2d_fusion {
    /* prologue, applied to each in-image input element before the contraction
       (zero padding stays zero):  x' = clamp(in_act(x * in_scale[n,ci]) * in_gain); in_gain > 0, in_act in {linear, relu, lrelu} */
    const float* in_scale;      /* [N, Cin]  style modulation (networks.py:74)                  */
    const float* in_bias;       /* [Cin]     must be NULL: a pre-activation bias would turn the zero padding into act(b)
                                             (PG_ERR_UNSUPPORTED); none of the generator's SPADE convs has one          */
    int          in_act;        /* pg_act; 0 or PG_ACT_LINEAR = none                             */
    float        in_alpha;
    float        in_gain;       /* used only when in_act/in_bias/in_gain stage is on (0 => 1)    */
    float        in_clamp;      /* < 0 = off                                                     */
    /* epilogue:  v = acc * out_scale[n,co] + noise[...] * noise_gain + bias[co];
                  v = clamp(act(v) * gain);  y = v + residual * residual_gain                    */
    const float* out_scale;     /* [N, Cout] demodulation coefficients (networks.py:68,77)       */
    const float* noise;         /* [OH, OW] (noise_batch_stride = 0) or [N, OH, OW]              */
    int64_t      noise_batch_stride;
    float        noise_gain;
    const float* bias;          /* [Cout]                                                        */
    int          act;           /* pg_act                                                        */
    float        alpha;
    float        gain;          /* 0 => 1 */
    float        clamp;         /* < 0 = off */
    const float* residual;      /* same shape/strides as y: y += residual (ResBlock add, img.add_) */
    /* SPADE combine mode (all three set, Cout = 2*C packed as alternating blocks of 32 gamma rows / 32 beta rows of the
       same channels): y[n,c] = (spade_x[n,c] - spade_mean[n,c]) * spade_rstd[n,c] * (1 + gamma[n,c]) + beta[n,c]
       (Spade_Norm_Block, networks.py:1715-1722); y and spade_x are [N, C, OH, OW] with the strides passed for y;
       act / alpha / gain / clamp then apply to that result (the pre-activation of the Spade_Conv2dLayer consuming it,
       networks.py:1627-1633); out_scale / noise / bias / residual are ignored in this mode;
       the other epilogue stages are not applied. */
    const float* spade_x;
    const float* spade_mean;    /* [N, C] */
    const float* spade_rstd;    /* [N, C] */
    /* Second input (channel concatenation without the copy): input channels [cin_split, Cin) are read from x2
       ([N, Cin - cin_split, H, W], contiguous) instead of x ([N, cin_split, H, W]) -- the `torch.cat([x, feat], 1)` in
       front of merge_conv (networks.py:2179-2181).  cin_split must be a multiple of 16. */
    const float* x2;
    int          cin_split;
    /* Instance-norm statistics of the OUTPUT, gathered where it is produced (round 4): when set, every workgroup tile also writes the sum and M2
       (the sum of squared deviations from the tile's own mean; round 5, was the sum of squares) of its in-image outputs per output channel to stats_partial[((n * Cout + co) * T + t) * 2 + {0, 1}], T = the tile count of one
       image (pg_conv2d_winograd4_stats_tiles), t = the tile's index; pg_instance_norm_finish turns them into mean / rstd (fixed order: deterministic).
       The values are those written to y (after the epilogue).  Only PG_WINO_F4 / PG_WINO_F4X3 launches of pg_conv2d_winograd_forward with the plain tail (no in_scale, noise,
       residual, SPADE) gather them; every other launch with this field set is declined (PG_ERR_UNSUPPORTED).  The SPADE res-blocks normalise the
       output of such a convolution (networks.py:1896-1904, 1715-1723): the separate statistics pass over it (pg_instance_norm_stats) is what this removes. */
    float*       stats_partial;
} pg_conv2d_fusion;

/*
 * y[n, co, oy*osy + ooy, ox*osx + oox] (+)= sum_{ci,ky,kx} wp[ci][ky*KW+kx][co] * x'[n, ci, oy*stride + ky - pad_y, ox*stride + kx - pad_x]
 * for oy in [0, OH), ox in [0, OW).  (osy, osx, ooy, oox) = (1,1,0,0) for ordinary convs; a stride-2
 * transposed conv is issued as up to four such calls, one per output phase (see conv2d_gradfix.py of
 * this package).  x: [N, Cin, H, W] contiguous; y: strides given in elements.
 */
int pg_conv2d_forward(const float* x, const float* packed_w, float* y,
                      int N, int Cin, int H, int W, int Cout, int KH, int KW,
                      int stride, int pad_y, int pad_x, int OH, int OW,
                      const int64_t ystride[4], int out_step_y, int out_step_x, int out_off_y, int out_off_x,
                      const pg_conv2d_fusion* fusion, void* stream);

/*
 * Split-K form of pg_conv2d_forward for launches with too few output tiles to occupy the chip (the 8x8 .. 32x32 layers of the
 * style branch: a workgroup's K loop is then a serial chain of 512 channels).  `ksplit` workgroups per tile each reduce
 * Cin / ksplit channels into their own slice of `workspace` (ksplit * N * Cout * OH * OW floats, caller-provided: this library
 * never allocates), then one elementwise pass sums the slices in fixed order and applies the fused epilogue.
 * pg_conv2d_splitk_plan returns the ksplit this library would choose (1 = use pg_conv2d_forward); not for spade_x / x2 launches.
 */
int pg_conv2d_splitk_plan(int N, int Cin, int OH, int OW, int Cout, int KH, int KW, int stride);
/* Which kernel the last stride-1 1x1 launch of pg_conv2d_forward went to: 2 = the ring form of the streaming kernel, 1 = the streaming kernel,
 * 0 = the tiled kernel (csrc/conv2d_s1x1.h).  For tests that assert a route; not synchronised with other host threads. */
int pg_conv2d_last_1x1_route(void);
int pg_conv2d_forward_splitk(const float* x, const float* packed_w, float* y,
                             int N, int Cin, int H, int W, int Cout, int KH, int KW,
                             int stride, int pad_y, int pad_x, int OH, int OW,
                             const int64_t ystride[4], int out_step_y, int out_step_x, int out_off_y, int out_off_x,
                             const pg_conv2d_fusion* fusion, float* workspace, int ksplit, void* stream);

/*
 * Winograd forms of pg_conv2d_forward for KH = KW = 3, stride 1, out_step 1 (the bulk of the synthesis network): one entry set, `form` picks the kernel.
 * Weights are pre-transformed once per weight version (U = G g G^T per (ci, co)) by pg_conv2d_winograd_pack_weight -- same scale / flip_hw / transpose_oi
 * meaning as pg_conv2d_pack_weight -- into that form's operand stream of pg_conv2d_winograd_packed_size float32 units (CinP = Cin rounded up to 16,
 * CoutP64 = Cout rounded up to 64; padded rows and channels are zero).  A form outside the enum: PG_ERR_INVALID_ARG (packed_size: 0), nothing launched.
 *
 *   PG_WINO_F2    F(2x2, 3x3), csrc/conv2d_wino.h: 16 * CinP * CoutP64 floats, transformed in float32.  The same result as pg_conv2d_forward up to fp32
 *                 summation order (~2e-6 of the output scale) with 2.25x fewer multiplies.  Fusion: every stage of pg_conv2d_fusion except x2 and
 *                 stats_partial; SPADE mode uses the same 32/32 gamma/beta row interleave as pg_conv2d_forward.
 *   PG_WINO_F4    F(4x4, 3x3), one 12-wave workgroup per CU (round 3; csrc/conv2d_wino4.h): 2.25 multiplies per output instead of 4.  36 * CinP * CoutP64
 *                 floats, transformed in float64 and rounded once.  float32 error ~4x that of F(2x2): max-abs 3.7e-5 on the config-2 image against the
 *                 direct float32 network (tools/f43_error_probe.py).  Launches with the plain tail can gather stats_partial (below).
 *   PG_WINO_F4B   the same algorithm with TWO workgroups per CU (round 4; csrc/conv2d_wino4b.h, v_mfma_f32_16x16x4_f32, 64 couts x 16 tiles per workgroup):
 *                 the same 36 * CinP * CoutP64 values in its own stream order, bit-identical results.  SPADE combine mode expects gamma / beta rows packed as
 *                 ADJACENT cout pairs (row 2c = gamma of channel c, row 2c + 1 = beta), not as blocks of 32.  No stats_partial.
 *   PG_WINO_F4X3  the PG_WINO_F4 kernel with its transform-domain GEMM on the bf16 matrix pipe (round 6; csrc/conv2d_wino4.h, X3 form): every float32 operand
 *                 of that GEMM is the exact sum of three bf16 values (truncation split, 8 + 8 + 8 significand bits) and the product is evaluated as the six
 *                 largest of the nine plane products on v_mfma_f32_32x32x16_bf16 with float32 accumulation -- float32-class results (the three dropped
 *                 products are below 2^-24 of the product), at 6/16 of the fp32 MFMA's issue time.  The PG_WINO_F4 values split into three 16-bit planes:
 *                 54 * CinP * CoutP64 float32 units (6 bytes per transformed weight).  Fused stages and statistics as PG_WINO_F4.
 *
 * Every form declines x2 and a pad_x outside [0, 4] (PG_ERR_UNSUPPORTED; use pg_conv2d_forward).  The three F(4x4) forms also decline -- callers then use
 * PG_WINO_F2 -- unless W % 4 == 0, x is 16-byte aligned, there is no input pre-activation stage (in_scale is supported), gain > 0 and an lrelu slope lies
 * in [0, 1] (their tail evaluates the activation as a max), SPADE mode has no in_scale, and stats_partial comes with the plain tail only.
 * Size limits (PG_ERR_TOO_LARGE): those of pg_conv2d_forward -- one image of x at most 2^31 - 1 bytes, the extent of y (through ystride) at most 2^31 - 1
 * elements, N * OH * OW at most 2^31 - 1 -- and, for every form, one IMAGE of y (and of residual / spade_x) at most 2^32 - 1 bytes: the tails add 32-bit byte
 * offsets to a 64-bit per-sample base.  N itself is not bounded: x, y, residual, spade_x and a per-sample noise plane may lie past 2, 4 and 8 GiB.
 */
enum { PG_WINO_F2 = 1, PG_WINO_F4 = 2, PG_WINO_F4B = 3, PG_WINO_F4X3 = 4 };
int64_t pg_conv2d_winograd_packed_size(int form, int Cout, int Cin);
int pg_conv2d_winograd_pack_weight(int form, const float* w, float* packed, int Cout, int Cin,
                                   float scale, int flip_hw, int transpose_oi, void* stream);
int pg_conv2d_winograd_forward(int form, const float* x, const float* packed_u, float* y,
                               int N, int Cin, int H, int W, int Cout, int pad_y, int pad_x, int OH, int OW,
                               const int64_t ystride[4], const pg_conv2d_fusion* fusion, void* stream);

/* Statistics gathered by PG_WINO_F4 / PG_WINO_F4X3 launches (pg_conv2d_fusion::stats_partial): tiles of one image for an OH x OW output, and the
 * reduction of the per-tile (sum, M2) pairs into mean[n*C + c] and rstd = 1 / sqrt(var + eps) (biased variance over OH*OW): Chan's pairwise merge in
 * float64, tiles in index order per lane, then a fixed-shape wave reduction -- deterministic, and not E[x^2] - E[x]^2.  T = pg_conv2d_winograd4_stats_tiles(OH, OW). */
int pg_conv2d_winograd4_stats_tiles(int OH, int OW);
int pg_instance_norm_finish(const float* stats_partial, float* mean, float* rstd, int NC, int T, int OH, int OW, float eps, void* stream);

/* Demodulation coefficients of modulated_conv2d (networks.py:64-68):
 *   dcoefs[n,o] = rsqrt(sum_{i,k} (w[o,i,k] * scale * styles[n,i])^2 + 1e-8);  w is OIHW. */
int pg_modconv_dcoefs(const float* w, const float* styles, float* dcoefs,
                      int N, int Cout, int Cin, int KHW, float scale, void* stream);

/* The same coefficients in two steps, for callers that keep weights across calls (eval): the tap energy
 *   w2[o,i] = scale^2 * sum_k w[o,i,k]^2        (pg_modconv_w2: weights only, once per weight version)
 * and the per-call style preparation (pg_modconv_prep, one launch):
 *   normalize != 0: smax[n] = max(max_i |styles[n,i]|, 1e-20), s' = styles / smax (the half-precision pre-normalisation of
 *                   networks.py:57-59); s_norm (float32 [N,Cin]) and s16 (bf16 / fp16 [N,Cin], half_dtype) receive s' when non-NULL
 *   normalize == 0: s' = styles
 *   out[n,o] = demodulate ? rsqrt(sum_i w2[o,i] * s'[n,i]^2 + 1e-8) : smax[n]. */
int pg_modconv_w2(const float* w, float* w2, int Cout, int Cin, int KHW, float scale, void* stream);
int pg_modconv_prep(const float* w2, const float* styles, float* out, float* s_norm, void* s16, int half_dtype,
                    int N, int Cout, int Cin, int normalize, int demodulate, void* stream);

/* pg_modconv_prep for every modulated convolution of a network in one launch (the per-layer launches are ~8 us each, 15 per step of the 1024^2 stack).
 * Job j = one pg_modconv_prep call: flags bit 0 = normalize, bit 1 = demodulate; `half_dtype` (PG_BF16 | PG_F16, or 0 when no job has an s16) is shared.
 * The table is passed BY VALUE to the kernel (a captured hipGraph keeps it; nothing is copied to the device per call). */
#define PG_MODCONV_PREP_MAX_JOBS 32
typedef struct {
    const float* w2[PG_MODCONV_PREP_MAX_JOBS];
    const float* styles[PG_MODCONV_PREP_MAX_JOBS];
    float*       out[PG_MODCONV_PREP_MAX_JOBS];
    float*       s_norm[PG_MODCONV_PREP_MAX_JOBS];
    void*        s16[PG_MODCONV_PREP_MAX_JOBS];
    int          cout[PG_MODCONV_PREP_MAX_JOBS];
    int          cin[PG_MODCONV_PREP_MAX_JOBS];
    int          flags[PG_MODCONV_PREP_MAX_JOBS];
    int          njobs;
    int          half_dtype;
} pg_modconv_prep_jobs;
int pg_modconv_prep_batched(const pg_modconv_prep_jobs* jobs, int N, void* stream);

/* Stride-2 transposed 3x3 convolution, all four output parities in one launch (csrc/conv2d_up2.h) -- the `up = 2` layers:
 * conv2d_gradfix.conv_transpose2d(stride=2, padding=0) behind conv2d_resample.py:125-142, with the modulation / demodulation of
 * networks.py:73-94 around it:
 *   y[n, co, 2 iy + ky, 2 ix + kx] += x[n, ci, iy, ix] * in_scale[n, ci] * w[co, ci, ky, kx];   y *= out_scale[n, co]
 * `packed` = pg_conv2d_pack_weight of the OIHW 3x3 kernel w.  y is [N, Cout, 2H+1, 2W+1] with strides `ystride` (elements; an even row
 * pitch gives 8-byte stores).  Every element of y is written (since ABI 6; before, the caller computed the last column ox = 2W itself).
 * in_scale / out_scale may be NULL. */
int pg_conv2d_up2_forward(const float* x, const float* packed, float* y, int N, int Cin, int H, int W, int Cout,
                          const int64_t ystride[4], const float* in_scale, const float* out_scale, void* stream);
/* Split-K form (ABI 11) for the low-resolution layers, whose few tiles would each walk all K chunks serially: `pg_conv2d_up2_splitk_plan` = the share
 * count the launch wants (1: call pg_conv2d_up2_forward).  Every tile then exists `ksplit` times, share z reduces its part of the input channels into slice z of
 * `workspace` (ksplit * N * ystride[0] floats, 16-byte aligned, laid out like y: y must be dense over n and N * ystride[0] % 4 == 0), and one pass adds the
 * slices into y in a fixed order. */
int pg_conv2d_up2_splitk_plan(int N, int Cin, int H, int W, int Cout);
int pg_conv2d_up2_forward_splitk(const float* x, const float* packed, float* y, int N, int Cin, int H, int W, int Cout,
                                 const int64_t ystride[4], const float* in_scale, const float* out_scale, float* workspace, int ksplit, void* stream);

/* Round 6 -- the same layer with its multiplies on the bf16 matrix pipe (csrc/conv2d_up2x3.h): every float32 operand the exact sum of three bf16 values
 * (truncation split), a float32 product = the six largest plane products on v_mfma_f32_32x32x16_bf16, float32 accumulation -- float32-class results at 6/16 of
 * the fp32 MFMA's issue time.  `packed` as above (its edge pass computes the last output column / row), `packed_x3` = pg_conv2d_up2x3_pack_weight(packed),
 * pg_conv2d_up2x3_packed_size(Cout, Cin) BYTES, once per weight version.  Serves W > 16, W % 4 == 0, Cin % 16 == 0, x 16-byte aligned; anything else
 * returns PG_ERR_UNSUPPORTED (callers then use pg_conv2d_up2_forward).  `edge_column`: N * Cin * H floats of scratch (the main kernel leaves input column W - 1
 * there for the kernel that makes the last output column / row, csrc/conv2d_up2_edges.h), or NULL (that kernel gathers the column from x: slower). */
int64_t pg_conv2d_up2x3_packed_size(int Cout, int Cin);
int pg_conv2d_up2x3_pack_weight(const float* packed, void* packed_x3, int Cout, int Cin, void* stream);
int pg_conv2d_up2x3_forward(const float* x, const float* packed, const void* packed_x3, float* y, int N, int Cin, int H, int W, int Cout,
                            const int64_t ystride[4], const float* in_scale, const float* out_scale, float* edge_column, void* stream);

/* Round 6 -- the 7x7 three-channel stem of the garment encoder (networks.py:2233-2238: Conv2dLayer(3, 64, kernel_size=7) = conv2d_resample.py:145-147 ->
 * conv2d_gradfix.conv2d, bias_act in the epilogue) on the bf16 matrix pipe with the three-term operand split (csrc/conv2d_stem7x3.h): float32-class results.
 * x [N, 3, H, W] contiguous, stride 1, padding 3; `packed` = pg_conv2d_stem7x3_pack_weight of the OIHW kernel w [Cout, 3, 7, 7] * scale (flip_hw as
 * pg_conv2d_pack_weight), pg_conv2d_stem7x3_packed_size(Cout) BYTES, once per weight version.  Fusion: bias, act in {linear, relu, lrelu}, gain, clamp;
 * any other stage set -> PG_ERR_UNSUPPORTED (callers then use pg_conv2d_forward). */
int64_t pg_conv2d_stem7x3_packed_size(int Cout);
int pg_conv2d_stem7x3_pack_weight(const float* w, void* packed, int Cout, float scale, int flip_hw, void* stream);
int pg_conv2d_stem7x3_forward(const float* x, const void* packed, float* y, int N, int H, int W, int Cout, const int64_t ystride[4],
                              const pg_conv2d_fusion* fusion, void* stream);

/* ABI 20 -- the fp32 stride-2 3x3 convolution with padding 0 (what follows the FIR pass of a `down = 2` 3x3 layer: conv2d_resample.py:119-122 ->
 * conv2d_gradfix.conv2d, bias_act in the epilogue, networks.py:170-179) on the bf16 matrix pipe (csrc/conv2d_s2x3.h): x [N, Cin, H, W] contiguous,
 * y [N, Cout, (H - 3) / 2 + 1, (W - 3) / 2 + 1] with strides ystride.  The arithmetic is pg_conv2d_up2x3_forward's: every float32 operand the exact sum of three
 * bf16 values (truncation split), a float32 product = the six largest of the nine plane products on v_mfma_f32_32x32x16_bf16, accumulated in float32, smallest
 * first.  The dropped products (each below 2^-24 of the product) and the behaviour on non-finite operands are as documented for conv2d_up2x3:
 * the split of +-inf leaves inf - inf = NaN in the second plane, so an infinite operand yields NaN where the fp32 kernel yields +-inf.  A NaN sample stays
 * local in the forward kernels that tests/test_nonfinite_locality.py lists: NaN in exactly the outputs that depend on it, -clamp under a fused clamp.
 * `packed_x3` = pg_conv2d_s2x3_pack_weight(packed) with `packed` = pg_conv2d_pack_weight of the OIHW 3x3 kernel; pg_conv2d_s2x3_packed_size(Cout, Cin) BYTES,
 * 16-byte aligned, once per weight version: [cout group of 128][16-channel chunk][m-block 4][tap 9][plane 3][k-half 2][32 couts][8 channels] bf16, zero
 * beyond Cout.  Serves Cin % 16 == 0, Cin >= 32, H, W >= 3, one image of x below 2^31 bytes.  x is read in whole aligned 16-byte words: of the memory outside
 * x only the rest of the 16-byte-aligned words that hold its first and last element is touched.  Fusion: bias, act in {linear, relu, lrelu}, gain, clamp;
 * any other stage set (residual, in_scale / out_scale, noise, SPADE, x2, statistics, an input pre-activation) -> PG_ERR_UNSUPPORTED before any launch
 * (callers then use pg_conv2d_forward). */
int64_t pg_conv2d_s2x3_packed_size(int Cout, int Cin);
int pg_conv2d_s2x3_pack_weight(const float* packed, void* packed_x3, int Cout, int Cin, void* stream);
int pg_conv2d_s2x3_forward(const float* x, const void* packed_x3, float* y, int N, int Cin, int H, int W, int Cout, const int64_t ystride[4],
                           const pg_conv2d_fusion* fusion, void* stream);

/* Streaming 1x1 convolution with few output channels (Cout <= 8; the ToRGB / parsing heads, networks.py:287-316,
 * modulated_conv2d with demodulate=False at networks.py:37-94): float32 NCHW, HW % 4 == 0, 16-byte aligned tensors:
 *   y[n,o,p] = clamp(sum_c x[n,c,p] * w[o,c] * scale * styles[n,c] + bias[o]) + skip[n,o,p]
 * styles / bias / skip may be NULL; clamp < 0 disables it.  PG_ERR_UNSUPPORTED otherwise (use pg_conv2d_forward). */
int pg_conv1x1_small(const float* x, const float* w, const float* styles, const float* bias, const float* skip, float* y,
                     int N, int Cin, int64_t HW, int Cout, float scale, float clamp, void* stream);

/* Folded heads: a linear 1x1 convolution over [x ; x2] followed by modulated linear 1x1 heads is one linear map of the two inputs per sample
 * (csrc/conv1x1_fold.hip); where only the heads' results are consumed the intermediate feature map is never written.
 *   pg_conv1x1_fold_prep:   w_out[n,o,c] = sum_k wh[o,k] * styles[n,k] * wm[k,c]          (wm [Cm, C] = the first convolution's weight with its gain applied)
 *                           b_out[n,o]   = sum_k wh[o,k] * styles[n,k] * bm[k] + bh[o]     (bm [Cm], bh [Cout], styles [N, Cm] may be NULL)
 *                           float64 accumulation in a fixed order; w_out [N, Cout, C], b_out [N, Cout].
 *   pg_conv1x1_fold_heads:  r[n,o,p] = clamp(sum_{c < C1} x[n,c,p] * w[n,o,c] + sum_{c < C2} x2[n,c,p] * w[n,o,C1 + c] + bias[n,o]) (+ skip[n,o,p] for o < n_skip)
 *                           channels [0, c_a) -> y_a [N, c_a, HW], channels [c_a, Cout) -> y_b [N, Cout - c_a, HW] (y_b NULL iff c_a == Cout);
 *                           skip [N, n_skip, HW] (NULL iff n_skip == 0); clamp < 0 disables it.  One pass over x and x2 with 16-byte loads.
 * float32 dense NCHW, Cout <= 16, HW % 4 == 0, 16-byte aligned tensors, (C1 + C2) * roundup(Cout, 4) * 4 bytes <= 64 KB; PG_ERR_UNSUPPORTED otherwise (run the
 * two convolutions one after the other). */
int pg_conv1x1_fold_prep(const float* wm, const float* bm, const float* wh, const float* bh, const float* styles, float* w_out, float* b_out,
                         int N, int Cm, int C, int Cout, void* stream);
int pg_conv1x1_fold_heads(const float* x, const float* x2, const float* w, const float* bias, const float* skip, float* y_a, float* y_b,
                          int N, int C1, int C2, int64_t HW, int Cout, int c_a, int n_skip, float clamp, void* stream);

/* Folded tail: a bias-free linear 3x3 convolution (padding 1) of xa plus a bias-free linear 1x1 convolution of xb, read only by a modulated linear 1x1 head,
 * is one linear map of (xa, xb) per sample (csrc/conv3x3_fold.hip); the sum of the two convolutions is never written.
 *   r[n,o,y,x] = clamp(sum_{c < C} sum_{ky,kx < 3} xa[n,c,y+ky-1,x+kx-1] * w[n,o,9c+3ky+kx] + sum_{c < C} xb[n,c,y,x] * w[n,o,9C+c] + bias[n,o]) (+ skip[n,o,y,x])
 * xa, xb [N, C, H, W]; w [N, Cout, 10 C] (pg_conv1x1_fold_prep over wm = [3x3 weight as [Cm, 9 C] | 1x1 weight [Cm, C]], cross-correlation as F.conv2d);
 * bias [N, Cout]; skip [N, Cout, H, W] or NULL; y [N, Cout, H, W]; samples of xa outside the image read as zero; clamp < 0 disables it.  One pass over xa
 * and xb with 16-byte loads, a fixed summation order, no atomics.
 * float32 dense NCHW, Cout <= 4, W % 4 == 0, 16-byte aligned tensors, H * W * 4 bytes <= 512 MB; PG_ERR_UNSUPPORTED otherwise (run the layers one after
 * the other). */
int pg_conv3x3_fold_head(const float* xa, const float* xb, const float* w, const float* bias, const float* skip, float* y,
                         int N, int C, int H, int W, int Cout, float clamp, void* stream);

/* 3x3 convolution of a one-channel image (first layer of the SPADE blocks on the parsing / mask map, networks.py:1708-1712):
 * y = act(conv2d(x [N,1,H,W], w [Cout,1,3,3] * scale, padding=1)), cross-correlation as F.conv2d; act = PG_ACT_LINEAR | PG_ACT_RELU
 * (gain 1).  float32, W % 4 == 0, 16-byte aligned; PG_ERR_UNSUPPORTED otherwise (use pg_conv2d_forward). */
int pg_conv3x3_cin1(const float* x, const float* w, float* y, int N, int H, int W, int Cout, float scale, int act, void* stream);

/* Per-(n,c) mean and rsqrt(var + eps) over H*W (nn.InstanceNorm2d(affine=False), networks.py:1713),
 * and the SPADE combine out = (x - mean) * rstd * (1 + gamma) + beta (networks.py:1722). */
int pg_instance_norm_stats(const float* x, float* mean, float* rstd, int NC, int64_t HW, float eps, void* stream);
int pg_spade_norm(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                  float* y, int NC, int64_t HW, void* stream);

/* The two passes above for the 16-bit (PG_BF16 | PG_F16) CHANNELS-LAST route (csrc/spade16.hip): x, y [N, H, W, C], C % 16 == 0, 16-byte aligned, HW = H * W.
 *   pg_instance_norm_stats_cl16: mean / rstd [N, C] float32 (biased variance), float32 accumulation of shifted data in two levels -- per pixel chunk, then
 *     over the chunks in chunk order; no atomics, bit-identical from run to run.  `workspace`: 2 * N * PG_STATS16_MAX_CHUNKS * C floats.  C <= 2048, N <= 65535.
 *   pg_spade_combine_cl16: y = clamp(act(((x - mean) * rstd) * (1 + gamma) + beta) * gain), gamma_beta [N, H, W, 2C] with gamma in the first C channels of a
 *     pixel (the output of the stacked gamma || beta convolution); act = PG_ACT_LINEAR (or 0) | PG_ACT_RELU | PG_ACT_LRELU (slope alpha); clamp < 0 disables
 *     it; rounded to the 16-bit type once, on the store.  N * HW * C / 8 < 2^31 (PG_ERR_TOO_LARGE otherwise).
 * PG_ERR_UNSUPPORTED: channel count, alignment or activation not covered. */
#define PG_STATS16_MAX_CHUNKS 256
int pg_instance_norm_stats_cl16(const void* x, float* mean, float* rstd, float* workspace, int dtype, int N, int64_t HW, int C, float eps, void* stream);
int pg_spade_combine_cl16(const void* x, const float* mean, const float* rstd, const void* gamma_beta, void* y, int dtype, int N, int64_t HW, int C,
                          int act, float alpha, float gain, float clamp, void* stream);

/* The same combine on the TRAINING route, with its gradient (autograd of networks.py:1715-1723: instance norm, then x_hat (1 + gamma) + beta).
 * x, y, dy, dx: [N, C, HW] contiguous.  gamma / beta (and dgamma / dbeta) may be planes of a larger tensor -- the two 3x3 convolutions that
 * produce them run as one launch over the stacked weights, output [N, 2C, HW]: plane (n, c) starts at base + n * sample_stride + c * HW.
 *   forward:   y = (x - mean) rstd (1 + gamma) + beta                      (mean / rstd from pg_instance_norm_stats)
 *   backward:  dbeta = dy,  dgamma = dy x_hat,  g = dy (1 + gamma),  dx = rstd (g - mean_hw(g) - x_hat mean_hw(g x_hat))
 * `sums`: 2 * N * C floats of scratch (the two plane means; fixed-order workgroup reductions: deterministic).  dx or the (dgamma, dbeta)
 * pair may be NULL when not needed. */
int pg_spade_train_forward(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* y,
                           int N, int C, int64_t HW, int64_t gamma_sample_stride, int64_t beta_sample_stride, void* stream);
int pg_spade_train_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* sums,
                            float* dx, float* dgamma, float* dbeta, int N, int C, int64_t HW,
                            int64_t gamma_sample_stride, int64_t dgamma_sample_stride, int64_t dbeta_sample_stride, void* stream);

/* Garment-feature assembly of the synthesis network (get_spade_feat + the merge, networks.py:2253-2276, 2311-2316) in two
 * launches instead of ~60 elementwise ones.  feat_*: [N,C,H,W]; masks: [N,1,2H,2W], sampled at the even pixels; with
 *   m = mask > 0.9,  v = m && denorm_mask > 0.9,  r = m - v,  count[n] = sum_p v,  sums[n,c] = sum_p feat * v:
 *   B   = feat * (1 - r) + sums / (count > 10 ? count : 256*256) * r
 *   out = B_upper * m_upper + B_lower * m_lower
 * pg_spade_masked_sums fills sums [N*C] and counts [N] of one branch. */
int pg_spade_masked_sums(const float* feat, const float* mask, const float* denorm_mask, float* sums, float* counts,
                         int N, int C, int H, int W, void* stream);
int pg_spade_feat_assemble(const float* feat_upper, const float* feat_lower, const float* mask_upper, const float* mask_lower,
                           const float* denorm_mask_upper, const float* denorm_mask_lower,
                           const float* sums_upper, const float* sums_lower, const float* counts_upper, const float* counts_lower,
                           float* out, int N, int C, int H, int W, void* stream);
int pg_conv2d_abi_version(void);
/* Multi-GPU training (round 5): keep `n` CUs free of this plugin's persistent grids (one workgroup per CU with most of its LDS: conv2d_wino4, conv2d_mfma16,
 * conv2d_wgrad, ...) so that RCCL's channel workgroups -- the gradient all-reduce launched from autograd hooks on a side stream, training/ddp.py -- find a CU
 * while the backward pass is still running.  0 = none.  Returns the CU count grids and split-K planners use from now on.  Process-wide, any device. */
int pg_conv2d_reserve_cus(int n);

/* Weight gradient of a float32 NCHW convolution (3x3 at stride 1 or 2, 1x1 at stride 1) -- what conv2d_gradfix.py:137-150 asks
 * aten::cudnn_convolution_backward_weight for:
 *   dw[co, ci, ky, kx] = sum_{n, oy, ox} dy[n, co, oy, ox] * x[n, ci, stride * oy + ky - pad_y, stride * ox + kx - pad_x]
 * A GEMM over pixels on the fp32 MFMA, split `splits` ways over the pixel axis with a fixed-order second pass (deterministic).
 * pg_conv2d_wgrad_plan returns the `splits` to use (0 = geometry not covered); `workspace` holds splits * KH*KW * Cout * Cin floats. */
int pg_conv2d_wgrad_plan(int N, int Cin, int OH, int OW, int Cout, int KH, int KW, int stride);
int pg_conv2d_wgrad(const float* x, const float* dy, float* dw, float* workspace,
                    int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad_y, int pad_x, int OH, int OW,
                    int splits, void* stream);

/* The same gradient for 16-bit (PG_F16 | PG_BF16) CHANNELS-LAST operands -- x [N, H, W, Cin], dy [N, OH, OW, Cout] -- on
 * v_mfma_f32_32x32x16_{f16,bf16} with float32 accumulation; dw is float32 [Cout, Cin, KH, KW].  Replaces aten::convolution_backward
 * (MIOpen) behind the half-precision discriminator blocks (reference conv2d_gradfix.py:137-150).  Covered: 3x3 stride 1 | 2, 1x1 stride 1,
 * Cin and Cout multiples of 8 (callers zero-pad the image channels of `fromrgb`).  pg_conv2d16_wgrad_plan returns the `splits` to use
 * (0 = not covered); `workspace` holds splits * KH*KW * Cout * Cin floats; deterministic (fixed-order reduction of the K splits). */
int pg_conv2d16_wgrad_plan(int N, int Cin, int OH, int OW, int Cout, int KH, int KW, int stride);
int pg_conv2d16_wgrad(const void* x, const void* dy, float* dw, float* workspace, int dtype,
                      int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad_y, int pad_x, int OH, int OW,
                      int splits, void* stream);

/* (ABI 11, exploratory: PG_WGRAD_BF16X3) The FLOAT32 weight gradient of pg_conv2d_wgrad on the bf16 matrix pipe by three-term operand splitting: every float32
 * value is the exact sum of three bf16 values (truncation), and of the nine partial products the six largest are accumulated in float32 -- float32-class results
 * (measured 1.3e-6 ... 2.8e-6 of max|dw| against float64; the fp32 MFMA kernel 1.0e-6 ... 1.7e-6), exact on integer data below 2^24 like the fp32 kernel.
 *   pg_split3_bf16_cl: float32 NCHW x [N, C, HW] -> out = three bf16 channels-last planes [3][N][HW][C], x == plane 0 + plane 1 + plane 2.  C % 8 == 0.
 *   pg_conv2d16_wgrad_x3: dw [Cout, Cin, KH, KW] from x3 = split(x), dy3 = split(dy): ONE launch of the 16-bit kernel over 6 N plane-mapped "images" (the six
 *   products share its float32 accumulation and fixed-order split reduction).  splits = pg_conv2d16_wgrad_plan(6 * N, ...); workspace as pg_conv2d16_wgrad. */
int pg_split3_bf16_cl(const float* x, void* out, int N, int C, int64_t HW, void* stream);
int pg_conv2d16_wgrad_x3(const void* x3, const void* dy3, float* dw, float* workspace,
                         int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad_y, int pad_x, int OH, int OW,
                         int splits, void* stream);

/* ------------------------------------------------------------------------
 * 16-bit convolution (bf16 / fp16 storage, fp32 accumulation) on v_mfma_f32_32x32x16_{bf16,f16}: what cuDNN does behind
 * conv2d_gradfix.py:35-43 for the reference's half-precision blocks (discriminator `use_fp16`, networks.py:444-523;
 * the StyleGAN2 synthesis blocks with use_fp16, networks.py:2147-2194).  Activations are NHWC ("channels_last", the
 * layout the reference's --nhwc option selects): x is [N, H, W, Cin] dense with Cin % 16 == 0.
 *
 * Weights are packed once per parameter version -- and, for a modulated convolution, once per style batch -- by
 * pg_conv2d16_pack_weight into [ceil(Cin/32)*2][KH*KW][2][CoutP][8] (CoutP = Cout rounded up to 64; zero filled):
 *   packed[n][ci/16][tap][(ci/8)&1][co][ci&7] = T(w[co][ci][tap] * scale * styles[n][ci] * dcoefs[n][co])
 * with w float32 OIHW (IOHW when transpose_oi), optionally flipped in both spatial axes; styles [nsamples, Cin] /
 * dcoefs [nsamples, Cout] float32 or NULL (= 1).  This is the reference's fused modulated convolution
 * (networks.py:85-94: per-sample weights w * styles * dcoefs cast to the activation dtype) without the grouped-conv
 * reshape.  `taps_y` / `taps_x` (NULL = all) select kernel rows / columns in the given order: the gather-form
 * sub-kernels of a stride-2 transposed convolution.  pg_conv2d16_packed_size = 16-bit elements per sample.
 */
int64_t pg_conv2d16_packed_size(int Cout, int Cin, int KH, int KW);
int pg_conv2d16_pack_weight(const float* w, void* packed, int dtype, int Cout, int Cin, int KH, int KW,
                            const int* taps_y, int ntaps_y, const int* taps_x, int ntaps_x,
                            float scale, int flip_hw, int transpose_oi,
                            const float* styles, const float* dcoefs, int nsamples, void* stream);
/* The same for `ngroups` weight tensors of one shape in ONE launch (the four composite phase kernels of an up-by-2 modulated
 * convolution share styles / dcoefs): group g reads w + g * w_group_stride (floats) and writes packed[(g * nsamples + n)]. */
int pg_conv2d16_pack_weight_grouped(const float* w, void* packed, int dtype, int ngroups, int64_t w_group_stride,
                                    int Cout, int Cin, int KH, int KW, float scale, int flip_hw, int transpose_oi,
                                    const float* styles, const float* dcoefs, int nsamples, void* stream);

/* The per-sample packs (styles and / or dcoefs given) of SEVERAL 3x3 layers in one launch -- the ~7 us pg_conv2d16_pack_weight launch per modulated
 * convolution and step is what this removes.  Job j packs w[j] (OIHW, or IOHW when flags bit 1 = transpose_oi; bit 0 = flip_hw; all nine taps -- or, flags bit 2, the six taps of a 3 x 2 kernel: the stack of pg_conv2d16_up2_fused, packed size of (cout, cin, 3, 2)) into
 * packed[j] ([nsamples][pg_conv2d16_packed_size(cout, cin, 3, 3)]) scaled by scale[j] * styles[j][n, ci] * dcoefs[j][n, co % dcoefs_mod[j]] (either may
 * be NULL; dcoefs_mod < cout serves the four stacked phases of an up = 2 layer, which share one coefficient row).  The table is passed by value. */
#define PG_CONV2D16_PACK_MAX_JOBS 16
typedef struct {
    const float* w[PG_CONV2D16_PACK_MAX_JOBS];
    void*        packed[PG_CONV2D16_PACK_MAX_JOBS];
    const float* styles[PG_CONV2D16_PACK_MAX_JOBS];
    const float* dcoefs[PG_CONV2D16_PACK_MAX_JOBS];
    int          cout[PG_CONV2D16_PACK_MAX_JOBS];
    int          cin[PG_CONV2D16_PACK_MAX_JOBS];
    int          flags[PG_CONV2D16_PACK_MAX_JOBS];
    int          dcoefs_mod[PG_CONV2D16_PACK_MAX_JOBS];
    float        scale[PG_CONV2D16_PACK_MAX_JOBS];
    int          njobs;
    int          nsamples;
    int          dtype;
} pg_conv2d16_pack_jobs;
int pg_conv2d16_pack_weight_batched(const pg_conv2d16_pack_jobs* jobs, void* stream);

/* Fused epilogue of pg_conv2d16_forward:  v = acc * out_scale[n,co] + noise[n?,oy,ox] * noise_gain + bias[co];
 * v = clamp(act(v) * gain);  y = T(v + residual).  Every pointer may be NULL; all vectors are float32. */
typedef struct pg_conv2d16_fusion {
    const float* out_scale;     /* [N, Cout] */
    const float* noise;         /* [OH, OW] (noise_batch_stride 0) or [N, OH, OW] */
    int64_t      noise_batch_stride;
    float        noise_gain;
    const float* bias;          /* [Cout] */
    int          act;           /* pg_act: linear / relu / lrelu */
    float        alpha;
    float        gain;          /* 0 => 1 */
    float        clamp;         /* < 0 = off */
    const void*  residual;      /* dtype / strides of y */
    /* Four output phases in one launch (the composite kernels of an up-by-2 layer, conv2d_resample.py:125-142 with the FIR folded in):
     * phase_cout > 0 => the Cout = 4 * phase_cout output channels are four blocks; block ph = 2a + b is written as channels
     * 0 .. phase_cout-1 of output pixel (oy * out_step_y + a, ox * out_step_x + b) (out_off_* ignored); out_scale / bias have
     * phase_cout entries per row; noise is [N?, 4, OH, OW] with noise_phase_stride elements between phases.  phase_cout must be 32
     * or a multiple of 64 (PG_ERR_UNSUPPORTED otherwise); no residual. */
    int          phase_cout;
    int64_t      noise_phase_stride;
} pg_conv2d16_fusion;

/*
 * y[n, co, oy*osy + ooy, ox*osx + oox] = epilogue(sum_{ci,ky,kx} packed[n * w_sample_stride ...][ci][ky,kx][co] *
 *                                                  x[n, oy*stride + ky - pad_y, ox*stride + kx - pad_x, ci])
 * (KH, KW, stride) in {(3,3,1), (1,1,1), (2,2,1), (2,1,1), (1,2,1), (3,3,2)}.  w_sample_stride = 0 (shared weights) or
 * pg_conv2d16_packed_size (per-sample weights).  y has dtype `out_dtype` -- the activation dtype or PG_F32 -- and strides
 * ystride[4] = (n, c, y, x) in elements: channels_last 16-bit outputs with Cout % 8 == 0 are written as 16-byte vectors,
 * anything else (a float32 NCHW image from a ToRGB layer, say) element by element.
 */
int pg_conv2d16_forward(const void* x, const void* packed, void* y, int dtype, int out_dtype,
                        int N, int Cin, int H, int W, int Cout, int KH, int KW,
                        int stride, int pad_y, int pad_x, int OH, int OW, int64_t w_sample_stride,
                        const int64_t ystride[4], int out_step_y, int out_step_x, int out_off_y, int out_off_x,
                        const pg_conv2d16_fusion* fusion, void* stream);

/* Round 5 -- the reference's up-by-2 modulated 3x3 layer (conv2d_resample.py:125-142: conv_transpose2d stride 2, then upfirdn2d with the
 * separable 4-tap filter, padding 1, gain 4; then noise / bias_act, networks.py:73-94) in ONE launch without the (2H+1)^2 intermediate and with
 * half the tap-products of the composite four-phase launch above: the y half of the filter is folded into the weights on the host, the x half
 * is applied to the accumulators in the epilogue (csrc/conv2d_up2f16.h).
 *   packed: pg_conv2d16_pack_weight(transpose_oi) of the float32 stack [Cin, 4 * Cout, 3, 2], channel block p = 2a + b of it holding, for output
 *           row parity a and intermediate column parity b, tap (ty, tx) = Ky_a[ty][kx(b, tx)] with Ky = (2 fy) (*)_y w (rows 4+a, 2+a, a of the
 *           6-row result) and kx(0, .) = (2, 0), kx(1, .) = (none, 1): the plain transposed convolution along x
 *           (training/networks.py `_up2_fused_weights` builds it);  w_sample_stride = 0 or pg_conv2d16_packed_size(4 * Cout, Cin, 3, 2).
 *   fir_x:  2 * fx, applied as out[o] = sum_X fir_x[o + 2 - X] * z[X] over the 2W+1 intermediate columns.
 *   y:      [N, Cout, 2H, 2W] 16-bit with ystride[1] == 1 (channels-last), written whole.
 *   fusion: out_scale / bias [.., Cout], noise [N?, 4, H, W] phase-major (noise_phase_stride between the planes of output pixel parities
 *           (a, b) = 2a + b), act / gain / clamp as pg_conv2d16_forward; no residual; phase_cout is ignored.
 * Cin % 16 == 0, Cin >= 32, Cout % 32 == 0. */
int pg_conv2d16_up2_fused(const void* x, const void* packed, void* y, int dtype, int N, int Cin, int H, int W, int Cout,
                          int64_t w_sample_stride, const int64_t ystride[4], const float fir_x[4],
                          const pg_conv2d16_fusion* fusion, void* stream);

/* Round 5 -- the optimizer side of a training phase in one launch (csrc/optim.hip): torch.nan_to_num(grad, nan, posinf, neginf) followed by torch.optim.Adam's
 * step (training_loop_fullbody.py:632-639) over the phase's flat buffers.  p / g / m / v share one flat layout (every parameter starts on a 16-byte boundary);
 * chunks[nchunks][4] = (element offset, length <= pg_adam_flat_chunk(), parameter index, 1 for the parameter's first chunk), one workgroup each.  A parameter
 * with alive[i] <= 0 (no rank produced a gradient: `grad is None` in the reference) is left untouched and keeps its step count; steps_in / steps_out are the
 * per-parameter step counts before / after (two buffers: the chunks of a parameter read the count while its first chunk writes it).  g is cleaned in place. */
int pg_adam_flat_chunk(void);
int pg_adam_flat_step(float* p, float* g, float* m, float* v, const int* chunks, int nchunks, const float* alive, const float* steps_in, float* steps_out,
                      float lr, float beta1, float beta2, float eps, float nan_value, float posinf_value, float neginf_value, void* stream);

/* Split-K form for launches with fewer output tiles than CUs: `ksplit` launches-worth of workgroups each reduce Cin/ksplit
 * channels into float32 [ksplit][N][OH][OW][Cout] `workspace`; one pass sums the slices in fixed order, applies the
 * epilogue and writes y.  pg_conv2d16_splitk_plan returns the ksplit this library would choose (1 = do not split). */
int pg_conv2d16_splitk_plan(int N, int Cin, int OH, int OW, int Cout, int KH, int KW, int stride);
int pg_conv2d16_forward_splitk(const void* x, const void* packed, void* y, int dtype, int out_dtype,
                               int N, int Cin, int H, int W, int Cout, int KH, int KW,
                               int stride, int pad_y, int pad_x, int OH, int OW, int64_t w_sample_stride,
                               const int64_t ystride[4], int out_step_y, int out_step_x, int out_off_y, int out_off_x,
                               const pg_conv2d16_fusion* fusion, float* workspace, int ksplit, void* stream);

/* 1x1 modulated convolution to a handful of output channels (ToRGB / parsing heads, networks.py:1957-1967) as a streaming
 * dot product: y[n, o, p] = clamp(sum_c x[n, p, c] * w[o, c] * styles[n, c] + bias[o]) + skip[n, o, p], x 16-bit NHWC,
 * w float32 [Cout, Cin] (already scaled by weight_gain), y / skip float32 NCHW; Cout <= 8, Cin % 8 == 0. */
int pg_conv1x1_small16(const void* x, const float* w, const float* styles, const float* bias, const float* skip, float* y,
                       int dtype, int N, int Cin, int64_t HW, int Cout, float clamp, int skip_up2_width, void* stream);
/* skip_up2_width = 0: `skip` has y's shape.  skip_up2_width = W (the width of y, even; H = HW / W even): `skip` is the HALF-resolution image
 * [N, Cout, H/2, W/2] and is up-sampled on the fly exactly as upfirdn2d.upsample2d does with the [1, 3, 3, 1] filter (networks.py:2165-2167 with
 * upfirdn2d.py:308-342: zero insertion, padding (2, 1), gain 4) -- the skip image's own FIR launch per block disappears. */

/* ------------------------------------------------------------------------
 * patch_routing_plugin.so -- the perspective warps of the data loader's patch routing (training/dataset.py:2555-2700; there:
 * cv2.warpPerspective / cv2.erode on the DataLoader thread).  8-bit interleaved (HWC) images.
 *
 * pg_warp_perspective_u8: `njobs` independent warps in one launch.  Each job maps a destination pixel (x, y) through `minv`
 * (the INVERSE of the matrix cv2.warpPerspective is given, row major, double) with OpenCV's arithmetic: block-wise coordinate
 * evaluation (block_w = the WarpPerspectiveInvoker block width for this destination size), 5 fractional bits, 15-bit bilinear
 * weights, taps outside the source read 0 (INTER_LINEAR, BORDER_CONSTANT 0).  `jobs_device` lives in device memory.
 * pg_patch_compose_u8: canvas[p] = erode8x8(mask[..., 0])[p] == 255 ? patch[p] : canvas[p] (and the same into canvas2 if given):
 * the paste step of the de-normalisation (dataset.py:2624-2633); patch / canvas are HxWx3, mask HxWxmask_channels.
 * The `_k` forms take the erode window: ksize x ksize, anchored at (ksize/2, ksize/2) as cv2.erode's default anchor, pixels outside the image
 * ignored; 1 <= ksize <= 16, anything else returns PG_ERR_INVALID_ARG.  8 is the upper try-on mode's window (dataset.py:2589), 5 the lower and
 * full modes' (:1827, :3345).  The forms without `_k` are the `_k` forms with ksize = 8.
 */
typedef struct {
    const unsigned char* src;
    unsigned char*       dst;
    int    src_h, src_w, dst_h, dst_w, channels, block_w;
    double minv[9];
} pg_warp_job;
int pg_warp_perspective_u8(const pg_warp_job* jobs_device, int njobs, int max_dst_pixels, void* stream);
int pg_patch_compose_u8(const unsigned char* patch, const unsigned char* mask, unsigned char* canvas, unsigned char* canvas2,
                        int h, int w, int mask_channels, void* stream);
int pg_patch_compose_u8_k(const unsigned char* patch, const unsigned char* mask, unsigned char* canvas, unsigned char* canvas2,
                          int h, int w, int mask_channels, int ksize, void* stream);
/* Round 6 -- the whole paste sequence of `njobs` canvases in one launch (a batch's de-normalised garments: dataset.py:2620-2633 run per part and per sample
 * in the reference): job = one h x w x 3 canvas, its parts in paste order (patch, mask; later parts overwrite earlier ones), and optionally a second canvas that
 * receives only the parts with to_canvas2 != 0.  Every pixel of the canvases is written (0 where no part's eroded mask is set).  `jobs_device` lives in device memory. */
#define PG_COMPOSE_MAX_PARTS 10
typedef struct pg_compose_job {
    unsigned char* canvas;
    unsigned char* canvas2;                              /* may be NULL */
    const unsigned char* patch[PG_COMPOSE_MAX_PARTS];    /* h x w x 3 */
    const unsigned char* mask[PG_COMPOSE_MAX_PARTS];     /* h x w x mask_channels, channel 0 is used */
    int nparts;
    int to_canvas2[PG_COMPOSE_MAX_PARTS];
    int pad_;
} pg_compose_job;
int pg_patch_compose_ordered_u8(const pg_compose_job* jobs_device, int njobs, int h, int w, int mask_channels, void* stream);
int pg_patch_compose_ordered_u8_k(const pg_compose_job* jobs_device, int njobs, int h, int w, int mask_channels, int ksize, void* stream);
/* The fused de-normalisation of the snapshot grid (training/snapshot_grid.py): ph x pw patches -> H x W canvas in one launch, without the warped
 * intermediates.  job = one H x W x 3 canvas and up to PG_COMPOSE_MAX_PARTS parts in paste order, each a ph x pw x 3 patch, a ph x pw x mask_channels mask
 * (channel 0 is used) and `minv` (as pg_warp_job's).  Every canvas pixel is written: the patch of the LAST part whose eroded warped mask is 255 there, warped;
 * 0 where there is none.  The result equals, byte for byte, pg_warp_perspective_u8 of every patch and mask to H x W with the same `block_w` followed by
 * pg_patch_compose_ordered_u8_k with the same `ksize` (1..16, anchor ksize / 2, taps outside the canvas ignored).  `jobs_device` lives in device memory.
 * PG_ERR_INVALID_ARG: NULL table, a non-positive size, ksize outside 1..16. */
typedef struct pg_denorm_job {
    unsigned char* canvas;
    const unsigned char* patch[PG_COMPOSE_MAX_PARTS];
    const unsigned char* mask[PG_COMPOSE_MAX_PARTS];
    double minv[PG_COMPOSE_MAX_PARTS][9];
    int nparts;
    int pad_;
} pg_denorm_job;
int pg_patch_denorm_u8(const pg_denorm_job* jobs_device, int njobs, int H, int W, int ph, int pw, int mask_channels, int ksize, int block_w, void* stream);
int pg_patch_routing_abi_version(void);

/* snapshot_grid_plugin.so -- the image snapshots of the training driver (training/snapshot_grid.py; the reference's save_image_grid,
 * training_loop_fullbody.py:313-340, :700-719).
 * pg_snapshot_cells_u8: a chunk of generator outputs -> cells first_cell .. first_cell + n - 1 of two uint8 HWC grid images on the device, each
 *   (gh + 1) H x (gw + 1) W x 3; cell i sits at grid row 1 + i / gw, grid column 1 + i % gw (row 0 and column 0 hold the persons; not written here).
 *   finetune_img float32 [n, 3, H, W] -> clip(rint((x + 1) * 127.5), 0, 255) in float32 without a fused multiply-add, rint half to even; NaN gives 0
 *   (NumPy leaves that cast undefined).  pred_parsing float32 [n, C, H, W], 1 <= C <= 16 -> grey[k] on all three channels, k the FIRST index of the
 *   maximal logit (a NaN logit never wins; all logits NaN or -inf: class 0); grey: C bytes in device memory.  W % 4 == 0, the float tensors 16-byte and the grids 4-byte aligned
 *   (PG_ERR_UNSUPPORTED otherwise); first_cell < 0 or first_cell + n > gh * gw: PG_ERR_INVALID_ARG. */
int pg_snapshot_cells_u8(const float* finetune_img, const float* pred_parsing, const unsigned char* grey, unsigned char* grid_img,
                         unsigned char* grid_parsing, int n, int C, int H, int W, int gh, int gw, int first_cell, void* stream);
int pg_snapshot_grid_abi_version(void);

/* augment_plugin.so -- ADA discriminator augmentation (training/augment.py, AugmentPipe).  float32, dense NCHW, C <= 65535 / 4 per sample batch.
 * pg_augment_warp: x [n, c, h, w] -> y [n, c, 2(h+6), 2(w+6)]: reflect-pad by `margins` (device int32 [mx0, my0, mx1, my1], each clamped to
 *   [0, w-1] / [0, h-1]), 2x upsample with the 12 taps `f` (device, the normalised sym6 filter), bilinear sampling (align_corners=False, zeros outside)
 *   through the per-sample matrices `g_inv` (device float32 [n, 3, 3], pixel_out -> pixel_in before padding).  The 2x downsample is a pg_upfirdn2d call.
 * pg_augment_warp_adjoint: dx = transpose(warp)(dy); `workspace` = n * c * 2(3h-2) * 2(3w-2) floats (need not be initialised).  No atomics.
 * pg_augment_color: per sample, mat = device float32 [n, C, C + 1]; mode 0: y[c] = sum_k mat[c][k] x[k] + mat[c][C]; mode 1 (transpose):
 *   y[c] = sum_k mat[k][c] x[k]; mode 2 (linear part): y[c] = sum_k mat[c][k] x[k].  C in {1, 3} (PG_ERR_UNSUPPORTED otherwise); hw = h * w. */
int pg_augment_warp(const float* x, float* y, const float* g_inv, const int* margins, const float* f, int n, int c, int h, int w, void* stream);
int pg_augment_warp_adjoint(const float* dy, float* workspace, float* dx, const float* g_inv, const int* margins, const float* f,
                            int n, int c, int h, int w, void* stream);
int pg_augment_color(const float* x, float* y, const float* mat, int n, int c, int hw, int mode, void* stream);
/* pg_augment_late: the pipe's late stages (augment.py:372-431) in one launch.  F = the separable correlation with the per-sample 1-D filter `taps` (device
 *   float32 [n, ntaps]; rows, then columns) behind a reflect pad of p = ntaps / 2 pixels; M = the cutout mask of `cut` (device float32 [n, 4] = centre x,
 *   centre y, size x, size y, in units of the image: 0 where |(xi + 0.5) / w - cx| < sx / 2 and likewise in y, else 1; float32, true division);
 *   `noise` = device [n, c, h, w], `sigma` = device [n].  A NULL `taps` / (`noise`, `sigma`) / `cut` switches that stage off.
 *   mode 0 (affine): y = M (F x + noise sigma);  mode 1 (linear): y = M F x;  mode 2 (adjoint): y = F^T (M x).  Modes 1 and 2 ignore the noise.
 *   The padded image and the row pass stay in LDS: no workspace.  No atomics: bit-identical per call.  Without a filter the noise is x + (noise sigma) with the
 *   product rounded first (no fused multiply-add) and the mask multiplies by 0 or 1: torch's composition bit for bit.
 *   PG_ERR_INVALID_ARG: NULL x / y, non-positive sizes, `noise` without `sigma` or the reverse, n * c > 65535, unknown mode.  PG_ERR_UNSUPPORTED: even
 *   ntaps, ntaps > 43 (the kernel's tap registers and halo are built for Hz_fbank's 43), h <= p or w <= p (reflect padding needs p + 1 samples). */
int pg_augment_late(const float* x, float* y, const float* taps, int ntaps, const float* noise, const float* sigma, const float* cut,
                    int n, int c, int h, int w, int mode, void* stream);
int pg_augment_abi_version(void);

/* tryon_plugin.so -- the staging on either side of the generator in the try-on driver (training/tryon.py; reference test.py:126-181).  Results equal
 * torch's GPU arithmetic bit for bit (u / 127.5 is u * (1.0f / 127.5f), no fused multiply-adds).
 * pg_tryon_row_extent_u8: canvases [ncanvases, h, w, channels] uint8 (16-byte aligned, w * channels % 16 == 0) -> extents int32 [ncanvases, 2]:
 *   the first and last row holding a non-zero byte, -1 / -1 when the canvas is empty.  One launch.
 * pg_tryon_inputs: the seven float32 NCHW inputs of training.dataset.to_generator_inputs for a batch of n, in one launch.  Sources are uint8 NHWC
 *   (H x W canvases, h x w part patches; W, w multiples of 4; dword-aligned), outputs dense float32 NCHW (16-byte aligned).  The bound plane is
 *   bound_rows[i, y] after the mode's post-routing rule: PG_TRYON_UPPER zeroes the rows above extents[i, 1] (the last row of
 *   denorm_upper_img_wo_sleeve); PG_TRYON_FULL adds 255 (mod 256) from row extents[i, 0] on (the routed lower garment's first row) and zeroes the plane
 *   when label[i] == 2 (a dress); PG_TRYON_LOWER takes the rows as they are (extents may be NULL).  An extent of -1 leaves the rows unchanged.
 *   PG_TRYON_OUTFIT (the top of one clothes image, the lower garment of another: not one of the reference's modes) takes PG_TRYON_FULL's rule.
 * pg_tryon_triptych_u8: finetune_img float32 [n, 3, H, W] + clothes, image uint8 [n, H, W, 3] -> out uint8 [n, H, 3 cw, 3]: columns x0 : x0 + cw of
 *   clothes | person | result.  result = clip((x + 1) * 127.5, 0, 255) truncated, NaN -> 0; clothes / person = ((u / 127.5 - 1) + 1) * 127.5 truncated
 *   (the reference's round trip, unclipped: it can be one below u).  x0, cw, W multiples of 4.
 * pg_tryon_panels_u8: the same packing for k source images (1 <= k <= PG_TRYON_MAX_PANEL_SOURCES; `sources` is a HOST array of k device pointers, each
 *   uint8 [n, H, W, 3]) -> out uint8 [n, H, (k + 1) cw, 3]: columns x0 : x0 + cw of source 0 | ... | source k-1 | result, every panel with the triptych's
 *   arithmetic.  The outfit mode packs upper clothes | lower clothes | person | result (k = 3); k = 2 is pg_tryon_triptych_u8. */
enum pg_tryon_mode { PG_TRYON_UPPER = 0, PG_TRYON_LOWER = 1, PG_TRYON_FULL = 2, PG_TRYON_OUTFIT = 3 };
#define PG_TRYON_MAX_PANEL_SOURCES 3
typedef struct pg_tryon_io {
    const unsigned char* image;            /* [n, H, W, 3] */
    const unsigned char* pose;             /* [n, H, W, 3] */
    const unsigned char* retain_mask;      /* [n, H, W, 1] */
    const unsigned char* denorm_upper;     /* [n, H, W, 3] */
    const unsigned char* denorm_lower;     /* [n, H, W, 3] */
    const unsigned char* norm_img;         /* [n, h, w, 30] */
    const unsigned char* norm_img_lower;   /* [n, h, w, 15] */
    const float* skin;                     /* [n, 3]: the skin medians (float32, NaN kept) */
    const int* label;                      /* [n]: 0, 1 or 2 */
    const unsigned char* bound_rows;       /* [n, H]: the host part of lower_clothes_upper_bound, one value per row */
    const int* extents;                    /* [n, 2] from pg_tryon_row_extent_u8 (upper: of denorm_upper_img_wo_sleeve; full: of the routed lower garment) */
    float* c;                              /* [n, 45, h, w] */
    float* retain;                         /* [n, 6, H, W] */
    float* pose_out;                       /* [n, 5, H, W] */
    float* denorm_upper_out;               /* [n, 3, H, W] */
    float* denorm_lower_out;               /* [n, 3, H, W] */
    float* upper_mask_out;                 /* [n, 1, H, W] */
    float* lower_mask_out;                 /* [n, 1, H, W] */
} pg_tryon_io;
int pg_tryon_row_extent_u8(const unsigned char* canvases, int ncanvases, int h, int w, int channels, int* extents, void* stream);
int pg_tryon_inputs(const pg_tryon_io* io, int n, int H, int W, int h, int w, int mode, void* stream);
int pg_tryon_triptych_u8(const float* finetune_img, const unsigned char* clothes, const unsigned char* image, unsigned char* out, int n, int H, int W,
                         int x0, int cw, void* stream);
int pg_tryon_panels_u8(const float* finetune_img, const unsigned char* const* sources, int k, unsigned char* out, int n, int H, int W, int x0, int cw,
                       void* stream);
int pg_tryon_abi_version(void);

/* train_fetch_plugin.so -- the data fetch of the training loop (training/train_fetch.py; reference training_loop_fullbody.py:549-601 and the tail of
 * its loader, training/dataset.py:1146-1170, :1223-1241).  Results equal torch's GPU arithmetic bit for bit, as for tryon_plugin.so.
 * pg_train_fetch: the nine float32 NCHW tensors of a round for a batch of n, in one launch.  Sources are uint8 NHWC (H x W canvases, h x w part
 *   patches; W, w multiples of 4; dword-aligned), outputs dense float32 NCHW (16-byte aligned).  Per sample i the erase decision erase[i] =
 *   (kind, rows flag, erase_length, use_random_mask) is applied while reading, unless extents[i, 0] < 0 (the routed lower mask of part 0 is empty):
 *   PG_ERASE_DROP_PART0 zeroes channels 0..2 of norm_img_lower and, with the rows flag, rows 0 : erase_length of channels 3..5 and 9..11;
 *   PG_ERASE_BAND zeroes rows ty : by of channels 0..2, ty = extents[i, 0], by = min(ty + 1 + floor(band_u[i] * (h - ty)), h) in float32.
 *   With use_random_mask (and random_mask != NULL) the canvases are zeroed where random_mask > 0 before the masks are taken. */
enum pg_erase_kind { PG_ERASE_NONE = 0, PG_ERASE_DROP_PART0 = 1, PG_ERASE_BAND = 2 };
typedef struct pg_train_io {
    const unsigned char* image;            /* [n, H, W, 3] */
    const unsigned char* pose;             /* [n, H, W, 3] */
    const unsigned char* retain_mask;      /* [n, H, W, 1]: 0 / 1 */
    const unsigned char* gt_parsing;       /* [n, H, W, 1]: 0 .. 6 */
    const unsigned char* random_mask;      /* [n, H, W, 1] or NULL */
    const unsigned char* denorm_upper;     /* [n, H, W, 3] */
    const unsigned char* denorm_lower;     /* [n, H, W, 3] */
    const unsigned char* norm_img;         /* [n, h, w, 30] */
    const unsigned char* norm_img_lower;   /* [n, h, w, 15], before the erase */
    const float* skin;                     /* [n, 3]: the skin medians (float32, NaN kept) */
    const int* label;                      /* [n]: 0, 1 or 2 */
    const unsigned char* bound_rows;       /* [n, H]: lower_clothes_upper_bound_for_train, one value per row */
    const int* extents;                    /* [n, 2] from pg_tryon_row_extent_u8 over the routed lower mask of part 0 ([n, h, w, 3]) */
    const int* erase;                      /* [n, 4]: kind (pg_erase_kind), rows flag, erase_length, use_random_mask */
    const float* band_u;                   /* [n]: u in [0, 1) of PG_ERASE_BAND */
    float* real_img;                       /* [n, 3, H, W] */
    float* style_input;                    /* [n, 45, h, w] */
    float* retain;                         /* [n, 6, H, W] */
    float* pose_out;                       /* [n, 5, H, W] */
    float* denorm_upper_out;               /* [n, 3, H, W] */
    float* denorm_lower_out;               /* [n, 3, H, W] */
    float* upper_mask_out;                 /* [n, 1, H, W] */
    float* lower_mask_out;                 /* [n, 1, H, W] */
    float* gt_parsing_out;                 /* [n, 1, H, W] */
} pg_train_io;
int pg_train_fetch(const pg_train_io* io, int n, int H, int W, int h, int w, void* stream);
int pg_train_fetch_abi_version(void);

/* tryon_front_plugin.so -- the try-on loader's pre-routing maps on the GPU (training/tryon_front.py): everything ``TryOnTestSet.unrouted`` builds per
 * pixel, from the decoded files and the key-point tables of ``TryOnTestSet.raw``, bit for bit (float64 in the loader's operation order, nothing
 * contracted).  The frame is H x H; the W-wide sources sit at columns left : left + W of it (images pad with 255, everything else with 0).
 * Three launches per batch, in this order on one stream, none of which reads anything back:
 * pg_tryon_front_stats: zeroes stats (a memset node) and fills, per sample, PG_FRONT_STATS int32: the pixel counts of the label groups {5,7} {6} {9}
 *   {12} of person_parsing [0..3] and clothes_parsing [4..7], H - (first row) of each group (0 = absent) [8..15], and the 3 x 256 histogram of the
 *   person's image bytes under labels {10,13} [16..783] (bin 0 is not read: the skin medians ignore zero bytes), and, when lower_src_parsing != NULL,
 *   the pixel counts of its four label groups [784..787] (0 otherwise).  No mode argument: the pointer's presence switches the count.
 * pg_tryon_front_bit_rows: bit_rows [n, 5, H, (H + 31) / 32] uint32, bit x % 32 of word x / 32 = pixel x: planes 0..3 the four arm bands (the
 *   quadrilateral bands[i, b] dilated along x by 35 (upper arm) or 28 (fore-arm); b = 2 * arm + (0 upper arm, 1 fore-arm), arm 0 = label 14), plane 4 the mode's
 *   canvas mask eroded along x (taps -4..+3, taps outside the frame ignored).  Reads stats (the canvas mask depends on the garment classes).
 * pg_tryon_front_compose: resolves the per-sample decisions from stats (garment classes, dress rules, label, bound, the skin medians) and writes every
 *   map of a ``collate_unrouted`` batch; finishes the dilation / erosion along y.  sleeve is written iff garment_parsing != NULL; canvas is not
 *   written in PG_TRYON_FULL and PG_TRYON_OUTFIT.
 * PG_TRYON_OUTFIT is PG_TRYON_FULL with the lower garment cut from a second clothes source: lower_img / lower_mask come from lower_src_img under the
 *   garment classes of lower_src_parsing; label = 0 if that parsing has pants, else 1 if it has a skirt, else 2 if clothes_parsing has a dress, else 1
 *   (nothing is zeroed for a dress); lower_clothes = lower_src_img padded like clothes; bit_rows writes no canvas plane.  The mode needs both lower
 *   sources (bit_rows, compose) and lower_clothes (compose), and lower_clothes must be NULL in every other mode: PG_ERR_INVALID_ARG otherwise, before
 *   anything is launched.
 * H % 4 == 0, H <= 4096, 0 <= left, left + W <= H; pointers 4-byte aligned (PG_ERR_UNSUPPORTED otherwise). */
#define PG_FRONT_STATS 788
#define PG_FRONT_PRIMS 37                  /* rows of the pose table: 19 limbs + 18 joints */
typedef struct pg_front_io {
    const unsigned char* person_img;       /* [n, H, W, 3] as decoded */
    const unsigned char* clothes_img;      /* [n, H, W, 3] */
    const unsigned char* person_parsing;   /* [n, H, W] */
    const unsigned char* clothes_parsing;  /* [n, H, W] */
    const unsigned char* garment_parsing;  /* [n, H, W] or NULL (no sleeve mask) */
    const int* pose_prims;                 /* [n, PG_FRONT_PRIMS, 8]: kind (0 none, 1 segment of thickness 5, 2 disc of radius 5), x0, y0, x1, y1, r, g, b;
                                              integer coordinates in the W-wide frame, painting order */
    const double* bands;                   /* [n, 4, 4, 2]: the arm bands' corners (x, y) in the H x H frame */
    const int* band_absent;                /* [n, 4]: non-zero = no band: the whole hand label is removed */
    const int* hip_top;                    /* [n, 2]: (valid, row) of the upper mode's hip rule; the row may be negative */
    int* stats;                            /* [n, PG_FRONT_STATS] scratch */
    unsigned int* bit_rows;                /* [n, 5, H, (H + 31) / 32] scratch */
    unsigned char* upper_img;              /* [n, H, H, 3] */
    unsigned char* lower_img;              /* [n, H, H, 3] */
    unsigned char* upper_mask;             /* [n, H, H, 3] */
    unsigned char* lower_mask;             /* [n, H, H, 3] */
    unsigned char* sleeve;                 /* [n, H, H, 1] or NULL */
    unsigned char* image;                  /* [n, H, H, 3] */
    unsigned char* clothes;                /* [n, H, H, 3] */
    unsigned char* pose;                   /* [n, H, H, 3] */
    unsigned char* retain_mask;            /* [n, H, H, 1] */
    unsigned char* canvas;                 /* [n, H, H, 3] or NULL (PG_TRYON_FULL, PG_TRYON_OUTFIT) */
    unsigned char* bound;                  /* [n, H] */
    float* skin;                           /* [n, 3] */
    int* label;                            /* [n] */
    /* PG_TRYON_OUTFIT (appended: a caller that fills the fields above by name leaves these NULL) */
    const unsigned char* lower_src_img;    /* [n, H, W, 3] as decoded: the lower clothes, or NULL */
    const unsigned char* lower_src_parsing;/* [n, H, W] or NULL */
    unsigned char* lower_clothes;          /* [n, H, H, 3] or NULL */
} pg_front_io;
int pg_tryon_front_stats(const pg_front_io* io, int n, int H, int W, void* stream);
int pg_tryon_front_bit_rows(const pg_front_io* io, int n, int H, int W, int left, int mode, void* stream);
int pg_tryon_front_compose(const pg_front_io* io, int n, int H, int W, int left, int mode, void* stream);
int pg_tryon_front_abi_version(void);

/* vgg_loss_plugin.so -- the non-convolution operators of the VGG19 perceptual loss (training/vgg_loss.py).  float32, dense NCHW; `planes` = n * c.
 * No atomics (bit-identical run to run), nothing read to the host, no allocation.
 * pg_maxpool2x2: y [planes, h/2, w/2] = max over the 2x2 windows of x [planes, h, w] (nn.MaxPool2d(2, 2): a trailing odd row / column is dropped);
 *   aten's scan: row-major from -inf, an element replaces the maximum when it is greater or NaN.  h, w >= 2.
 * pg_maxpool2x2_backward: dx [planes, h, w] = dy routed to the element that scan picks (recomputed from x), 0 elsewhere; EVERY element of dx is written.
 * pg_l1_pair_sum: x = `groups` tensors of m elements each, stacked; y = one tensor of m elements, read once for all groups.
 *   out[g] = scale * sum_i |x[g][i] - y[i]|.  `partials` = workspace of groups * pg_l1_pair_blocks(m) floats (need not be initialised).  Two launches.
 * pg_l1_pair_grad: dx[g][i] = sgn(x[g][i] - y[i]) * (s[g] / (float)denom); sgn(0) = 0; `s` = `groups` device floats. */
#define PG_L1_PAIR_MAX_GROUPS 8
#define PG_L1_PAIR_MAX_BLOCKS 1024
int pg_maxpool2x2(const float* x, float* y, int64_t planes, int h, int w, void* stream);
int pg_maxpool2x2_backward(const float* x, const float* dy, float* dx, int64_t planes, int h, int w, void* stream);
int pg_l1_pair_blocks(int64_t m);
int pg_l1_pair_sum(const float* x, const float* y, float* partials, float* out, int groups, int64_t m, double scale, void* stream);
int pg_l1_pair_grad(const float* x, const float* y, const float* s, float* dx, int groups, int64_t m, double denom, void* stream);
int pg_vgg_loss_abi_version(void);

/* image_metrics_plugin.so -- the paired reconstruction metrics (torch_utils/ops/image_metrics.py, training/metrics.py, calc_metrics.py): per pair of
 * uint8 images of one shape [h, w, channels] the exact sums sad = sum |a - b| and ssd = sum (a - b)^2 over all pixels and channels, and the mean
 * SSIM (Wang et al. 2004: separable 11-tap Gaussian window, sigma 1.5, taps normalised; "valid" positions only, (h - 10)(w - 10) per channel;
 * population moments; C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; mean over positions and channels).  An image is a base pointer, a row stride and a
 * pixel stride in elements (channel stride 1), so a pair may be two windows of one larger image; no byte outside a window is read, and nothing need be
 * aligned.  No atomics (bit-identical run to run, and a pair's result does not depend on the other pairs of the call); nothing read to the host.
 * The job table is given twice: `jobs_host` is read by the call itself (argument checks, grid size), `jobs_device` -- the same bytes in device
 * memory -- by the kernels.  pg_image_pair_metrics_workspace: bytes of `workspace` for that table (need not be initialised), or a negative PG_ERR_*.
 * pg_image_pair_metrics_u8: sad[j], ssd[j] (int64) and ssim[j] (float32) for j < npairs.  Two launches.  PG_ERR_INVALID_ARG for npairs <= 0, a NULL
 *   table or pointer, h or w < 11, channels outside {1, 3}, pix_stride < channels or row_stride < 1; PG_ERR_TOO_LARGE for h * w * channels >= 2^31 or
 *   npairs > PG_METRIC_MAX_PAIRS. */
#define PG_METRIC_MAX_PAIRS 65535
typedef struct pg_metric_pair {
    const unsigned char* a;                /* first byte of window a */
    const unsigned char* b;
    int64_t a_row_stride;                  /* elements between rows */
    int64_t b_row_stride;
    int a_pix_stride;                      /* elements between pixels, >= channels */
    int b_pix_stride;
    int h, w, channels;
    int pad_;
} pg_metric_pair;
int64_t pg_image_pair_metrics_workspace(const pg_metric_pair* jobs_host, int npairs);
int pg_image_pair_metrics_u8(const pg_metric_pair* jobs_host, const pg_metric_pair* jobs_device, int npairs, void* workspace,
                             int64_t* sad, int64_t* ssd, float* ssim, void* stream);
int pg_image_metrics_abi_version(void);

/* region_metrics_plugin.so -- the reconstruction metrics restricted to label regions, and the confusion count of two label maps
 * (torch_utils/ops/region_metrics.py, training/metrics.py, calc_metrics.py).
 *
 * A pg_region_pair is a pg_metric_pair plus `labels`: a uint8 [h, w] window (one label per pixel) with its own row stride and a pixel stride >= 1.
 * A region is a 32-bit set over the label values 0..31 (bit v set: label v belongs to it); a label >= 32 is in no region; regions may overlap.
 * Per pair j and region r, in ONE pass over the bytes of a, b and labels (the same 32 x 32-position tiles, per-tile origins and filter as the
 * image_metrics plugin):
 *   n          pixels whose label is in the region;
 *   sad, ssd   sum |a - b| and sum (a - b)^2 over those pixels and all channels, exact;
 *   positions  valid SSIM positions (y < h - 10, x < w - 10) whose centre pixel (y + 5, x + 5) is in the region;
 *   ssim_sum   the sum of the SSIM map (image_metrics definitions) over those positions and all channels, float64.
 * A region holding every label gives the sad / ssd of pg_image_pair_metrics_u8 and ssim_sum / (positions * channels) = its SSIM up to rounding.
 * No byte outside a window is read, nothing need be aligned; no atomics (bit-identical run to run, and a pair's result does not depend on the
 * other pairs of the call); every pixel is counted once across tile seams; nothing is read to the host.
 * The job table is given twice, as for pg_image_pair_metrics_u8; `regions` are `nregions` host words, read by the call itself.
 * pg_region_pair_metrics_workspace: bytes of `workspace` for that table and region count (need not be initialised), or a negative PG_ERR_*.
 * pg_region_pair_metrics_u8: counts[q][j][r] (int64, q = 0 n, 1 sad, 2 ssd, 3 positions: [4, npairs, nregions]) and ssim_sum[j][r] (float64).
 *   Two launches.  PG_ERR_INVALID_ARG for npairs <= 0, nregions outside 1..PG_REGION_MAX, a NULL table or pointer, h or w < 11, channels outside
 *   {1, 3}, a / b pix_stride < channels, labels pix_stride < 1 or a row_stride < 1; PG_ERR_TOO_LARGE for h * w * channels >= 2^31 or
 *   npairs > PG_METRIC_MAX_PAIRS.
 *
 * pg_label_confusion_u8: a pg_label_pair is two uint8 [h, w] windows `pred` and `target` (h, w >= 1, any row stride >= 1, pixel stride >= 1).
 * `pred_lut` / `target_lut` are 256 host bytes each: the class index (< classes) of a byte, or PG_LABEL_IGNORE.  For every pixel at which both
 * sides map to a class, out[j][target class][predicted class] (int64 [npairs, classes, classes]) is incremented: `out` is ADDED to (integer
 * atomics: exact, so order does not matter), the caller zeroes it -- or keeps a running count.  One launch.  PG_ERR_INVALID_ARG for npairs <= 0, a
 * NULL pointer, h or w < 1, a stride < 1, classes outside 1..PG_CONFUSION_MAX_CLASSES or a look-up value >= classes other than PG_LABEL_IGNORE;
 * PG_ERR_TOO_LARGE for h * w >= 2^31 or npairs > PG_METRIC_MAX_PAIRS. */
#define PG_REGION_MAX 8
#define PG_CONFUSION_MAX_CLASSES 16
#define PG_LABEL_IGNORE 255
typedef struct pg_region_pair {
    const unsigned char* a;                /* first byte of window a */
    const unsigned char* b;
    const unsigned char* labels;           /* first byte of the label window */
    int64_t a_row_stride;                  /* elements between rows */
    int64_t b_row_stride;
    int64_t l_row_stride;
    int a_pix_stride;                      /* elements between pixels, >= channels */
    int b_pix_stride;
    int l_pix_stride;                      /* >= 1 */
    int h, w, channels;
} pg_region_pair;
typedef struct pg_label_pair {
    const unsigned char* pred;
    const unsigned char* target;
    int64_t p_row_stride;                  /* elements between rows */
    int64_t t_row_stride;
    int p_pix_stride;                      /* elements between pixels, >= 1 */
    int t_pix_stride;
    int h, w;
} pg_label_pair;
int64_t pg_region_pair_metrics_workspace(const pg_region_pair* jobs_host, int npairs, int nregions);
int pg_region_pair_metrics_u8(const pg_region_pair* jobs_host, const pg_region_pair* jobs_device, int npairs, const uint32_t* regions, int nregions,
                              void* workspace, int64_t* counts, double* ssim_sum, void* stream);
int pg_label_confusion_u8(const pg_label_pair* jobs_host, const pg_label_pair* jobs_device, int npairs, const unsigned char* pred_lut,
                          const unsigned char* target_lut, int classes, int64_t* out, void* stream);
int pg_region_metrics_abi_version(void);

/* contextual_plugin.so -- the contextual loss (torch_utils/ops/contextual_ops.py, training/contextual_loss.py).  float32.  x = `samples` = G * n
 * feature maps [channels, positions] (G <= PG_CX_MAX_GROUPS groups of n stacked on the batch axis), y = n of them; sample s of x meets sample s % n
 * of y.  Per sample, with mu_p = mean_c y[c][p], xn_p = (x_p - mu_p) / (|x_p - mu_p| + 2.220446049250313e-16), yn likewise, d_ij = 1 - xn_i . yn_j:
 *   m_i = min_j d_ij at jmin_i (lowest j on ties), e_i = m_i + 1e-3, w_ij = exp((1 - d_ij / e_i) / h), S_i = sum_j w_ij,
 *   a_i = max_j w_ij / S_i (at jmin_i: w falls with d), CX = mean_i a_i, loss = -log CX.
 * No positions x positions element is written to memory: the products are streamed on the float32 matrix instruction.  No atomics (bit-identical
 * run to run), nothing read to the host, no allocation; every element of every output is written.
 * pg_cx_padded_channels: Cp = channels rounded up to 32 (0 for channels < 1).
 * pg_cx_prepare: xn [samples, positions, Cp], yn [n, positions, Cp] (position-major, padding zero, 16-byte aligned) and rx [samples, positions] =
 *   |x_p - mu_p|, from dense NCHW x and y of any alignment.  One launch.
 * pg_cx_prepare_backward: dx (dense NCHW) from dxn [samples, positions, Cp]: dx_p = (dxn_p - xn_p (xn_p . dxn_p) (r + eps) / r) / (r + eps), r = rx_p;
 *   a zero row where r == 0.
 * pg_cx_forward: the row statistics row_min = m, row_argmin = jmin, row_others = S' = sum_{j != jmin} w_ij, row_wd = T' = sum_j w_ij (d_ij - m_i) and
 *   row_a = a [samples, positions], and cx, loss [samples].  Two launches.
 * pg_cx_backward: dxn [samples, positions, Cp] = (g a / (h e)) (yn_jmin - V) - (g a (m - D) / (h e^2)) yn_jmin per row, g = -gout[s] / (positions
 *   cx[s]), V_i = sum_j (w_ij / S_i) yn_j, D_i = sum_j w_ij d_ij / S_i, both differences formed from S', T' and U' = sum_{j != jmin} w_ij yn_j without
 *   a cancellation; `gout` = `samples` device floats.  One launch.
 * PG_ERR_INVALID_ARG: NULL pointer, non-positive size, samples % n != 0, h <= 0; PG_ERR_UNSUPPORTED: more than PG_CX_MAX_GROUPS groups, a
 * position-major operand that is not 16-byte aligned; PG_ERR_TOO_LARGE: positions > 2^31 - 129, samples + n > 65535, an extent past 2^60. */
#define PG_CX_MAX_GROUPS 8
#define PG_CX_CHANNEL_PAD 32
int pg_cx_padded_channels(int channels);
int pg_cx_prepare(const float* x, const float* y, float* xn, float* yn, float* rx, int samples, int n, int channels, int64_t positions, void* stream);
int pg_cx_prepare_backward(const float* dxn, const float* xn, const float* rx, float* dx, int samples, int channels, int64_t positions, void* stream);
int pg_cx_forward(const float* xn, const float* yn, float* row_min, int* row_argmin, float* row_others, float* row_wd, float* row_a, float* cx,
                  float* loss, int samples, int n, int channels, int64_t positions, double h, void* stream);
int pg_cx_backward(const float* xn, const float* yn, const float* row_min, const int* row_argmin, const float* row_others, const float* row_wd,
                   const float* row_a, const float* cx, const float* gout, float* dxn, int samples, int n, int channels, int64_t positions, double h,
                   void* stream);
int pg_contextual_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PASTA_GAN_OPS_H */
