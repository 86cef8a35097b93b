"""PASTA-GAN++ generator-synthesis stack on the MI355X-native ops.

``modulated_conv2d`` keeps the reference's exact signature (training/networks.py:37-94) and
the classes keep the reference's names, constructor arguments, parameter names and forward
signatures (FullyConnectedLayer :99-128, Conv2dLayer :133-179, ResBlock :287-316,
Spade_Conv2dLayer :1586-1635, Spade_Norm_Block :1702-1723, Spade_ResBlockV4_512 :1859-1904,
ToRGBLayerFull_v1_v4/_v5 :1910-1967, SynthesisBlockFull_v1_v4/_v6 :1971-2194,
SynthesisNetworkFull_v18 :2198-2327), so a reference ``state_dict`` loads unchanged.
``SynthesisLayer`` -- used but never defined in the reference tree --
is defined here from its call-site contract.

Two execution routes, chosen per call:
  * inference route (no autograd graph needed, float32): every layer is ONE launch of the MFMA
    implicit-GEMM conv with its neighbours folded in -- style scaling and SPADE pre-activation
    in the prologue; demodulation, noise, bias, activation, gain, clamp and the residual /
    skip-image add in the epilogue (csrc/conv2d_kernel.h);
  * differentiable route: the same maths composed from this package's ops
    (conv2d_resample / upfirdn2d / bias_act / fma), each of which carries its own gradient.
Both run only on the GPU; there is no CPU path.
"""

import os
from typing import NamedTuple, Optional
import numpy as np
import torch
import torch.nn as nn

from torch_utils import misc
from torch_utils.ops import _native as nat
from torch_utils.ops import bias_act
from torch_utils.ops import conv2d_gradfix
from torch_utils.ops import conv2d_mfma
from torch_utils.ops import conv2d_mfma16
from torch_utils.ops import conv2d_resample
from torch_utils.ops import fma
from torch_utils.ops import upfirdn2d

SQRT_HALF = float(np.sqrt(0.5))


def _needs_graph(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _fast_ok(x, *others):
    return x.is_cuda and x.dtype == torch.float32 and not _needs_graph(x, *others)


def _fast16_ok(x, *others):
    """Inference route of the half-precision blocks: bf16 / fp16 activations on the 16-bit MFMA kernel."""
    return x.is_cuda and x.dtype in conv2d_mfma16.DTYPES and x.shape[1] % 16 == 0 and not _needs_graph(x, *others)


class _PackCache:
    """Packed-weight cache of one layer: re-packs when the parameter is updated in place or replaced."""

    def __init__(self):
        self._store = {}

    def get(self, tag, params, build):
        key = tuple((p.data_ptr(), p._version, p.device) for p in params) + (nat.cache_epoch[0],)
        hit = self._store.get(tag)
        if hit is None or hit[0] != key:
            hit = (key, build())
            self._store[tag] = hit
        return hit[1]


# ----------------------------------------------------------------------------

@misc.profiled_function
def normalize_2nd_moment(x, dim=1, eps=1e-8):
    return x * (x.square().mean(dim=dim, keepdim=True) + eps).rsqrt()


def _up2_geometry(kh, kw, fw, fh, padding, up=2):
    """Paddings of the transposed-conv + FIR route of conv2d_resample (conv2d_resample.py:92-142)."""
    px0 = px1 = py0 = py1 = padding
    px0 += (fw + up - 1) // 2 - (kw - 1)
    px1 += (fw - up) // 2 - (kw - up)
    py0 += (fh + up - 1) // 2 - (kh - 1)
    py1 += (fh - up) // 2 - (kh - up)
    pxt = max(min(-px0, -px1), 0)
    pyt = max(min(-py0, -py1), 0)
    return (pyt, pxt), [px0 + pxt, px1 + pxt, py0 + pyt, py1 + pyt]


@misc.profiled_function
def modulated_conv2d(x, weight, styles, noise=None, up=1, down=1, padding=0, resample_filter=None, demodulate=True,
                     flip_weight=True, fused_modconv=True, _cache=None, _epilogue=None):
    """StyleGAN2 weight-(de)modulated convolution; signature of the reference (training/networks.py:37-49).

    x [N, I, H, W]; weight [O, I, kh, kw]; styles [N, I]; noise broadcastable to the output or None; up / down integer
    resampling factors with `resample_filter` from upfirdn2d.setup_filter(); padding relative to the up-sampled image;
    flip_weight=True means correlation (what F.conv2d computes).  `fused_modconv` picks between the reference's two
    formulations (per-sample grouped weights, :85-94, or scaled activations, :73-82); they differ only in rounding and
    both are ONE launch here.  Private: `_cache` = the calling layer's packed-weight cache, `_epilogue` =
    dict(bias, act, alpha, gain, clamp, residual) folded into the same launch.
    """
    n = x.shape[0]
    cout, cin, kh, kw = weight.shape
    misc.assert_shape(weight, [cout, cin, kh, kw])
    misc.assert_shape(x, [n, cin, None, None])
    misc.assert_shape(styles, [n, cin])

    plain_geometry = down == 1 and up in (1, 2) and isinstance(padding, int)
    if plain_geometry and _fast_ok(x, weight, styles, noise):
        out = _modconv_fast(x, weight, styles, noise, up, padding, resample_filter, demodulate, flip_weight, _cache, _epilogue)
        if out is not None:
            return out
    if plain_geometry and _fast16_ok(x, weight, styles, noise):
        out = _modconv_fast16(x, weight, styles, noise, up, padding, resample_filter, demodulate, flip_weight, _cache, _epilogue)
        if out is not None:
            return out
    if plain_geometry and up == 1 and flip_weight and _train_fused_ok(x, weight, styles, noise, padding):
        return _modconv_train(x, weight, styles, noise, padding, demodulate, _epilogue)
    if plain_geometry and up == 2 and not flip_weight and _train_fused_up2_ok(x, weight, styles, noise, padding, resample_filter):
        return _modconv_train(x, weight, styles, noise, padding, demodulate, _epilogue, up2_filter=resample_filter)
    y = _modconv_graph(x, weight, styles, noise, up, down, padding, resample_filter, demodulate, flip_weight, fused_modconv)
    if _epilogue:                # the native layer declined (uncovered geometry): compose the tail from the ops
        ep = dict(_epilogue)
        res = ep.pop('residual', None)
        b = ep.get('bias')
        y = bias_act.bias_act(y, b.to(y.dtype) if b is not None else None, act=ep.get('act', 'linear'), alpha=ep.get('alpha'),
                              gain=ep.get('gain', 1.0), clamp=ep.get('clamp'))
        if res is not None:
            y = y + res.to(y.dtype)
    return y


def _modconv_fast(x, weight, styles, noise, up, padding, resample_filter, demodulate, flip_weight, cache, epilogue):
    cout, cin, kh, kw = (int(s) for s in weight.shape)
    n, _, h, w = x.shape
    cache = cache if cache is not None else _PackCache()
    ep = dict(epilogue) if epilogue else {}
    dcoefs = None
    if demodulate:      # weight-only tap energy cached per weight version; one small launch per call (networks.py:64-68)
        w2 = cache.get(('w2',), [weight], lambda: conv2d_mfma.modconv_w2(weight))
        dcoefs = conv2d_mfma.modconv_prep(w2, styles, cout)[0]
    if up == 1:
        if not conv2d_mfma.supported(kh, kw, 1):
            return None
        wg = conv2d_mfma.use_winograd(kh, kw, 1, cout, cin, pad=(padding, padding), hw=x.shape[2:], ep=ep)
        packed = cache.get(('plain', flip_weight, wg), [weight], lambda: conv2d_mfma.pack_weight(weight, flip=not flip_weight, winograd=wg))
        return conv2d_mfma.conv2d_forward(x, packed, cout, kh, kw, stride=1, pad=(padding, padding), in_scale=styles,
                                          out_scale=dcoefs, noise=noise, winograd=wg, **ep)
    # up == 2: stride-2 transposed conv (one gather-form launch per output phase), then the FIR.
    fw, fh = upfirdn2d._get_filter_size(resample_filter)
    tpad, fir_pad = _up2_geometry(kh, kw, fw, fh, padding)
    out_hw = ((h - 1) * 2 - 2 * tpad[0] + kh, (w - 1) * 2 - 2 * tpad[1] + kw)

    def build():
        # conv2d_resample hands conv_transpose2d the O<->I transposed weight, flipped iff flip_weight (its `not flip_weight` twist)
        wt = weight.detach().transpose(0, 1)
        if flip_weight:
            wt = wt.flip([2, 3])
        return conv2d_mfma.pack_transposed(wt.contiguous(), 2, tpad, (h, w), out_hw)
    if (kh, kw) == (3, 3) and tuple(tpad) == (0, 0) and os.environ.get('PG_UP2_FUSED', '1') != '0':
        # all four output parities from one staged halo (csrc/conv2d_up2.h); the kernel indexes w[co, ci, ky, kx] of conv_transpose2d,
        # i.e. the weight flipped iff flip_weight (conv2d_resample's `not flip_weight` twist, as in build() below)
        packs = cache.get(('up2_fused', flip_weight), [weight], lambda: conv2d_mfma.pack_up2(weight, flip=flip_weight))
        y = conv2d_mfma.conv_up2_forward(x, packs, cout, in_scale=styles, out_scale=dcoefs)
    else:
        phases = cache.get(('up2', flip_weight, h, w), [weight], build)
        if phases is None:
            return None
        y = conv2d_mfma.conv_transpose2d_forward(x, phases, cout, out_hw, stride=2, in_scale=styles, out_scale=dcoefs)
    if ep.get('residual') is None:      # FIR + noise + bias_act in one pass over the tensor
        fused = upfirdn2d.upfirdn2d_bias_act(y, resample_filter, padding=fir_pad, gain=4, noise=noise, b=ep.get('bias'), act=ep.get('act', 'linear'),
                                             alpha=ep.get('alpha') or 0.0, act_gain=ep.get('gain', 1.0), clamp=ep.get('clamp'))
        if fused is not None:
            return fused
    y = upfirdn2d.upfirdn2d(y, resample_filter, padding=fir_pad, gain=4)
    if noise is not None:
        y = y.add_(noise)
    if ep:
        res = ep.pop('residual', None)
        y = bias_act.bias_act(y, ep.get('bias'), act=ep.get('act', 'linear'), alpha=ep.get('alpha'), gain=ep.get('gain', 1.0), clamp=ep.get('clamp'))
        if res is not None:
            y = y.add_(res)
    return y


def _up2_composite_phases(wt_iohw, f):
    """Stride-2 transposed 3x3 convolution followed by the 4x4 FIR (gain 4, padding [1,1,1,1]) == one 6x6 kernel
    K = 4 * (f (*) w) applied at stride 2, i.e. four 3x3 convolutions of the LOW-resolution input, one per output parity
    (a, b):  out[2q+a, 2r+b] = sum_{ty,tx} K[1 - 2 ty + a, 1 - 2 tx + b] * x[q + ty - 1, r + tx - 1]   (index range -3..2).
    The (2H+1)^2 intermediate of the two-step form (conv2d_resample.py:125-142) is never written or read: in half
    precision that traffic, not the 4x multiply count, is what the layer costs.  Returns {(a, b): IOHW weights}."""
    cin, cout = int(wt_iohw.shape[0]), int(wt_iohw.shape[1])
    # full 2-D convolution of every 3x3 kernel with the 4x4 filter as nine shifted multiply-adds (K[i+a, j+b] += w[i, j] f[a, b]).
    # Not F.conv2d: with Cin*Cout one-pixel "images" MIOpen's solver search runs for minutes on the first call.
    g = (4 * f).to(wt_iohw.dtype)
    k6 = wt_iohw.new_zeros([cin, cout, 6, 6])
    for i in range(3):
        for j in range(3):
            k6[:, :, i:i + 4, j:j + 4] += wt_iohw[:, :, i:i + 1, j:j + 1] * g
    return {(a, b): k6[:, :, [4 + a, 2 + a, a]][:, :, :, [4 + b, 2 + b, b]].contiguous() for a in (0, 1) for b in (0, 1)}


def _up2_transposed_phases_2x2(wt_iohw):
    """conv_transpose2d(x, wt, stride=2, padding=0) for a 3x3 kernel as FOUR 2x2 correlations of the zero-padded (by 1) input, one per output
    parity (a, b), stacked along Cout in the order (0,0), (0,1), (1,0), (1,1) of the 16-bit kernel's four-phase launch:
        y[2q + a, 2r + b] = sum_{ty, tx} k_ab[ty, tx] * x[q - 1 + ty, r - 1 + tx],   q = 0..H, r = 0..W   ((H+1) x (W+1) positions per phase)
    with, per axis, parity 0: k[0] = w[2] (sample q - 1), k[1] = w[0] (sample q); parity 1: k[0] = 0, k[1] = w[1].  16 taps of which 9 are non-zero,
    against 36 of the composite kernels (`_up2_composite_phases`).  Position q = H of an odd parity lands on output row 2H + 1, one past the
    result: the caller gives the launch a (2H+2) x (2W+2) buffer.  Returns IOHW [Cin, 4 * Cout, 2, 2]."""
    cin, cout = int(wt_iohw.shape[0]), int(wt_iohw.shape[1])
    sel = {0: (2, 0), 1: (None, 1)}
    out = []
    for a in (0, 1):
        for b in (0, 1):
            k = wt_iohw.new_zeros([cin, cout, 2, 2])
            for ty, ky in enumerate(sel[a]):
                for tx, kx in enumerate(sel[b]):
                    if ky is not None and kx is not None:
                        k[:, :, ty, tx] = wt_iohw[:, :, ky, kx]
            out.append(k)
    return torch.cat(out, dim=1).contiguous()


def _separable_taps(f):
    """(fy, fx) with f == outer(fy, fx) for a rank-1 2-D filter (what upfirdn2d.setup_filter makes of [1, 3, 3, 1]), else None."""
    if f is None or f.ndim != 2:
        return None
    hit = getattr(f, '_pg_separable', None)      # (version, result) kept ON the tensor object: the read-back below is a host sync, which a graph capture forbids
    if hit is not None and hit[0] == f._version:
        return hit[1]
    g = f.detach().double().cpu()
    tot = float(g.sum())
    out = None
    if tot != 0.0:
        fy, fx = g.sum(dim=1), g.sum(dim=0) / tot
        if float((torch.outer(fy, fx) - g).abs().max()) <= 1e-6 * float(g.abs().max()):
            out = (fy.float(), fx.float())
    f._pg_separable = (f._version, out)
    return out


def _up2_fused_weights(wt_iohw, fy):
    """Weights of `conv2d_mfma16.conv_up2_fused` (csrc/conv2d_up2f16.h): the stride-2 transposed 3x3 convolution followed by the y half of the separable
    FIR (padding 1, gain 2 per axis) as a 3 x 2 kernel per phase p = 2a + b, stacked along Cout -> IOHW [Cin, 4 * Cout, 3, 2]:
        Ky = (2 fy) (*)_y w   (6 x 3: rows 4+a, 2+a, a are the taps of output-row parity a on input rows q-1, q, q+1 -- `_up2_composite_phases` in one axis)
        along x the plain transposed convolution of `_up2_transposed_phases_2x2`: column parity b of the (2W+1)-wide intermediate takes
        (x[r-1], x[r]) * (w[.., 2], w[.., 0]) for b = 0 and x[r] * w[.., 1] for b = 1 (its tx = 0 tap is zero and never loaded by the kernel).
    The x half of the filter runs in the kernel's epilogue on the accumulators."""
    cin, cout = int(wt_iohw.shape[0]), int(wt_iohw.shape[1])
    g = (2 * fy).to(wt_iohw.dtype).to(wt_iohw.device)
    k6 = wt_iohw.new_zeros([cin, cout, 6, 3])
    for i in range(3):
        k6[:, :, i:i + 4, :] += wt_iohw[:, :, i:i + 1, :] * g[None, None, :, None]
    sel = {0: (2, 0), 1: (None, 1)}
    out = []
    for a in (0, 1):
        rows = k6[:, :, [4 + a, 2 + a, a]]                           # [Cin, Cout, 3 (ty), 3 (kx)]
        for b in (0, 1):
            k = wt_iohw.new_zeros([cin, cout, 3, 2])
            for tx, kx in enumerate(sel[b]):
                if kx is not None:
                    k[:, :, :, tx] = rows[:, :, :, kx]
            out.append(k)
    return torch.cat(out, dim=1).contiguous()


def _up2_transposed_weight(weight, flip_weight):
    """The float32 IOHW weight conv2d_resample hands conv_transpose2d: O <-> I transposed, flipped iff flip_weight (its `not flip_weight` twist)."""
    wt = weight.detach().float().transpose(0, 1)
    return (wt.flip([2, 3]) if flip_weight else wt).contiguous()


def _up2_fused_cached(cache, weight, flip_weight, resample_filter):
    """([Cin, 4 Cout, 3, 2] stack, 2 * fx as four floats) of an up = 2 layer, once per weight version."""
    def build():
        fy, fx = _separable_taps(resample_filter)
        return _up2_fused_weights(_up2_transposed_weight(weight, flip_weight), fy), [2.0 * float(v) for v in fx]
    return cache.get(('up2_fusedx', flip_weight), [weight], build)


def _up2_composite_cached(cache, weight, flip_weight, resample_filter):
    """The four composite 3x3 phase kernels of an up = 2 layer ({(a, b): [Cin, Cout, 3, 3]}), once per weight version."""
    return cache.get(('up2_composite', flip_weight), [weight],
                     lambda: _up2_composite_phases(_up2_transposed_weight(weight, flip_weight), resample_filter.float()))


R16_UP1 = 'up1'                             # the forms of a 16-bit modulated convolution (`_Route16.form`).  up = 1: one launch
R16_FUSED_X = 'up2_fused_x'                 # up = 2, one launch: the y half of the FIR in the weights, its x half in the epilogue (`_up2_fused_weights`)
R16_COMPOSITE = 'up2_composite'             # up = 2, one four-phase launch of the composite 3x3 kernels (`_up2_composite_phases`) stacked along Cout
R16_COMPOSITE_X4 = 'up2_composite_x4'       # up = 2, the same kernels as four launches (a Cout the four-phase launch does not cover, or PG_UP2_MERGED=0)
R16_MERGED_T = 'up2_merged_t'               # up = 2, the transposed convolution's phases as ONE launch of 2x2 kernels (`_up2_transposed_phases_2x2`), then the FIR
R16_TRANSPOSED = 'up2_transposed'           # up = 2, every other shape: the transposed convolution's phases, one launch each, then the FIR
_R16_TAPS = {R16_FUSED_X: 24, R16_COMPOSITE: 36, R16_COMPOSITE_X4: 36, R16_MERGED_T: 16}        # packed tap slots per weight; the other forms pack kh * kw


class _Route16(NamedTuple):
    """How one 16-bit modulated convolution runs: `form` = one of the R16_* above; `shared` = one weight pack for the batch, with x * styles and demodulation as
    the epilogue's scale, instead of one pack per sample; `tpad` / `fir_pad` = the paddings of the transposed convolution and of the FIR (None for up = 1)."""
    form: str
    shared: bool
    tpad: Optional[tuple]
    fir_pad: Optional[list]


def _modconv16_route(weight_shape, hw, up, padding, resample_filter):
    """The route of a 16-bit modulated convolution: pure host logic over the shapes, read by `_modconv_fast16` and by the stack's batched preparation
    (`SynthesisStack._prepare_all`); nothing else decides any part of it.  The environment is read on every call."""
    cout, cin, kh, kw = (int(v) for v in weight_shape)
    h, w = (int(v) for v in hw)
    env = os.environ.get
    form, tpad, fir_pad = R16_UP1, None, None
    if up == 2:
        fw, fh = upfirdn2d._get_filter_size(resample_filter)
        tpad, fir_pad = _up2_geometry(kh, kw, fw, fh, padding)
        form = R16_TRANSPOSED
        policy = env('PG_UP2_POLICY', 'composite')
        weight_bound = cout * 36 > 2 * h * w
        four_phase = conv2d_mfma16.phases_supported(cout)       # the four phases stacked along Cout, ONE launch
        composite = ((kh, kw, fw, fh) == (3, 3, 4, 4) and tuple(tpad) == (0, 0) and list(fir_pad) == [1, 1, 1, 1] and resample_filter.ndim == 2
                     and env('PG_UP2_COMPOSITE', '1') != '0')
        # Per-layer policy, measured in round 4 and NOT adopted: the composite kernel has 36 taps per output phase set where the
        # reference's transposed convolution has 9 (conv2d_resample.py:125-142) -- 4x the multiplies and 4x the packed weights -- so the layers with
        # Cout * 36 > 2 * H * W (the 8^2 ... 64^2 inputs of the 1024-wide stack) were tried as the transposed convolution's four phases on ONE shared
        # weight pack + the channels-last FIR (PG_UP2_POLICY=auto).  Those layers are latency-bound, not multiply-bound: four phase launches of
        # 30-97 us + the FIR pass against ONE composite launch of 69-137 us -- config 5 2023 -> 1696 images/s on the same box
        # (profiles/r04_cfg5_up2_policy.txt).  What would pay is the four transposed phases as ONE launch (taps zero-padded to 2x2: 16 instead of 36).
        if composite and not (weight_bound and policy == 'auto'):
            # ... which is the `merged` policy (PG_UP2_POLICY=merged): the four transposed phases as 2x2 kernels (16 taps, 9 non-zero) stacked along Cout, ONE
            # launch (two-role form, 16 x 16-pixel tiles) into a (2H+2) x (2W+2) buffer, then the channels-last FIR with the fused tail on its [2H+1, 2W+1]
            # view, for the weight-dominated layers with H >= 32.  Built, parity-green (tests/test_conv16.py::test_up2_layer_routes_vs_oracle) and measured:
            # 512 -> 256 at 64^2 116 + FIR vs 143 us composite, 1024 -> 512 at 32^2 157 + FIR vs 144 us (the (H+1) x (W+1) = 33 x 33 positions pad 16 x 16 tiles
            # by 44 %, 64 K chunks per tile stay latency-bound); config 5 1882 vs 1921 images/s -- NOT adopted either.
            if weight_bound and min(h, w) >= int(env('PG_UP2_MERGED_T_MIN', '32')) and four_phase and policy == 'merged':
                form = R16_MERGED_T
            # fused-x (round 5): 18 tap-products per input position instead of the composite's 36 (the reference's transposed convolution has 9 + the FIR pass)
            elif (cin % 16 == 0 and cin >= 32 and cout % 32 == 0 and min(h, w) >= int(env('PG_UP2_FUSEDX_MIN', '32')) and env('PG_UP2_FUSEDX', '1') != '0'
                  and _separable_taps(resample_filter) is not None):
                form = R16_FUSED_X
            else:
                form = R16_COMPOSITE if four_phase and env('PG_UP2_MERGED', '1') != '0' else R16_COMPOSITE_X4
    # Weight-dominated layers (the low-resolution blocks: N per-sample copies of a 512..1024-channel kernel outweigh the
    # activations): the reference's NON-fused form (networks.py:73-84; its own choice for half precision at batch > 1,
    # networks.py:2152-2154) -- x * styles, ONE shared weight pack cached across steps, demodulation as the epilogue's
    # per-(n, cout) scale.  Styles are normalised per sample like networks.py:57-59 so that x * s stays in 16-bit range;
    # the factor returns through dcoefs (computed from the normalised styles).
    shared = cout * _R16_TAPS.get(form, kh * kw) > float(env('PG_MODCONV16_SHARED_RATIO', '1')) * h * w and env('PG_MODCONV16_SHARED', '1') != '0'
    return _Route16(form, shared, tpad, fir_pad)


class _PackSource16(NamedTuple):
    """What the one weight pack of a single-pack route is built from: the float32 tensor with pack_weight's `flip` / `transpose_oi`, whether the demodulation
    coefficients repeat four times along Cout (the stacked phases of an up = 2 layer), and the layer-cache tag of its shared pack."""
    w: torch.Tensor
    flip: bool
    transpose_oi: bool
    repeat4: bool
    shared_tag: tuple


def _modconv16_pack_source(cache, weight, flip_weight, resample_filter, route):
    """The `_PackSource16` of a layer on `route`, or None for the forms that run on more than one pack (four composite launches, the transposed phases)."""
    if route.form == R16_UP1:
        return _PackSource16(weight.detach().float(), not flip_weight, False, False, ('shared', flip_weight))
    if route.form == R16_FUSED_X:
        return _PackSource16(_up2_fused_cached(cache, weight, flip_weight, resample_filter)[0], False, True, True, ('up2_fusedx_shared', flip_weight))
    if route.form == R16_COMPOSITE:         # the four composite kernels stacked along Cout: [Cin, 4 Cout, 3, 3]
        wcat = cache.get(('up2_cat', flip_weight), [weight],
                         lambda: torch.cat(list(_up2_composite_cached(cache, weight, flip_weight, resample_filter).values()), dim=1).contiguous())
        return _PackSource16(wcat, False, True, True, ('up2_cat_shared', flip_weight))
    if route.form == R16_MERGED_T:
        wcat = cache.get(('up2_t_cat', flip_weight), [weight], lambda: _up2_transposed_phases_2x2(_up2_transposed_weight(weight, flip_weight)))
        return _PackSource16(wcat, False, True, True, ('up2_t_cat_shared', flip_weight))
    return None


def _modconv16_pack(cache, weight, src, shared, dtype, s32, dcoefs):
    """(packed, per-sample stride) of `src`: the shared pack from the layer cache; else the pack the stack's batch left for this layer
    (`SynthesisStack._prepare_all`); else T(w * styles * dcoefs) packed here (networks.py:85-94)."""
    if shared:
        return cache.get(src.shared_tag + (dtype,), [weight], lambda: conv2d_mfma16.pack_weight(src.w, dtype, flip=src.flip, transpose_oi=src.transpose_oi)[0]), 0
    hit = conv2d_mfma16.pack_lookup(src.w, dtype, src.flip, src.transpose_oi, s32)
    if hit is not None:
        return hit
    if dcoefs is not None and src.repeat4:
        dcoefs = dcoefs.repeat(1, 4)
    return conv2d_mfma16.pack_weight(src.w, dtype, flip=src.flip, transpose_oi=src.transpose_oi, styles=s32, dcoefs=dcoefs)[:2]


def _noise_phase_major(cache, noise, h, w):
    """Phase-major copy [B, 2, 2, h, w] of an output-resolution noise map, one pass; the constant map of inference (one tensor per parameter version,
    SynthesisLayer.forward) is copied once per version."""
    if noise is None:
        return None
    build = lambda: noise.reshape(-1, h, 2, w, 2).permute(0, 2, 4, 1, 3).contiguous()
    return build() if noise.requires_grad or noise.ndim != 2 else cache.get(('noise_phases',), [noise], build)


def _modconv_fast16(x, weight, styles, noise, up, padding, resample_filter, demodulate, flip_weight, cache, epilogue):
    """bf16 / fp16 inference route: the reference's fused form (networks.py:85-94) -- per-sample weights T(w * styles * dcoefs) packed by one small
    kernel -- or, where `route.shared`, its non-fused form on one pack for the batch; then the launches of `route.form` (`_modconv16_route`) with noise / bias /
    activation / gain / clamp (/ residual) in the epilogue of the convolution or, for the two forms that end in the FIR, of that pass."""
    cout, cin, kh, kw = (int(v) for v in weight.shape)
    n, _, h, w = x.shape
    cache = cache if cache is not None else _PackCache()
    ep = dict(epilogue) if epilogue else {}
    s32 = styles.detach().float()
    route = _modconv16_route((cout, cin, kh, kw), (h, w), up, padding, resample_filter)
    form, shared, tpad, fir_pad = route
    out_scale = dcoefs = None
    w2 = cache.get(('w2',), [weight], lambda: conv2d_mfma.modconv_w2(weight.detach().float())) if demodulate else None
    if shared:          # one launch: per-sample maximum, normalised styles (float32 + 16-bit), coefficients of the normalised styles
        out_scale, s32, s16 = conv2d_mfma.modconv_prep(w2, s32, cout, normalize=True, demodulate=demodulate, half_dtype=x.dtype)
        x = x * s16[:, :, None, None]
    elif demodulate:
        dcoefs = conv2d_mfma.modconv_prep(w2, s32, cout)[0]

    def single_pack():
        src = _modconv16_pack_source(cache, weight, flip_weight, resample_filter, route)
        return _modconv16_pack(cache, weight, src, shared, x.dtype, s32, dcoefs)
    if form == R16_UP1:
        if not conv2d_mfma16.supported(kh, kw, 1):
            return None
        packed, per = single_pack()
        return conv2d_mfma16.conv2d_forward(x, packed, cout, kh, kw, pad=(padding, padding), sample_stride=per, out_scale=out_scale, noise=noise, **ep)
    res = ep.pop('residual', None)
    if form == R16_FUSED_X:
        fir_x = _up2_fused_cached(cache, weight, flip_weight, resample_filter)[1]
        noise_phases = _noise_phase_major(cache, noise, h, w)
        packed, per = single_pack()
        y = conv2d_mfma16.conv_up2_fused(x, packed, cout, fir_x, sample_stride=per, out_scale=out_scale, noise=noise_phases, **ep)
    elif form in (R16_COMPOSITE, R16_COMPOSITE_X4):
        y = torch.empty([n, cout, 2 * h, 2 * w], dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        xcl = conv2d_mfma16.to_channels_last(x)
        noise_phases = _noise_phase_major(cache, noise, h, w)
        if form == R16_COMPOSITE:
            # cout block 2a + b is written to output phase (a, b): the input is read once, a quarter of the launches and of the split-K shares
            packed, per = single_pack()
            conv2d_mfma16.conv2d_forward(xcl, packed, cout, 3, 3, pad=(1, 1), out_hw=(h, w), y=y, sample_stride=per, out_scale=out_scale, noise=noise_phases,
                                         phases=True, **ep)
        else:
            phases = _up2_composite_cached(cache, weight, flip_weight, resample_filter)
            if shared:
                packs, per = cache.get(('up2_shared', flip_weight, x.dtype), [weight],
                                       lambda: [conv2d_mfma16.pack_weight(wab, x.dtype, transpose_oi=True)[0] for wab in phases.values()]), 0
            else:                       # the four per-sample phase packs in one launch
                stacked = cache.get(('up2_stacked', flip_weight), [weight], lambda: torch.stack(list(phases.values())).contiguous())
                packs, per = conv2d_mfma16.pack_weight_grouped(stacked, x.dtype, transpose_oi=True, styles=s32, dcoefs=dcoefs)
            for packed, (a, b) in zip(packs, phases):       # each phase with its samples of the output-resolution noise map
                conv2d_mfma16.conv2d_forward(xcl, packed, cout, 3, 3, pad=(1, 1), out_hw=(h, w), y=y, out_step=(2, 2), out_off=(a, b), sample_stride=per,
                                             out_scale=out_scale, noise=noise_phases[:, a, b] if noise is not None else None, **ep)
    else:
        # the FIR pass follows and carries the tail; where the pack is shared, demodulation is a per-(n, cout) scale, which commutes with the FIR
        if form == R16_MERGED_T:
            packed, per = single_pack()
            ybuf = torch.empty([n, cout, 2 * h + 2, 2 * w + 2], dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
            conv2d_mfma16.conv2d_forward(conv2d_mfma16.to_channels_last(x), packed, cout, 2, 2, pad=(1, 1), out_hw=(h + 1, w + 1), y=ybuf, sample_stride=per,
                                         out_scale=out_scale, phases=True)
            y = ybuf[:, :, :2 * h + 1, :2 * w + 1]                    # a pitched channels-last view: the FIR below reads it in place
        else:
            out_hw = ((h - 1) * 2 - 2 * tpad[0] + kh, (w - 1) * 2 - 2 * tpad[1] + kw)
            pack = lambda **kw_: conv2d_mfma16.pack_transposed(_up2_transposed_weight(weight, flip_weight), x.dtype, 2, tpad, (h, w), out_hw, **kw_)
            phases = cache.get(('up2_t_shared', flip_weight, x.dtype, tuple(tpad), (h, w)), [weight], pack) if shared else pack(styles=s32, dcoefs=dcoefs)
            if phases is None:
                return None
            y = conv2d_mfma16.conv_transpose2d_forward(x, phases, cout, out_hw, stride=2, **(dict(out_scale=out_scale) if out_scale is not None else {}))
        b = ep.get('bias')
        fused = upfirdn2d.upfirdn2d_bias_act(y, resample_filter, padding=fir_pad, gain=4, noise=noise, b=b, act=ep.get('act', 'linear'),
                                             alpha=ep.get('alpha') or 0.0, act_gain=ep.get('gain', 1.0), clamp=ep.get('clamp'))
        if fused is None:
            if not y.is_contiguous(memory_format=torch.channels_last):
                y = y.contiguous(memory_format=torch.channels_last)      # (the fused FIR declined the pitched view of the merged route: dense copy)
            y = upfirdn2d.upfirdn2d(y, resample_filter, padding=fir_pad, gain=4)
            if noise is not None:
                y = y.add_(noise.to(y.dtype))
            fused = bias_act.bias_act(y, b.to(y.dtype) if b is not None else None, act=ep.get('act', 'linear'), alpha=ep.get('alpha'),
                                      gain=ep.get('gain', 1.0), clamp=ep.get('clamp'))
        y = fused
    return y if res is None else y.add_(res)


fused_training_modconv = os.environ.get('PG_TRAIN_MODCONV', '1') != '0'    # False / PG_TRAIN_MODCONV=0: the differentiable composition (any order of derivative)


def _train_fused_ok(x, weight, styles, noise, padding):
    """The training-route modulated convolution as native launches: float32 GPU tensors, stride 1, images of >= 32 x 32 (below that the
    per-sample weight gradients cost more than the elementwise passes they replace), a geometry the weight-gradient kernel covers."""
    if not (fused_training_modconv and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and styles.dtype == torch.float32):
        return False
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, styles, noise))):
        return False
    cout, cin, kh, kw = (int(v) for v in weight.shape)
    n, _, h, w = x.shape
    if h * w < 32 * 32 or not conv2d_mfma.supported(kh, kw, 1) or kh - 1 - padding < 0:
        return False
    oh, ow = h + 2 * padding - kh + 1, w + 2 * padding - kw + 1
    if noise is not None and (noise.dtype != torch.float32 or noise.numel() not in (oh * ow, n * oh * ow)):
        return False
    return oh == h and ow == w and conv2d_mfma.weight_gradient_supported(1, cin, oh, ow, cout, kh, kw, 1)


def _train_fused_up2_ok(x, weight, styles, noise, padding, resample_filter):
    """The up = 2 layer (stride-2 transposed 3x3 convolution, 4x4 FIR, noise, bias_act) on the training route as native launches: the geometry
    of the one-launch transposed kernel (csrc/conv2d_up2.h), input images of >= 32 x 32, per-sample weight gradients covered."""
    if not (fused_training_modconv and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and styles.dtype == torch.float32):
        return False
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, styles, noise))):
        return False
    cout, cin, kh, kw = (int(v) for v in weight.shape)
    n, _, h, w = x.shape
    if (kh, kw) != (3, 3) or h * w < 32 * 32 or resample_filter is None or resample_filter.ndim != 2:
        return False
    fw, fh = upfirdn2d._get_filter_size(resample_filter)
    tpad, fir_pad = _up2_geometry(kh, kw, fw, fh, padding)
    oh, ow = 2 * h + 1 + fir_pad[2] + fir_pad[3] - fh + 1, 2 * w + 1 + fir_pad[0] + fir_pad[1] - fw + 1
    if tuple(tpad) != (0, 0) or min(fir_pad) < 0 or (oh, ow) != (2 * h, 2 * w):
        return False
    if noise is not None and (noise.dtype != torch.float32 or noise.numel() not in (oh * ow, n * oh * ow)):
        return False
    return conv2d_mfma.weight_gradient_supported(1, cout, h, w, cin, 3, 3, 2)      # dz -> x: a stride-2 convolution with O = Cin, I = Cout


def _modconv_train(x, weight, styles, noise, padding, demodulate, epilogue, up2_filter=None):
    """modulated_conv2d (up = 1, or up = 2 with `up2_filter`) + the layer's bias_act on the training route.  The demodulation coefficients stay torch ops on the
    [N, O, I, k, k] products (small next to the activations; autograd differentiates them); everything that touches activations is
    `_ModConvTrain`."""
    n = x.shape[0]
    dcoefs = None
    if demodulate:
        dcoefs = ((weight.unsqueeze(0) * styles.reshape(n, 1, -1, 1, 1)).square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()
    ep = dict(epilogue) if epilogue else {}
    res = ep.pop('residual', None)
    cfg = conv2d_gradfix._epilogue_cfg(ep)
    if cfg is not None and cfg[0] not in conv2d_mfma.FUSED_ACTS:
        cfg, tail = None, ep
    else:
        tail = None
    bias = ep.get('bias') if tail is None else None
    if up2_filter is not None:
        y = _ModConvUp2Train.apply(x, weight, styles, dcoefs, noise, bias, up2_filter, int(padding), cfg)
    else:
        y = _ModConvTrain.apply(x, weight, styles, dcoefs, noise, bias, int(padding), cfg)
    if tail is not None:
        b = tail.get('bias')
        y = bias_act.bias_act(y, b.to(y.dtype) if b is not None else None, act=tail.get('act', 'linear'), alpha=tail.get('alpha'), gain=tail.get('gain', 1.0), clamp=tail.get('clamp'))
    return y if res is None else y + res.to(y.dtype)


class _ModConvTrain(torch.autograd.Function):
    """y = bias_act(conv2d(x * s, w) * d + noise + b) with per-sample s [N, I] and d [N, O] (networks.py:73-82, the non-fused form the
    reference trains with, plus the layer's bias_act :176-178) as ONE forward launch, and its first-order gradient as native launches:

        dpre, db = bias_act'(dy; y)                         one pass (pg_bias_act_grad_bias)
        dx       = conv2d(dpre * d, w^T flipped) * s         one launch (the scales ride as in_scale / out_scale)
        H_n      = weight gradient of sample n for (x_n, dpre_n), UNSCALED operands -> [N, O, I, k, k]  (N launches of pg_conv2d_wgrad)
        dw = sum_n d_n s_n H_n    ds_n = sum_{o,k} w d_n H_n    dd_n = sum_{i,k} w s_n H_n        (small tensor ops)

    -- the reference's graph spends ~23 traversals of the activation tensors on the same quantities (x*s, fma, their products and
    plane sums in backward).  Second-order requests are refused loudly (set networks.fused_training_modconv = False for them)."""

    @staticmethod
    def forward(ctx, x, weight, styles, dcoefs, noise, bias, padding, ep):
        x, styles = x.contiguous(), styles.contiguous()
        dcoefs = dcoefs.contiguous() if dcoefs is not None else None
        cout, cin, kh, kw = (int(v) for v in weight.shape)
        fz = dict(act=ep[0], alpha=ep[1], gain=ep[2], clamp=ep[3] if ep[3] >= 0 else None) if ep is not None else {}
        wg = conv2d_mfma.use_winograd(kh, kw, 1, cout, cin, pad=(padding, padding), hw=x.shape[2:], ep=fz)
        y = conv2d_mfma.conv2d_forward(x, conv2d_gradfix._packed(weight, wg), cout, kh, kw, stride=1, pad=(padding, padding), in_scale=styles,
                                       out_scale=dcoefs, noise=noise, bias=bias, winograd=wg, **fz)
        ctx.save_for_backward(x, weight, styles, dcoefs, y if ep is not None else None)
        ctx.cfg = (padding, ep, tuple(noise.shape) if noise is not None else None, bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, styles, dcoefs, y = ctx.saved_tensors
        padding, ep, noise_shape, has_bias = ctx.cfg
        cout, cin, kh, kw = (int(v) for v in weight.shape)
        n = x.shape[0]
        need_x, need_w, need_s, need_d, need_noise, need_b = ctx.needs_input_grad[:6]
        dy = dy.contiguous()
        db = None
        if ep is not None:
            if has_bias and need_b:
                dy, db = bias_act._BiasActGrad.apply(dy, None, None, y, 1, ep[0], ep[1], ep[2], ep[3], True)
            else:
                dy = bias_act._BiasActGrad.apply(dy, None, None, y, 1, ep[0], ep[1], ep[2], ep[3])
        elif has_bias and need_b:
            db = bias_act.channel_sum(dy, 1)
        dnoise = dy.sum_to_size(noise_shape) if (need_noise and noise_shape is not None) else None
        dx = None
        if need_x:
            py, px = kh - 1 - padding, kw - 1 - padding
            wg = conv2d_mfma.use_winograd(kh, kw, 1, cin, cout, pad=(py, px), hw=dy.shape[2:])
            dx = conv2d_mfma.conv2d_forward(dy, conv2d_gradfix._packed(weight, wg, flip=True, transpose_oi=True), cin, kh, kw, stride=1, pad=(py, px),
                                            in_scale=dcoefs, out_scale=styles, winograd=wg)
        dw = ds = dd = None
        if (need_w and not conv2d_gradfix.weight_gradients_disabled) or need_s or need_d:
            per = torch.stack([conv2d_mfma.weight_gradient(x[i:i + 1], dy[i:i + 1], weight.shape, (padding, padding), stride=1) for i in range(n)])   # [N, O, I, k, k]
            dw, ds, dd = _fold_per_sample(per, weight, styles, dcoefs, need_w and not conv2d_gradfix.weight_gradients_disabled, need_s, need_d)
        return dx, dw, ds, dd, dnoise, db, None, None


def _fold_per_sample(per, weight, styles, dcoefs, need_w, need_s, need_d):
    """Per-sample weight gradients H_n [N, O, I, k, k] for UNSCALED operands -> (dw, dstyles, ddcoefs) of y_n = d_n conv(x_n s_n, w):
    dw = sum_n d_n s_n H_n,  ds_n[i] = sum_{o,k} w d_n H_n,  dd_n[o] = sum_{i,k} w s_n H_n."""
    n, cout = per.shape[0], per.shape[1]
    d1 = dcoefs if dcoefs is not None else torch.ones([n, cout], dtype=per.dtype, device=per.device)
    dw = ds = dd = None
    if need_w:
        dw = (per * (d1.unsqueeze(2) * styles.unsqueeze(1))[:, :, :, None, None]).sum(dim=0)
    if need_s or need_d:
        m = (per * weight.unsqueeze(0)).sum(dim=[3, 4])                  # [N, O, I]
        if need_s:
            ds = (m * d1.unsqueeze(2)).sum(dim=1)
        if need_d and dcoefs is not None:
            dd = (m * styles.unsqueeze(1)).sum(dim=2)
    return dw, ds, dd


class _ModConvUp2Train(torch.autograd.Function):
    """The up = 2 synthesis layer on the training route (networks.py:73-82 with conv2d_resample.py:125-142 inside, then bias_act):
        z = conv_transpose2d(x s, w^T, stride 2) d          one launch, all four output parities (csrc/conv2d_up2.h)
        y = bias_act(FIR_4x4(z) * 4 + noise + b)            one pass (upfirdn2d_bias_act)
    backward: bias_act' + db in one pass, the FIR's adjoint (one upfirdn2d pass), dx = conv2d(dz d, w^T, stride 2) s in one launch, and the
    per-sample stride-2 weight gradients folded like _ModConvTrain's."""

    @staticmethod
    def forward(ctx, x, weight, styles, dcoefs, noise, bias, f, padding, ep):
        x, styles = x.contiguous(), styles.contiguous()
        dcoefs = dcoefs.contiguous() if dcoefs is not None else None
        cout, cin, kh, kw = (int(v) for v in weight.shape)
        fw, fh = upfirdn2d._get_filter_size(f)
        _, fir_pad = _up2_geometry(kh, kw, fw, fh, padding)
        # x3=False: the training route keeps the fp32-MFMA kernel for this layer.  The bf16x3 form (csrc/conv2d_up2x3.h) is float32-class at the kernel call -- closer to
        # float64 than the fp32 kernel, tests/test_hip_parity.py -- but it is another draw of the forward's roundings, and the network-level gradient bars (frozen in round 5,
        # VERDICT r5 item 5) have two ill-conditioned tensors that move by 1.4e-3 of their maximum with it (4.3e-3 against the 3e-3 bar).  Cost: 1.6 ms of a 235 ms iteration.
        z = conv2d_mfma.conv_up2_forward(x, conv2d_mfma.pack_up2(weight, flip=False, x3=False), cout, in_scale=styles, out_scale=dcoefs, x3=False)
        act, alpha, gain, clamp = ep if ep is not None else ('linear', 0.0, 1.0, -1.0)
        y = upfirdn2d.upfirdn2d_bias_act(z, f, padding=fir_pad, gain=4, noise=noise, b=bias, act=act, alpha=alpha, act_gain=gain, clamp=clamp if clamp >= 0 else None)
        if y is None:                     # the fused FIR tail declined: the same steps one by one
            y = upfirdn2d.upfirdn2d(z, f, padding=fir_pad, gain=4)
            if noise is not None:
                y = y.add_(noise)
            y = bias_act.bias_act(y, bias, act=act, alpha=alpha, gain=gain, clamp=clamp if clamp >= 0 else None)
        ctx.save_for_backward(x, weight, styles, dcoefs, y if ep is not None else None, f)
        ctx.cfg = (fir_pad, ep, tuple(noise.shape) if noise is not None else None, bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, styles, dcoefs, y, f = ctx.saved_tensors
        fir_pad, ep, noise_shape, has_bias = ctx.cfg
        cout, cin, kh, kw = (int(v) for v in weight.shape)
        n, _, h, w = x.shape
        need_x, need_w, need_s, need_d, need_noise, need_b = ctx.needs_input_grad[:6]
        dy = dy.contiguous()
        db = None
        if ep is not None:
            if has_bias and need_b:
                dy, db = bias_act._BiasActGrad.apply(dy, None, None, y, 1, ep[0], ep[1], ep[2], ep[3], True)
            else:
                dy = bias_act._BiasActGrad.apply(dy, None, None, y, 1, ep[0], ep[1], ep[2], ep[3])
        elif has_bias and need_b:
            db = bias_act.channel_sum(dy, 1)
        dnoise = dy.sum_to_size(noise_shape) if (need_noise and noise_shape is not None) else None
        # adjoint of y = FIR(z): upfirdn2d with the flipped filter and the complementary padding (upfirdn2d.py:216-220 of this package)
        fw, fh = upfirdn2d._get_filter_size(f)
        zh, zw = 2 * h + 1, 2 * w + 1
        adj = (fw - fir_pad[0] - 1, zw - dy.shape[3] + fir_pad[0], fh - fir_pad[2] - 1, zh - dy.shape[2] + fir_pad[2])
        dz = upfirdn2d.upfirdn2d(dy, f, padding=adj, flip_filter=True, gain=4).contiguous()
        dx = None
        if need_x:      # z = conv_transpose2d(x, wt[Cin, Cout]) -> dx = conv2d(dz, wt read as OIHW with O = Cin, stride 2)
            dx = conv2d_mfma.conv2d_forward(dz, conv2d_gradfix._packed(weight, False, transpose_oi=True), cin, kh, kw, stride=2, pad=(0, 0),
                                            in_scale=dcoefs, out_scale=styles)
        dw = ds = dd = None
        want_w = need_w and not conv2d_gradfix.weight_gradients_disabled
        if want_w or need_s or need_d:
            # H'_n[ci, co, ky, kx] = sum x_n[ci, iy, ix] dz_n[co, 2 iy + ky, 2 ix + kx]: the weight gradient of the stride-2 convolution dz -> x
            per = torch.stack([conv2d_mfma.weight_gradient(dz[i:i + 1], x[i:i + 1], (cin, cout, kh, kw), (0, 0), stride=2) for i in range(n)]).transpose(1, 2)
            dw, ds, dd = _fold_per_sample(per, weight, styles, dcoefs, want_w, need_s, need_d)
        return dx, dw, ds, dd, dnoise, db, None, None, None


def _modconv_graph(x, weight, styles, noise, up, down, padding, resample_filter, demodulate, flip_weight, fused_modconv):
    """Differentiable composition (the two forms of networks.py:61-94)."""
    n = x.shape[0]
    cout, cin, kh, kw = weight.shape
    if x.dtype == torch.float16 and demodulate:      # keep fp16 in range (networks.py:57-59)
        weight = weight * (1 / np.sqrt(cin * kh * kw) / weight.norm(float('inf'), dim=[1, 2, 3], keepdim=True))
        styles = styles / styles.norm(float('inf'), dim=1, keepdim=True)
    per_sample = dcoefs = None
    if demodulate or fused_modconv:
        per_sample = weight.unsqueeze(0) * styles.reshape(n, 1, -1, 1, 1)
    if demodulate:
        dcoefs = (per_sample.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()
    if not fused_modconv:
        y = x * styles.to(x.dtype).reshape(n, -1, 1, 1)
        y = conv2d_resample.conv2d_resample(x=y, w=weight.to(x.dtype), f=resample_filter, up=up, down=down, padding=padding, flip_weight=flip_weight)
        if demodulate and noise is not None:
            return fma.fma(y, dcoefs.to(x.dtype).reshape(n, -1, 1, 1), noise.to(x.dtype))
        if demodulate:
            return y * dcoefs.to(x.dtype).reshape(n, -1, 1, 1)
        if noise is not None:
            return y.add_(noise.to(x.dtype))
        return y
    if demodulate:
        per_sample = per_sample * dcoefs.reshape(n, -1, 1, 1, 1)
    y = conv2d_resample.conv2d_resample(x=x.reshape(1, -1, *x.shape[2:]), w=per_sample.reshape(-1, cin, kh, kw).to(x.dtype), f=resample_filter,
                                        up=up, down=down, padding=padding, groups=n, flip_weight=flip_weight)
    y = y.reshape(n, -1, *y.shape[2:])
    if noise is not None:
        y = y.add_(noise)
    return y


# ----------------------------------------------------------------------------

class _GainedAlias(torch.autograd.Function):
    """`weight * gain` without the two elementwise launches: forward hands out the provider's pre-scaled copy (an alias, no kernel), backward passes the
    gradient through UNSCALED -- whoever installed the provider multiplies the parameter's accumulated gradient by `gain` once (training.ddp.GradBucket's
    gather).  Linear in its input, so double backward (R1) passes through it."""

    @staticmethod
    def forward(ctx, weight, scaled):
        return scaled.view_as(scaled)

    @staticmethod
    def backward(ctx, g):
        return g, None


# Installed by training.training_step.TrainingStep on the GPU (round 5, VERDICT r4 item 3: ~1 100 weight-gain multiplies per iteration): id(parameter) ->
# (pre-scaled float32 copy, parameter version it was made from).  The copies are refreshed by ONE multi-tensor pass after the optimizer step of their module
# set; a parameter whose version moved since (a checkpoint load, a broadcast) gets its copy refreshed on the spot.
_gained_provider = [None]


def _gained_weight(mod):
    """`mod.weight * mod.weight_gain` (reference networks.py:176 / :1620), through the provider's copy when there is one."""
    prov = _gained_provider[0]
    if prov is not None and torch.is_grad_enabled():
        hit = prov.get(id(mod.weight))
        if hit is not None and hit[2] is mod.weight:
            if hit[1] != mod.weight._version:     # written since the last refresh (a checkpoint load, a broadcast): bring this copy up to date here -- the bucket's
                with torch.no_grad():             # gather WILL multiply this parameter's gradient by the gain, so the multiply below must not be taken instead
                    hit[0].copy_(mod.weight.detach()).mul_(float(mod.weight_gain))
                hit[1] = mod.weight._version
            return _GainedAlias.apply(mod.weight, hit[0])
    return mod.weight * mod.weight_gain


class FullyConnectedLayer(nn.Module):
    def __init__(self, in_features, out_features, bias=True, activation='linear', lr_multiplier=1, bias_init=0):
        super().__init__()
        self.activation = activation
        self.weight = nn.Parameter(torch.randn([out_features, in_features]) / lr_multiplier)
        self.bias = nn.Parameter(torch.full([out_features], np.float32(bias_init))) if bias else None
        self.weight_gain = lr_multiplier / np.sqrt(in_features)
        self.bias_gain = lr_multiplier

    def forward(self, x):
        """Equalised-LR dense layer (reference networks.py:115-128): the runtime gains scale the operands, a linear layer
        is one GEMM with the bias in its epilogue (hipBLASLt), anything else hands bias + activation to bias_act."""
        weight = self.weight.to(x.dtype)
        bias = None
        if self.bias is not None:
            bias = self.bias.to(x.dtype)
            bias = bias if self.bias_gain == 1 else bias.mul(self.bias_gain)
        if x.ndim == 2:
            # the weight gain rides on the GEMM's alpha (no scaled copy of the weight per call)
            if self.activation == 'linear' and bias is not None:
                return torch.addmm(bias, x, weight.t(), alpha=self.weight_gain)      # 1-D bias: the GEMM's own bias epilogue, no broadcast copy
            y = torch.mm(x, weight.t()).mul_(self.weight_gain)
        else:
            y = torch.nn.functional.linear(x, weight.mul(self.weight_gain))
        if self.activation == 'linear' and bias is None:
            return y
        return bias_act.bias_act(y, bias, act=self.activation)


class _ConvBase(nn.Module):
    """Shared constructor of Conv2dLayer / Spade_Conv2dLayer (identical in the reference, :133-168 / :1586-1621)."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True, activation='linear', up=1, down=1,
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, channels_last=False, trainable=True):
        super().__init__()
        self.activation, self.up, self.down, self.conv_clamp = activation, up, down, conv_clamp
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        self.padding = kernel_size // 2
        self.weight_gain = 1 / np.sqrt(in_channels * (kernel_size ** 2))
        self.act_gain = bias_act.activation_funcs[activation].def_gain
        memory_format = torch.channels_last if channels_last else torch.contiguous_format
        weight = torch.randn([out_channels, in_channels, kernel_size, kernel_size]).to(memory_format=memory_format)
        bias = torch.zeros([out_channels]) if bias else None
        if trainable:
            self.weight = nn.Parameter(weight)
            self.bias = nn.Parameter(bias) if bias is not None else None
        else:
            self.register_buffer('weight', weight)
            if bias is not None:
                self.register_buffer('bias', bias)
            else:
                self.bias = None
        self._cache = _PackCache()

    def _packed(self, flip, winograd=False):
        return self._cache.get(('plain', flip, winograd), [self.weight],
                               lambda: conv2d_mfma.pack_weight(self.weight, scale=self.weight_gain, flip=flip, winograd=winograd))

    def _fast_geometry(self):
        k = int(self.weight.shape[2])
        return self.up == 1 and conv2d_mfma.supported(k, k, self.down) and self.activation in conv2d_mfma.FUSED_ACTS

    def _fast16_geometry(self, x, *others):
        """16-bit inference: a stride-1 layer the 16-bit MFMA convolution runs in one launch on these tensors."""
        k = int(self.weight.shape[2])
        return (_fast16_ok(x, self.weight, self.bias, *others) and self.up == 1 and self.down == 1 and conv2d_mfma16.supported(k, k, 1)
                and self.activation in conv2d_mfma16.FUSED_ACTS)


class Conv2dLayer(_ConvBase):
    """conv2d_resample -> bias_act (networks.py:170-179); `residual` (private) is added to the result."""

    def forward(self, x, gain=1, residual=None, x2=None, _filtered=None):
        """`x2` (private): a second input whose channels follow x's -- `layer(torch.cat([x, x2], 1))` without the copy.
        `_filtered` (private, inference route of a down = 2 layer): the FIR pass over x the caller has already made (ResBlock: one pass for both of its
        down = 2 layers) -- the full-resolution result for a 3x3 layer, its odd samples for a 1x1 layer."""
        act_gain = self.act_gain * gain
        act_clamp = self.conv_clamp * gain if self.conv_clamp is not None else None
        cout, _, k, _ = self.weight.shape
        try:
            y = self._forward_fused(x, act_gain, act_clamp, residual, x2, _filtered)
            if y is not None:
                return y
        except nat.NativeNotCovered:           # a valid request the kernels decline (size / geometry): compose it from the ops
            pass
        if x2 is not None:
            x, x2 = torch.cat([x, x2], dim=1), None
            if self._fast16_geometry(x, residual):
                # 16-bit inference (the try-on generator's half mode, merge_conv): the two channels-last inputs concatenated, then ONE launch of the 16-bit
                # MFMA convolution with bias / activation / gain / clamp (/ residual) in its epilogue
                packed = self._cache.get(('plain16', x.dtype), [self.weight], lambda: conv2d_mfma16.pack_weight(self.weight, x.dtype, scale=self.weight_gain)[0])
                return conv2d_mfma16.conv2d_forward(x, packed, cout, k, k, pad=(self.padding, self.padding), bias=self.bias, act=self.activation,
                                                    alpha=bias_act.activation_funcs[self.activation].def_alpha, gain=act_gain, clamp=act_clamp, residual=residual)
        w = _gained_weight(self)
        b = self.bias.to(x.dtype) if self.bias is not None else None
        # conv2d_resample -> bias_act (networks.py:176-178); on the GPU the bias_act rides in the convolution's epilogue where that is the route's last step
        # (16-bit activations on the GPU: the float32 weight goes down as it is -- conv2d_gradfix's 16-bit route packs from float32 and returns a float32 gradient)
        wx = w if (x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and w.dtype == torch.float32 and os.environ.get('PG_W32_ON_16', '1') != '0') else w.to(x.dtype)
        x = conv2d_resample.conv2d_resample(x=x, w=wx, f=self.resample_filter, up=self.up, down=self.down, padding=self.padding,
                                            flip_weight=(self.up == 1), _epilogue=dict(bias=b, act=self.activation, gain=act_gain, clamp=act_clamp))
        return x if residual is None else residual.add_(x) if not _needs_graph(residual, x) else residual + x

    def _forward_fused(self, x, act_gain, act_clamp, residual, x2, filtered=None):
        """Inference route: one launch of the MFMA convolution with bias / activation / gain / clamp / residual in its epilogue
        (after the FIR pass for down=2); None when this layer or these tensors do not qualify."""
        cout, _, k, _ = self.weight.shape
        if not (_fast_ok(x, self.weight, self.bias, residual, x2) and self._fast_geometry()):
            return None
        ep = dict(bias=self.bias, act=self.activation, alpha=bias_act.activation_funcs[self.activation].def_alpha, gain=act_gain,
                  clamp=act_clamp, residual=residual)
        if self.down == 1:
            if x2 is not None and x.shape[1] % 16 != 0:
                x, x2 = torch.cat([x, x2], dim=1), None
            if k == 7 and x.shape[1] == 3 and x2 is None and residual is None and conv2d_mfma.STEM7_X3:
                # round 6: the garment encoder's stem on the bf16 matrix pipe (three-term operand split, float32-class: csrc/conv2d_stem7x3.h)
                packed = self._cache.get(('stem7x3',), [self.weight], lambda: conv2d_mfma.pack_stem7(self.weight, scale=self.weight_gain))
                return conv2d_mfma.conv_stem7_forward(x, packed, cout, bias=self.bias, act=ep['act'], alpha=ep['alpha'], gain=ep['gain'], clamp=ep['clamp'])
            wg = conv2d_mfma.use_winograd(k, k, 1, cout, x.shape[1], x2, pad=(self.padding, self.padding), hw=x.shape[2:], ep=ep)
            return conv2d_mfma.conv2d_forward(x, self._packed(False, wg), cout, k, k, pad=(self.padding, self.padding), x2=x2, winograd=wg, **ep)
        if x2 is not None:
            x = torch.cat([x, x2], dim=1)
        # down == 2: FIR first (conv2d_resample.py:107-110, 119-122), then the (strided) conv with the fused epilogue
        fw, fh = upfirdn2d._get_filter_size(self.resample_filter)
        p = self.padding
        pads = [p + (fw - self.down + 1) // 2, p + (fw - self.down) // 2, p + (fh - self.down + 1) // 2, p + (fh - self.down) // 2]
        if k == 1:
            x = filtered if filtered is not None else upfirdn2d.upfirdn2d(x, self.resample_filter, down=self.down, padding=pads)
            return conv2d_mfma.conv2d_forward(x, self._packed(False), cout, 1, 1, **ep)
        x = filtered if filtered is not None else upfirdn2d.upfirdn2d(x, self.resample_filter, padding=pads)
        return conv2d_mfma.conv2d_forward(x, self._packed(False), cout, k, k, stride=self.down, **ep)


class ResBlock(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, bias=True, activation='linear', up=1, down=1,
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, channels_last=False, trainable=True):
        super().__init__()
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        kw = dict(resample_filter=resample_filter, conv_clamp=conv_clamp, channels_last=channels_last)
        self.conv0 = Conv2dLayer(in_channels, out_channels, kernel_size=3, activation=activation, up=up, down=down, bias=bias, **kw)
        self.conv1 = Conv2dLayer(out_channels, out_channels, kernel_size=3, activation=activation, bias=bias, **kw)
        self.skip = Conv2dLayer(in_channels, out_channels, kernel_size=1, bias=False, up=up, down=down, **kw)

    def forward(self, x):
        full = odd = None
        c0, sk = self.conv0, self.skip
        if (c0.down == 2 and sk.down == 2 and c0.up == 1 and sk.up == 1 and int(c0.weight.shape[2]) == 3 and int(sk.weight.shape[2]) == 1 and _fast_ok(x, c0.weight, sk.weight)
                and c0._fast_geometry() and sk._fast_geometry() and x.is_contiguous() and os.environ.get('PG_FIR_SHARED', '1') != '0'):
            # inference route, down = 2: both layers start with a FIR pass over x -- padding 2 in front of the strided 3x3 convolution, padding 1 and every second
            # sample in front of the 1x1 skip convolution (conv2d_resample.py:119-122, 107-110) -- and the second is the odd rows / columns of the first: one pass
            # writes both (round 6, pg_upfirdn2d_with_odd_samples; bit-identical)
            fw, fh = upfirdn2d._get_filter_size(self.resample_filter)
            p = c0.padding
            if fw == fh and fw % 2 == 0 and sk.padding == 0:
                try:
                    full, odd = upfirdn2d.filter_with_odd_samples(x, self.resample_filter, padding=[p + (fw - 1) // 2, p + (fw - 2) // 2, p + (fh - 1) // 2, p + (fh - 2) // 2])
                except nat.NativeNotCovered:
                    full = odd = None
        y = self.skip(x, gain=SQRT_HALF, _filtered=odd)
        x = self.conv0(x, _filtered=full)
        return self.conv1(x, gain=SQRT_HALF, residual=y)      # y + conv1(x), the add folded into conv1's epilogue


class Spade_Conv2dLayer(_ConvBase):
    """bias_act first (unless no_act), then the conv (networks.py:1623-1635).  On the inference route the
    pre-activation is the conv's prologue; `post_act` / `residual` (private) fold a following ReLU or add."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True, activation='relu', **kw):
        super().__init__(in_channels, out_channels, kernel_size, bias=bias, activation=activation, **kw)

    def pre_activation(self, gain=1):
        """The bias-free pre-activation of forward() as epilogue arguments for the producer of its input."""
        return dict(act=self.activation, alpha=bias_act.activation_funcs[self.activation].def_alpha, gain=self.act_gain * gain,
                    clamp=self.conv_clamp * gain if self.conv_clamp is not None else None)

    def forward(self, x, gain=1, no_act=False, post_act='linear', residual=None, stats_eps=None):
        """`stats_eps` (private, inference route): also return the instance-norm statistics (mean, rstd) of the OUTPUT -- the SPADE norm blocks
        that consume it need them (networks.py:1715-1723); gathered in the convolution's tail when the F(4x4) kernel runs it, by a second pass
        over the output otherwise.  Returns (y, (mean, rstd)) then."""
        act_gain = self.act_gain * gain
        act_clamp = self.conv_clamp * gain if self.conv_clamp is not None else None
        cout, _, k, _ = self.weight.shape
        if no_act and self._fast16_geometry(x, residual):
            # 16-bit inference (half mode): one launch, ReLU / residual in the epilogue; the statistics of the output by the channels-last pass over it
            packed = self._cache.get(('plain16', x.dtype), [self.weight], lambda: conv2d_mfma16.pack_weight(self.weight, x.dtype, scale=self.weight_gain)[0])
            y = conv2d_mfma16.conv2d_forward(x, packed, cout, k, k, pad=(self.padding, self.padding), act=post_act, residual=residual)
            return y if stats_eps is None else (y, conv2d_mfma16.instance_norm_stats16(y, eps=stats_eps))
        # a pre-activation bias cannot ride in the conv prologue (zero padding); none of the generator's SPADE convs has one
        if _fast_ok(x, self.weight, self.bias, residual) and self._fast_geometry() and self.down == 1 and (no_act or self.bias is None):
            pro = {} if no_act else dict(in_act=self.activation, in_gain=act_gain, in_clamp=act_clamp,
                                         in_alpha=bias_act.activation_funcs[self.activation].def_alpha)
            wg = conv2d_mfma.use_winograd(k, k, 1, cout, x.shape[1], pad=(self.padding, self.padding), hw=x.shape[2:], xf=not no_act)
            if stats_eps is not None and wg in (2, 4) and no_act and residual is None and post_act == 'linear' and os.environ.get('PG_FUSED_STATS', '1') != '0':
                try:
                    return conv2d_mfma.conv2d_forward(x, self._packed(False, wg), cout, k, k, pad=(self.padding, self.padding), winograd=wg, stats_eps=stats_eps)
                except nat.NativeNotCovered:
                    pass
            try:
                y = conv2d_mfma.conv2d_forward(x, self._packed(False, wg), cout, k, k, pad=(self.padding, self.padding), act=post_act, residual=residual,
                                               winograd=wg, **pro)
                return y if stats_eps is None else (y, conv2d_mfma.instance_norm_stats(y, eps=stats_eps))
            except nat.NativeNotCovered:       # e.g. a pre-activation in front of a geometry without the prologue variant
                pass
        w = _gained_weight(self)
        b = self.bias.to(x.dtype) if self.bias is not None else None
        if not no_act:
            x = bias_act.bias_act(x, b, act=self.activation, gain=act_gain, clamp=act_clamp)
        x = conv2d_resample.conv2d_resample(x=x, w=w.to(x.dtype), f=self.resample_filter, up=self.up, down=self.down, padding=self.padding,
                                            flip_weight=(self.up == 1), _epilogue=(dict(act=post_act, gain=1) if post_act != 'linear' else None))
        x = x if residual is None else residual + x
        return x if stats_eps is None else (x, conv2d_mfma.instance_norm_stats(x, eps=stats_eps))


class _SpadeCombine(torch.autograd.Function):
    """Training route of `normalized * (1 + gamma) + beta` with `normalized = InstanceNorm2d(affine=False)(x)` (networks.py:1715-1723) and its
    gradient as native passes (csrc/conv2d.hip, pg_spade_train_*): statistics + combine forward; two plane means + one elementwise pass backward
    (dx through the instance norm included) instead of the ~25 tensor traversals of the composed autograd graph.  `gamma_beta`: [N, 2C, H, W],
    gamma = the first C channels.  Higher-order requests differentiate the composition instead."""

    @staticmethod
    def forward(ctx, x, gamma_beta, eps):
        # (inputs are contiguous: `spade_combine` below makes them so OUTSIDE the Function -- a copy made in here, where grad mode is off, would be
        # detached from the graph, and the create_graph branch of backward would differentiate tensors that do not require grad: ADVICE r4)
        assert x.is_contiguous() and gamma_beta.is_contiguous()
        gb = gamma_beta
        mean, rstd = conv2d_mfma.instance_norm_stats(x, eps=eps)
        ctx.save_for_backward(x, gb, mean, rstd)
        ctx.eps = eps
        return conv2d_mfma.spade_train_forward(x, mean, rstd, gb)

    @staticmethod
    def backward(ctx, dy):
        x, gb, mean, rstd = ctx.saved_tensors
        if torch.is_grad_enabled() and any(t.requires_grad for t in (dy, x, gb)):
            with torch.enable_grad():
                c = x.shape[1]
                y = torch.nn.functional.instance_norm(x, eps=ctx.eps) * (1 + gb[:, :c]) + gb[:, c:]
                gx, ggb = torch.autograd.grad(y, [x, gb], dy, create_graph=True, allow_unused=True)
            return gx, ggb, None
        dx, dgb = conv2d_mfma.spade_train_backward(dy, x, mean, rstd, gb, need_dx=ctx.needs_input_grad[0], need_dgb=ctx.needs_input_grad[1])
        return dx, dgb, None


def spade_combine(x, gamma_beta, eps):
    """`_SpadeCombine` on contiguous inputs (made contiguous here, inside the graph)."""
    return _SpadeCombine.apply(x.contiguous(), gamma_beta.contiguous(), eps)


class Spade_Norm_Block(nn.Module):
    def __init__(self, in_channels, norm_channels):
        super().__init__()
        self.conv_mlp = Spade_Conv2dLayer(in_channels, norm_channels, kernel_size=3, bias=False)
        self.conv_mlp_act = nn.ReLU()
        self.conv_gamma = Spade_Conv2dLayer(norm_channels, norm_channels, kernel_size=3, bias=False)
        self.conv_beta = Spade_Conv2dLayer(norm_channels, norm_channels, kernel_size=3, bias=False)
        self.param_free_norm = nn.InstanceNorm2d(norm_channels, affine=False)
        self._cache = _PackCache()

    def forward(self, x, denorm_feats, post=None, stats=None):
        """`post` (private): dict(act, alpha, gain, clamp) -- the pre-activation of the one Spade_Conv2dLayer consuming the
        result (networks.py:1627-1633), applied here so that the consumer runs without a prologue.  `stats` (private):
        (mean, rstd) of x when the caller already has them (two norm blocks of a res-block normalise the same tensor)."""
        if _fast16_ok(x, denorm_feats, self.conv_mlp.weight, self.conv_gamma.weight, self.conv_beta.weight):
            return self._forward16(x, denorm_feats, post or {}, stats)
        if _fast_ok(x, denorm_feats, self.conv_mlp.weight, self.conv_gamma.weight, self.conv_beta.weight):
            post = post or {}
            mean, rstd = stats if stats is not None else conv2d_mfma.instance_norm_stats(x, eps=self.param_free_norm.eps)
            m = self.conv_mlp
            if conv2d_mfma.conv3x3_cin1_ok(denorm_feats, m.weight, m.padding) and m.up == 1 and m.down == 1 and os.environ.get('PG_CIN1_STENCIL', '1') != '0':
                actv = conv2d_mfma.conv3x3_cin1(denorm_feats, m.weight, scale=m.weight_gain, act='relu')     # one-channel map: a 9-tap stencil, output-stream bound
            else:
                actv = m(denorm_feats, no_act=True, post_act='relu')             # conv + ReLU in one launch
            g, b = self.conv_gamma, self.conv_beta
            c = int(g.weight.shape[0])
            if c % 32 == 0 and g._fast_geometry() and g.down == 1 and x.is_contiguous():
                # gamma and beta convolutions as ONE launch (they share `actv`) whose epilogue applies the normalisation
                wg = conv2d_mfma.use_winograd(3, 3, 1, 2 * c, actv.shape[1], pad=(g.padding, g.padding), hw=actv.shape[2:])
                packed = self._cache.get(('gamma_beta', wg), [g.weight, b.weight],
                                         lambda: conv2d_mfma.pack_spade_gamma_beta(g.weight, b.weight, g.weight_gain, b.weight_gain, winograd=wg))
                return conv2d_mfma.conv2d_forward(actv, packed, 2 * c, 3, 3, pad=(g.padding, g.padding), spade=(x, mean, rstd), winograd=wg, **post)
            gamma = g(actv, no_act=True)
            beta = b(actv, no_act=True)
            y = conv2d_mfma.spade_norm(x, mean, rstd, gamma, beta)
            return bias_act.bias_act(y, act=post['act'], alpha=post['alpha'], gain=post['gain'], clamp=post['clamp']) if post else y
        assert post is None and stats is None
        g, b = self.conv_gamma, self.conv_beta
        if (x.is_cuda and x.dtype == torch.float32 and denorm_feats.dtype == torch.float32 and os.environ.get('PG_TRAIN_SPADE', '1') != '0'
                and all(l.bias is None and l.up == 1 and l.down == 1 for l in (g, b)) and g.weight.shape == b.weight.shape):
            # training route on the GPU: conv + ReLU in one launch, the gamma and beta convolutions as ONE convolution over the stacked
            # weights (they share `actv`: one input gradient instead of two and their sum), instance norm + combine as _SpadeCombine
            actv = self.conv_mlp(denorm_feats, no_act=True, post_act='relu')
            w = torch.cat([_gained_weight(g), _gained_weight(b)], dim=0)
            gb = conv2d_resample.conv2d_resample(x=actv, w=w, f=g.resample_filter, padding=g.padding, flip_weight=True)
            return spade_combine(x, gb, self.param_free_norm.eps)
        normalized = self.param_free_norm(x)
        actv = self.conv_mlp_act(self.conv_mlp(denorm_feats, no_act=True))
        gamma = self.conv_gamma(actv, no_act=True)
        beta = self.conv_beta(actv, no_act=True)
        return normalized * (1 + gamma) + beta


    def _forward16(self, x, denorm_feats, post, stats):
        """16-bit inference (half mode), x channels-last bf16 / fp16: conv_mlp + ReLU in one launch (the one-channel parsing map keeps the float32 stencil, its
        output is cast), gamma || beta as ONE convolution over the stacked weights, then the streaming combine with the consumer's pre-activation."""
        mean, rstd = stats if stats is not None else conv2d_mfma16.instance_norm_stats16(x, eps=self.param_free_norm.eps)
        m, g, b = self.conv_mlp, self.conv_gamma, self.conv_beta
        if (denorm_feats.dtype == torch.float32 and conv2d_mfma.conv3x3_cin1_ok(denorm_feats, m.weight, m.padding) and m.up == 1 and m.down == 1
                and os.environ.get('PG_CIN1_STENCIL', '1') != '0'):
            actv = conv2d_mfma.conv3x3_cin1(denorm_feats, m.weight, scale=m.weight_gain, act='relu').to(dtype=x.dtype, memory_format=torch.channels_last)
        else:
            actv = m(denorm_feats.to(dtype=x.dtype, memory_format=torch.channels_last), no_act=True, post_act='relu')
        c = int(g.weight.shape[0])
        packed = self._cache.get(('gamma_beta16', x.dtype), [g.weight, b.weight],
                                 lambda: conv2d_mfma16.pack_weight(torch.cat([g.weight.detach() * g.weight_gain, b.weight.detach() * b.weight_gain]), x.dtype)[0])
        gb = conv2d_mfma16.conv2d_forward(actv, packed, 2 * c, 3, 3, pad=(g.padding, g.padding))
        return conv2d_mfma16.spade_combine16(x, mean, rstd, gb, **post)


class Spade_ResBlockV4_512(nn.Module):
    def __init__(self, in_channels, out_channels, spade_channels, kernel_size=3, bias=True, activation='linear', up=1, down=1,
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, channels_last=False, trainable=True, resolution=256):
        super().__init__()
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        kw = dict(bias=False, resample_filter=resample_filter, conv_clamp=conv_clamp, channels_last=channels_last)
        self.conv = Spade_Conv2dLayer(in_channels, in_channels, kernel_size=3, **kw)
        self.conv0 = Spade_Conv2dLayer(in_channels, out_channels, kernel_size=3, **kw)
        self.conv1 = Spade_Conv2dLayer(out_channels, out_channels, kernel_size=3, **kw)
        self.skip = Spade_Conv2dLayer(in_channels, out_channels, kernel_size=1, **kw)
        self.spade_skip = Spade_Norm_Block(spade_channels, in_channels)
        self.spade0 = Spade_Norm_Block(spade_channels, in_channels)
        self.spade1 = Spade_Norm_Block(spade_channels, out_channels)

    def forward(self, x, denorm_feat, _defer_tail=False):
        """`_defer_tail` (private): on the float32 inference route stop in front of the linear tail `conv1(h') + skip(s')` and return (h', s') -- the two SPADE
        outputs, each with its consumer's pre-activation applied -- for a caller that folds the tail into what reads it (`tail` finishes it otherwise)."""
        if (_fast_ok(x, denorm_feat, self.conv.weight, self.conv0.weight) or _fast16_ok(x, denorm_feat, self.conv.weight, self.conv0.weight)) and all(l.bias is None and l.activation in conv2d_mfma.FUSED_ACTS for l in (self.skip, self.conv0, self.conv1)):
            # inference route: each SPADE output feeds exactly one convolution, so that convolution's pre-activation is applied
            # where the SPADE output is produced and the convolutions run without a prologue; the statistics the norm blocks need come out of
            # the tail of the convolution that produces their input (round 4: no second pass over x / dx)
            assert self.spade_skip.param_free_norm.eps == self.spade0.param_free_norm.eps
            x, stats = self.conv(x, no_act=True, stats_eps=self.spade0.param_free_norm.eps)       # spade_skip and spade0 normalise the same x
            s = self.spade_skip(x, denorm_feat, post=self.skip.pre_activation(SQRT_HALF), stats=stats)
            defer = _defer_tail and s.dtype == torch.float32
            y = None if defer else self.skip(s, no_act=True)
            x, stats1 = self.conv0(self.spade0(x, denorm_feat, post=self.conv0.pre_activation(), stats=stats), no_act=True, stats_eps=self.spade1.param_free_norm.eps)
            h = self.spade1(x, denorm_feat, post=self.conv1.pre_activation(SQRT_HALF), stats=stats1)
            return (h, s) if defer else self.conv1(h, no_act=True, residual=y)
        x = self.conv(x, no_act=True)
        y = self.skip(self.spade_skip(x, denorm_feat), gain=SQRT_HALF)
        x = self.conv0(self.spade0(x, denorm_feat))
        return self.conv1(self.spade1(x, denorm_feat), gain=SQRT_HALF, residual=y)

    def tail(self, h, s):
        """The tail a `_defer_tail` call left out: conv1(h') + skip(s'), the launches of the undeferred inference route."""
        return self.conv1(h, no_act=True, residual=self.skip(s, no_act=True))


class SynthesisLayer(nn.Module):
    """affine -> modulated_conv2d (+noise) -> bias_act.  Absent from the reference tree; contract from its call
    sites: ctor kwargs networks.py:2006-2011, forward kwargs :2054-2062, parameter names legacy.py:178-195."""

    def __init__(self, in_channels, out_channels, w_dim, resolution, kernel_size=3, up=1, use_noise=True, activation='lrelu',
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, channels_last=False):
        super().__init__()
        self.resolution, self.up, self.use_noise, self.activation, self.conv_clamp = resolution, up, use_noise, activation, conv_clamp
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        self.padding = kernel_size // 2
        self.act_gain = bias_act.activation_funcs[activation].def_gain
        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)
        memory_format = torch.channels_last if channels_last else torch.contiguous_format
        self.weight = nn.Parameter(torch.randn([out_channels, in_channels, kernel_size, kernel_size]).to(memory_format=memory_format))
        if use_noise:
            self.register_buffer('noise_const', torch.randn([resolution, resolution]))
            self.noise_strength = nn.Parameter(torch.zeros([]))
        self.bias = nn.Parameter(torch.zeros([out_channels]))
        self._cache = _PackCache()

    def forward(self, x, w, noise_mode='random', fused_modconv=True, gain=1, styles=None):
        assert noise_mode in ['random', 'const', 'none']
        in_res = self.resolution // self.up
        misc.assert_shape(x, [None, self.weight.shape[1], in_res, in_res])
        if styles is None:              # (private `styles`: the affine output computed by the caller, SynthesisStack.all_styles)
            styles = self.affine(w)
        noise = None
        if self.use_noise and noise_mode == 'random':
            noise = torch.randn([x.shape[0], 1, self.resolution, self.resolution], device=x.device) * self.noise_strength
        if self.use_noise and noise_mode == 'const':
            if torch.is_grad_enabled() and self.noise_strength.requires_grad:
                noise = self.noise_const * self.noise_strength
            else:       # inference: the product only changes with its operands
                noise = self._cache.get(('noise',), [self.noise_const, self.noise_strength], lambda: (self.noise_const * self.noise_strength).detach())
        act_gain = self.act_gain * gain
        act_clamp = self.conv_clamp * gain if self.conv_clamp is not None else None
        fusable = (_fast_ok(x, self.weight, self.bias, styles, noise) or _fast16_ok(x, self.weight, self.bias, styles, noise)
                   or (self.up == 1 and _train_fused_ok(x, self.weight, styles, noise, self.padding))
                   or (self.up == 2 and _train_fused_up2_ok(x, self.weight, styles, noise, self.padding, self.resample_filter)))
        if fusable and self.activation in conv2d_mfma.FUSED_ACTS:
            ep = dict(bias=self.bias, act=self.activation, alpha=bias_act.activation_funcs[self.activation].def_alpha, gain=act_gain, clamp=act_clamp)
            return modulated_conv2d(x=x, weight=self.weight, styles=styles, noise=noise, up=self.up, padding=self.padding,
                                    resample_filter=self.resample_filter, flip_weight=(self.up == 1), fused_modconv=fused_modconv,
                                    _cache=self._cache, _epilogue=ep)
        x = modulated_conv2d(x=x, weight=self.weight, styles=styles, noise=noise, up=self.up, padding=self.padding,
                             resample_filter=self.resample_filter, flip_weight=(self.up == 1), fused_modconv=fused_modconv)
        return bias_act.bias_act(x, self.bias.to(x.dtype), act=self.activation, gain=act_gain, clamp=act_clamp)




def _is_1331(f):
    """True for the FIR taps setup_filter([1, 3, 3, 1]) produces (2-D, normalised): decided once per filter tensor, on the host.  The verdict is kept ON the
    tensor object with the version it was taken at (an (address, version, shape) key could outlive the tensor and answer for another one)."""
    hit = getattr(f, '_pg_is_1331', None)
    if hit is None or hit[0] != f._version:
        ref = torch.tensor([1.0, 3.0, 3.0, 1.0])
        ref = torch.outer(ref, ref) / 64.0
        hit = (f._version, bool(f.ndim == 2 and tuple(f.shape) == (4, 4) and torch.equal(f.detach().float().cpu(), ref)))
        f._pg_is_1331 = hit
    return hit[1]


class _ToRGBBase(nn.Module):
    PARSING_CHANNELS = 7

    def __init__(self, in_channels, out_channels, w_dim, kernel_size=1, conv_clamp=None, channels_last=False, is_last=False, is_style=False):
        super().__init__()
        self.conv_clamp = conv_clamp
        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)
        memory_format = torch.channels_last if channels_last else torch.contiguous_format
        self.weight = nn.Parameter(torch.randn([out_channels, in_channels, kernel_size, kernel_size]).to(memory_format=memory_format))
        self.bias = nn.Parameter(torch.zeros([out_channels]))
        self.weight_gain = 1 / np.sqrt(in_channels * (kernel_size ** 2))
        self.is_last, self.is_style = is_last, is_style
        if self.is_last and self.is_style:
            self.m_weight1 = nn.Parameter(torch.randn([self.PARSING_CHANNELS, in_channels, kernel_size, kernel_size]).to(memory_format=memory_format))
            self.m_bias1 = nn.Parameter(torch.zeros([self.PARSING_CHANNELS]))
        self._cache, self._cache_p = _PackCache(), _PackCache()

    def forward(self, x, w, fused_modconv=True, skip_img=None, styles=None, skip_up2_filter=None):
        """Returns (rgb, pred_parsing); `skip_img` (private) is added to rgb inside the same launch; `styles` (private) =
        affine(w) * weight_gain computed by the caller; `skip_up2_filter` (private): `skip_img` is the HALF-resolution image and
        upfirdn2d.upsample2d(skip_img, skip_up2_filter) is what has to be added (networks.py:2165-2167)."""
        if styles is None:
            styles = self.affine(w) * self.weight_gain
        if _fast16_ok(x, self.weight, self.bias, styles, skip_img) and self.weight.shape[2:] == (1, 1):
            # half-precision inference: each head is one streaming pass (float32 image out, skip image added in it -- up-sampled in it when it is the
            # usual [1, 3, 3, 1] filter: the skip image's own FIR launch disappears)
            up2 = False
            if skip_up2_filter is not None and skip_img is not None:
                if _is_1331(skip_up2_filter) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and skip_img.dtype == torch.float32 and os.environ.get('PG_HEAD16_UP2', '1') != '0':
                    up2 = True
                else:
                    skip_img = upfirdn2d.upsample2d(skip_img, skip_up2_filter)
            pred_parsing = None
            if self.is_last and self.is_style:
                pred_parsing = conv2d_mfma16.conv1x1_small(x, self.m_weight1, styles, self.m_bias1, clamp=self.conv_clamp)
            return conv2d_mfma16.conv1x1_small(x, self.weight, styles, self.bias, skip=skip_img, clamp=self.conv_clamp, skip_up2=up2), pred_parsing
        if skip_up2_filter is not None and skip_img is not None:
            skip_img = upfirdn2d.upsample2d(skip_img, skip_up2_filter)
        fast = _fast_ok(x, self.weight, self.bias, styles, skip_img)
        if fast and conv2d_mfma.conv1x1_small_ok(x, self.weight, skip_img) and os.environ.get('PG_HEAD_STREAM', '1') != '0':
            # fp32 inference: each head is one streaming pass over x (HBM-bound; the MFMA kernel would pad it to 32 output channels)
            pred_parsing = None
            if self.is_last and self.is_style:
                pred_parsing = conv2d_mfma.conv1x1_small(x, self.m_weight1, styles, self.m_bias1, clamp=self.conv_clamp)
            return conv2d_mfma.conv1x1_small(x, self.weight, styles, self.bias, skip=skip_img, clamp=self.conv_clamp), pred_parsing
        pred_parsing = None
        if self.is_last and self.is_style:
            if fast:
                pred_parsing = modulated_conv2d(x=x, weight=self.m_weight1, styles=styles, demodulate=False, fused_modconv=fused_modconv,
                                                _cache=self._cache_p, _epilogue=dict(bias=self.m_bias1, clamp=self.conv_clamp))
            elif _train_fused_ok(x, self.m_weight1, styles, None, 0):
                pred_parsing = modulated_conv2d(x=x, weight=self.m_weight1, styles=styles, demodulate=False, fused_modconv=fused_modconv,
                                                _epilogue=dict(bias=self.m_bias1, clamp=self.conv_clamp))
            else:
                pred_parsing = modulated_conv2d(x=x, weight=self.m_weight1, styles=styles, demodulate=False, fused_modconv=fused_modconv)
                pred_parsing = bias_act.bias_act(pred_parsing, self.m_bias1.to(x.dtype), clamp=self.conv_clamp)
        if fast:
            y = modulated_conv2d(x=x, weight=self.weight, styles=styles, demodulate=False, fused_modconv=fused_modconv,
                                 _cache=self._cache, _epilogue=dict(bias=self.bias, clamp=self.conv_clamp, residual=skip_img))
            return y, pred_parsing
        if _train_fused_ok(x, self.weight, styles, None, 0):     # training route: bias + clamp inside the launch
            y = modulated_conv2d(x=x, weight=self.weight, styles=styles, demodulate=False, fused_modconv=fused_modconv,
                                 _epilogue=dict(bias=self.bias, clamp=self.conv_clamp))
        else:
            y = modulated_conv2d(x=x, weight=self.weight, styles=styles, demodulate=False, fused_modconv=fused_modconv)
            y = bias_act.bias_act(y, self.bias.to(x.dtype), clamp=self.conv_clamp)
        if skip_img is not None:
            y = skip_img + y
        return y, pred_parsing


class ToRGBLayerFull_v1_v5(_ToRGBBase):
    PARSING_CHANNELS = 7


class ToRGBLayerFull_v1_v4(_ToRGBBase):
    PARSING_CHANNELS = 6


class _SynthesisBlockBase(nn.Module):
    """One resolution of the generator (reference networks.py:2086-2194 / 1971-2082): [conv0 up=2] -> conv1 ->
    [merge_conv with the warped-garment features] -> [parsing-conditioned SPADE block] -> skip image += ToRGB.
    Constructor arguments, sub-module names and creation order follow the reference (checkpoint contract)."""
    TORGB = ToRGBLayerFull_v1_v5
    TEXTURE = False

    def __init__(self, in_channels, out_channels, w_dim, resolution, img_channels, is_last, is_style=False, architecture='skip',
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, use_fp16=False, fp16_channels_last=False, **layer_kwargs):
        assert architecture in ['orig', 'skip', 'resnet']
        super().__init__()
        self.in_channels, self.w_dim, self.resolution, self.img_channels = in_channels, w_dim, resolution, img_channels
        self.is_last, self.architecture, self.use_fp16 = is_last, architecture, use_fp16
        self.channels_last = (use_fp16 and fp16_channels_last)
        self.half_dtype = None          # SynthesisNetworkFull_v18.set_half: the 16-bit type of this block's inference forward (channels-last), None = float32
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        first = in_channels == 0
        layer = dict(w_dim=w_dim, resolution=resolution, conv_clamp=conv_clamp, channels_last=self.channels_last, **layer_kwargs)
        if first:
            self.const = nn.Parameter(torch.randn([out_channels, resolution, resolution]))   # checkpoint parity only: the pose feature replaces it
        else:
            self.conv0 = SynthesisLayer(in_channels, out_channels, up=2, resample_filter=resample_filter, **layer)
        self.conv1 = SynthesisLayer(out_channels, out_channels, **layer)
        self.num_conv = 1 if first else 2
        self.has_torgb = is_last or architecture == 'skip'
        self.num_torgb = int(self.has_torgb)
        if self.has_torgb:
            self.torgb = self.TORGB(out_channels, img_channels, w_dim=w_dim, conv_clamp=conv_clamp, channels_last=self.channels_last,
                                    is_last=is_last, is_style=is_style)
        if not first and architecture == 'resnet':
            self.skip = Conv2dLayer(in_channels, out_channels, kernel_size=1, bias=False, up=2, resample_filter=resample_filter, channels_last=self.channels_last)
        if resolution > 32:
            self.merge_conv = Conv2dLayer(out_channels + 64, out_channels, kernel_size=1, resample_filter=resample_filter, channels_last=self.channels_last)
        if self.TEXTURE:
            self.spade_b512 = Spade_ResBlockV4_512(out_channels, out_channels, spade_channels=1)
        self._fold_cache = _PackCache()

    def affine_layers(self):
        """(layer, index of its w within the block's ws, gain folded into its styles) in call order."""
        convs = [self.conv1] if self.in_channels == 0 else [self.conv0, self.conv1]
        return [(m, i, 1.0) for i, m in enumerate(convs)] + ([(self.torgb, self.num_conv, self.torgb.weight_gain)] if self.has_torgb else [])

    def _heads_folded(self, x, feat, w, styles, img):
        """fp32 inference, style blocks: merge_conv (linear, bias, no clamp) and the ToRGB heads behind it are one linear map of (x, feat) per sample,
        head([x ; feat]) = (W_head o s_n) (g W_m [x ; feat] + b_m) + b_head; one streaming pass over the two inputs computes the heads without the merged
        feature map (csrc/conv1x1_fold.hip).  Returns (rgb, pred_parsing), or None where the route or the kernel does not cover the call (the caller then
        runs the two layers one after the other).  PG_HEAD_FOLD=0: never (A/B runs)."""
        mc, tr = getattr(self, 'merge_conv', None), getattr(self, 'torgb', None)
        if mc is None or tr is None or self.TEXTURE or self.architecture != 'skip' or os.environ.get('PG_HEAD_FOLD', '1') == '0' or os.environ.get('PG_HEAD_STREAM', '1') == '0':
            return None
        if (mc.conv_clamp is not None or mc.activation != 'linear' or mc.up != 1 or mc.down != 1 or tuple(mc.weight.shape[2:]) != (1, 1)
                or tuple(tr.weight.shape[2:]) != (1, 1) or int(mc.weight.shape[1]) != int(x.shape[1]) + int(feat.shape[1])):
            return None
        parsing = tr.is_last and tr.is_style
        params = [mc.weight, tr.weight, tr.bias] + ([mc.bias] if mc.bias is not None else []) + ([tr.m_weight1, tr.m_bias1] if parsing else [])
        if not (_fast_ok(x, feat, styles, img, tr.affine.weight, tr.affine.bias, *params) and conv2d_mfma.conv1x1_fold_ok(x, feat, img)):
            return None

        def build():
            cm = int(mc.weight.shape[0])
            heads = [(tr.weight, tr.bias)] + ([(tr.m_weight1, tr.m_bias1)] if parsing else [])
            return ((mc.weight.detach().float().reshape(cm, -1) * mc.weight_gain * mc.act_gain).contiguous(),
                    (mc.bias.detach().float() * mc.act_gain).contiguous() if mc.bias is not None else None,
                    torch.cat([hw.detach().float().reshape(hw.shape[0], cm) for hw, _ in heads]).contiguous(),
                    torch.cat([hb.detach().float() for _, hb in heads]).contiguous())
        wm, bm, wh, bh = self._fold_cache.get(('fold',), params, build)
        if styles is None:
            styles = tr.affine(w) * tr.weight_gain
        try:
            wn, bn = conv2d_mfma.conv1x1_fold_prep(wm, bm, wh, bh, styles)
            return conv2d_mfma.conv1x1_fold_heads(x, feat, wn, bn, int(tr.weight.shape[0]), skip=img, clamp=tr.conv_clamp)
        except nat.NativeNotCovered:
            return None

    def _merge_heads(self, x, feat, w, styles, img, fused_modconv, feat_unused=False):
        """merge_conv over [x ; feat], then img + ToRGB (and the parsing head): (x, rgb, pred_parsing).  `feat_unused`: nothing reads the merged feature map
        but the heads -- it is then not computed where `_heads_folded` covers the call, and x comes back as None."""
        if feat_unused:
            heads = self._heads_folded(x, feat, w, styles, img)
            if heads is not None:
                return (None,) + tuple(heads)
        x = self.merge_conv(x, x2=feat)
        rgb, pred_parsing = self.torgb(x, w, fused_modconv=fused_modconv, skip_img=img, styles=styles)
        return x, rgb, pred_parsing

    def _tail_fold_ok(self):
        """The layer properties under which the texture block's tail folds into its ToRGB head (`_tail_folded`): spade_b512 ends with a bias-free 3x3
        (padding 1) plus a bias-free 1x1, both without resampling, and the only head is a 1x1 ToRGB.  PG_TEX_FOLD=0: never (A/B runs)."""
        sb, tr = getattr(self, 'spade_b512', None), getattr(self, 'torgb', None)
        if sb is None or tr is None or not self.TEXTURE or torch.is_grad_enabled() or os.environ.get('PG_TEX_FOLD', '1') == '0':
            return False
        c1, sk = sb.conv1, sb.skip
        cm = int(tr.weight.shape[1])
        return (all(l.bias is None and l.up == 1 and l.down == 1 and int(l.weight.shape[0]) == cm for l in (c1, sk))
                and tuple(c1.weight.shape[2:]) == (3, 3) and c1.padding == 1 and tuple(sk.weight.shape[2:]) == (1, 1) and sk.padding == 0
                and c1.weight.shape[1] == sk.weight.shape[1] and tuple(tr.weight.shape[2:]) == (1, 1) and not (tr.is_last and tr.is_style))

    def _tail_folded(self, h, s, w, styles, img):
        """fp32 inference, texture block: the tail of spade_b512, conv1(h') + skip(s') (both linear and bias-free, so zero padding stays exact), and the ToRGB
        head behind it are one linear map of (h', s') per sample with 3 x C x 9 + 3 x C weights; one streaming pass over h' and s' computes the image without
        the block's feature map (csrc/conv3x3_fold.hip).  Returns rgb, or None where the kernel does not cover the call (the caller then runs the layers one
        after the other)."""
        sb, tr = self.spade_b512, self.torgb
        c1, sk = sb.conv1, sb.skip
        params = [c1.weight, sk.weight, tr.weight, tr.bias]
        if not (_fast_ok(h, s, styles, img, tr.affine.weight, tr.affine.bias, *params) and conv2d_mfma.conv3x3_fold_ok(h, s, img)):
            return None

        def build():
            cm = int(c1.weight.shape[0])
            return (torch.cat([(c1.weight.detach().float() * c1.weight_gain).reshape(cm, -1), (sk.weight.detach().float() * sk.weight_gain).reshape(cm, -1)], dim=1).contiguous(),
                    tr.weight.detach().float().reshape(tr.weight.shape[0], cm).contiguous(), tr.bias.detach().float().contiguous())
        wm, wh, bh = self._fold_cache.get(('tail',), params, build)
        if styles is None:
            styles = tr.affine(w) * tr.weight_gain
        try:
            wn, bn = conv2d_mfma.conv1x1_fold_prep(wm, None, wh, bh, styles)
            return conv2d_mfma.conv3x3_fold_head(h, s, wn, bn, skip=img, clamp=tr.conv_clamp)
        except nat.NativeNotCovered:
            return None

    def _spade_heads(self, x, parsing, w, styles, img, fused_modconv, feat_unused=False):
        """spade_b512 over x, then img + ToRGB: (x, rgb, pred_parsing).  `feat_unused`: nothing reads the SPADE block's result but the head -- its tail is
        then not computed where `_tail_folded` covers the call, and x comes back as None."""
        x = self.spade_b512(x, parsing, _defer_tail=feat_unused and self._tail_fold_ok())
        if isinstance(x, tuple):
            rgb = self._tail_folded(*x, w, styles, img)
            if rgb is not None:
                return None, rgb, None
            x = self.spade_b512.tail(*x)
        rgb, pred_parsing = self.torgb(x, w, fused_modconv=fused_modconv, skip_img=img, styles=styles)
        return x, rgb, pred_parsing

    def _forward(self, x, img, ws, pose_feature, cat_feat, parsing, force_fp32, fused_modconv, styles=None, _feat_unused=False, **layer_kwargs):
        """`styles` (private): the block's affine outputs in `affine_layers()` order when the network computed them for all layers at once.
        `_feat_unused` (private): the caller does not read the returned feature map (the network's last style block, the texture block); it may come back
        as None."""
        misc.assert_shape(ws, [None, self.num_conv + self.num_torgb, self.w_dim])
        half = (self.use_fp16 or self.half_dtype is not None) and not force_fp32
        fmt = dict(dtype=(self.half_dtype or torch.float16) if half else torch.float32,
                   memory_format=torch.channels_last if ((self.channels_last or self.half_dtype is not None) and not force_fp32) else torch.contiguous_format)
        if fused_modconv is None:      # the reference's rule (networks.py:2152-2154); both forms are one launch here
            fused_modconv = (not self.training) and (not half or int(ws.shape[0]) == 1)
        style = lambda i: ws[:, i]
        st = styles if styles is not None else [None] * (self.num_conv + self.num_torgb)
        conv = lambda layer, t, i, **kw: layer(t, style(i), fused_modconv=fused_modconv, styles=st[i], **kw, **layer_kwargs)

        if self.in_channels == 0:      # 8x8 block: starts from the pose encoder's feature map
            x = conv(self.conv1, pose_feature.to(**fmt), 0)
        else:
            misc.assert_shape(x, [None, self.in_channels, self.resolution // 2, self.resolution // 2])
            x = x.to(**fmt)
            if self.architecture == 'resnet':
                shortcut = self.skip(x, gain=SQRT_HALF)
                x = conv(self.conv1, conv(self.conv0, x, 0), 1, gain=SQRT_HALF)
                x = shortcut.add_(x)
            else:
                x = conv(self.conv1, conv(self.conv0, x, 0), 1)
                if self.resolution > 32:   # mix in the warped-garment feature map: conv1x1(cat([x, feat])) without the copy
                    feat = cat_feat[str(self.resolution)].to(**fmt)
                    if _feat_unused and self.has_torgb and not self.TEXTURE and not half:
                        # the merged map feeds only the heads: they are computed from (x, feat) directly where the folded kernel covers the call
                        if img is not None:
                            misc.assert_shape(img, [None, self.img_channels, self.resolution // 2, self.resolution // 2])
                            img = upfirdn2d.upsample2d(img, self.resample_filter)
                        x, rgb, pred_parsing = self._merge_heads(x, feat, style(self.num_conv), st[self.num_conv], img, fused_modconv, feat_unused=True)
                        return x, rgb.to(dtype=torch.float32, memory_format=torch.contiguous_format), pred_parsing
                    x = self.merge_conv(x, x2=feat)
                if self.TEXTURE:
                    if _feat_unused and self.has_torgb and not half:
                        # the SPADE block's result feeds only the image head: the head is computed from the block's two last SPADE outputs directly where
                        # the folded kernel covers the call
                        if img is not None:
                            misc.assert_shape(img, [None, self.img_channels, self.resolution // 2, self.resolution // 2])
                            img = upfirdn2d.upsample2d(img, self.resample_filter)
                        x, rgb, pred_parsing = self._spade_heads(x, parsing, style(self.num_conv), st[self.num_conv], img, fused_modconv, feat_unused=True)
                        return x, rgb.to(dtype=torch.float32, memory_format=torch.contiguous_format), pred_parsing
                    x = self.spade_b512(x, parsing)

        if img is not None:
            misc.assert_shape(img, [None, self.img_channels, self.resolution // 2, self.resolution // 2])
            img = upfirdn2d.upsample2d(img, self.resample_filter)
        pred_parsing = None
        if self.has_torgb:             # img + torgb(x) in one launch
            rgb, pred_parsing = self.torgb(x, style(self.num_conv), fused_modconv=fused_modconv, skip_img=img, styles=st[self.num_conv])
            img = rgb.to(dtype=torch.float32, memory_format=torch.contiguous_format)
        return x, img, pred_parsing


class SynthesisBlockFull_v1_v6(_SynthesisBlockBase):
    """Style-branch block (networks.py:2086-2194)."""
    TORGB = ToRGBLayerFull_v1_v5

    def forward(self, x, img, ws, pose_feature, cat_feat, force_fp32=False, fused_modconv=None, styles=None, _feat_unused=False, **layer_kwargs):
        return self._forward(x, img, ws, pose_feature, cat_feat, None, force_fp32, fused_modconv, styles=styles, _feat_unused=_feat_unused, **layer_kwargs)


class SynthesisBlockFull_v1_v4(_SynthesisBlockBase):
    """Texture-branch block with the parsing-conditioned SPADE residual block (networks.py:1971-2082)."""
    TORGB = ToRGBLayerFull_v1_v4
    TEXTURE = True

    def forward(self, x, img, ws, pose_feature, cat_feat, parsing, force_fp32=False, fused_modconv=None, styles=None, _feat_unused=False, **layer_kwargs):
        return self._forward(x, img, ws, pose_feature, cat_feat, parsing, force_fp32, fused_modconv, styles=styles, _feat_unused=_feat_unused, **layer_kwargs)


def _half_nearest(t):
    """F.interpolate(t, scale_factor=0.5), default 'nearest' (networks.py:2255-2256, 2311-2312): every other pixel."""
    return t[:, :, ::2, ::2]


def _batched_affine(owner, entries, ws, num_ws, w_dim):
    """Inference: the ~2 dozen affine layers of a synthesis network (FullyConnectedLayer, networks.py:115-128: w @ (W * gain)^T + b) as ONE GEMM over all
    (w index, layer) pairs -- mostly unused products, a fraction of a GFLOP -- instead of a launch per layer, and one gather that leaves each layer's
    [N, Cin] styles contiguous.  entries: (key, layer, absolute w index, gain folded into the styles); weights are concatenated once per parameter version.
    Returns {key: [styles, ...]} in entry order."""
    n = ws.shape[0]
    params = [t for _, m, _, _ in entries for t in (m.affine.weight, m.affine.bias)]

    def build():
        wt = torch.cat([m.affine.weight.detach().float() * (m.affine.weight_gain * g) for _, m, _, g in entries]).t().contiguous()
        b = torch.cat([m.affine.bias.detach().float() * (m.affine.bias_gain * g) for _, m, _, g in entries]).contiguous()
        return wt, b
    if not hasattr(owner, '_affine_cache'):
        owner._affine_cache, owner._gather = _PackCache(), {}
    wt, b = owner._affine_cache.get(('all',), params, build)
    total = wt.shape[1]
    key = (n, ws.device)
    if key not in owner._gather:     # flat index of styles[l][n, c] inside the [N * num_ws, total] product
        idx, col = [], 0
        rows = torch.arange(n, dtype=torch.int64)[:, None] * num_ws
        for _, m, wi, _ in entries:
            c = m.affine.weight.shape[0]
            idx.append(((rows + wi) * total + col + torch.arange(c, dtype=torch.int64)[None, :]).reshape(-1))
            col += c
        owner._gather[key] = torch.cat(idx).to(ws.device)
    flat = torch.addmm(b, ws.reshape(n * num_ws, w_dim), wt).reshape(-1).index_select(0, owner._gather[key])
    out, off = {}, 0
    for k, m, _, _ in entries:
        c = m.affine.weight.shape[0]
        out.setdefault(k, []).append(flat[off:off + n * c].view(n, c))
        off += n * c
    return out


class SynthesisNetworkFull_v18(nn.Module):
    """The 512^2 try-on generator body (reference networks.py:2198-2327): style branch b8..b512, garment-feature encoder,
    two SPADE blocks at 256^2 and the texture block at 512^2.  float32 throughout, like the reference (:2223, :2294), unless `set_half` switches the
    inference forward of the high-resolution blocks to bf16 / fp16."""

    def __init__(self, w_dim, img_resolution, img_channels, channel_base=32768, channel_max=512, num_fp16_res=0, **block_kwargs):
        assert img_resolution >= 8 and img_resolution & (img_resolution - 1) == 0
        super().__init__()
        self.w_dim, self.img_resolution, self.img_channels = w_dim, img_resolution, img_channels
        self.img_resolution_log2 = int(np.log2(img_resolution))
        self.block_resolutions = [1 << e for e in range(3, self.img_resolution_log2 + 1)]
        width = lambda res: min(channel_base // res, channel_max)
        common = dict(w_dim=w_dim, img_channels=img_channels, use_fp16=False, **block_kwargs)
        self.num_ws = 0
        for res in self.block_resolutions:
            last = res == img_resolution
            block = SynthesisBlockFull_v1_v6(width(res // 2) if res > 8 else 0, width(res), resolution=res, is_last=last, is_style=True, **common)
            setattr(self, f'b{res}', block)
            self.num_ws += block.num_conv + (block.num_torgb if last else 0)
        mid, top = self.block_resolutions[-2], self.block_resolutions[-1]
        self.spade_b256_1 = Spade_ResBlockV4_512(width(mid), width(mid), spade_channels=128)
        self.spade_b256_2 = Spade_ResBlockV4_512(width(mid), width(mid), spade_channels=128)
        self.texture_b512 = SynthesisBlockFull_v1_v4(width(mid), width(top), resolution=top, is_last=True, is_style=False, **common)
        ngf = 64
        self.spade_encoder = nn.Sequential(
            Conv2dLayer(3, ngf, kernel_size=7, activation='relu'),
            ResBlock(ngf, ngf, kernel_size=4, activation='relu'),                 # 512
            ResBlock(ngf, ngf * 2, kernel_size=4, activation='relu', down=2),     # 256
        )
        self.half_dtype, self.half_from_res = None, 64

    def set_half(self, dtype, from_res=64):
        """Opt-in 16-bit inference: run the blocks at resolution >= `from_res` -- the style blocks, the two SPADE blocks at the second-highest resolution and
        the texture block with its SPADE block -- in `dtype` (torch.bfloat16 | torch.float16), channels-last, on the 16-bit kernels; None restores the float32
        route exactly.  A plain attribute switch (no parameter is touched: call it after loading a checkpoint); `num_fp16_res` stays ignored.  Mapping, both
        encoders, the garment-feature encoder and assembly, the blocks below `from_res`, the running skip image, `pred_parsing` and both returned images stay
        float32.  The 16-bit route is inference on the GPU only: with autograd enabled, in training mode or on CPU tensors the blocks run their float32 code
        (on a CPU network `set_half` changes nothing in the arithmetic).  Returns self."""
        if dtype is not None and dtype not in conv2d_mfma16.DTYPES:
            raise ValueError(f'set_half: dtype must be None, torch.bfloat16 or torch.float16, not {dtype!r}')
        if dtype is not None:
            narrow = [res for res in self.block_resolutions if res >= int(from_res) and any(int(c) % 16 for c in (getattr(self, f'b{res}').in_channels, getattr(self, f'b{res}').conv1.weight.shape[0]))]
            if narrow:
                raise ValueError(f'set_half: the 16-bit kernels need channel counts that are multiples of 16; the blocks at {narrow} have narrower layers')
        self.half_dtype, self.half_from_res = dtype, int(from_res)
        for res in self.block_resolutions:
            getattr(self, f'b{res}').half_dtype = dtype if res >= int(from_res) else None
        self.texture_b512.half_dtype = dtype if self.block_resolutions[-1] >= int(from_res) else None
        return self

    def _half_on(self, block, ws):
        """This call runs `block` in its 16-bit type: inference (no autograd, eval mode) on GPU tensors."""
        return block.half_dtype is not None and ws.is_cuda and not torch.is_grad_enabled() and not self.training

    def get_spade_feat(self, mask_512, denorm_mask, denorm_input):
        """Garment features of one branch (reference :2253-2276): encode the warped garment inside the predicted region,
        then fill the part of that region the warp did not cover with the mean feature of the part it did cover."""
        region = mask_512 > 0.9
        region_256 = _half_nearest(region)
        covered = region_256 & (_half_nearest(denorm_mask) > 0.9)
        hole = (region_256 & ~covered).to(denorm_input.dtype)
        feat = self.spade_encoder(torch.where(region, denorm_input, -1.0))
        covered = covered.to(feat.dtype)
        count = covered.sum(dim=(2, 3), keepdim=True)
        count = torch.where(count > 10, count, 256.0 * 256.0)
        mean = (feat * covered).sum(dim=(2, 3), keepdim=True) / count
        return feat * (1 - hole) + mean * hole

    def _block_styles(self, ws):
        """The slice of `ws` each style block consumes: its own convolutions plus the ToRGB that shares the next block's
        first style vector (reference :2281-2289)."""
        misc.assert_shape(ws, [None, self.num_ws, self.w_dim])
        ws = ws.to(torch.float32)
        out, start = [], 0
        for res in self.block_resolutions:
            block = getattr(self, f'b{res}')
            out.append(ws[:, start:start + block.num_conv + block.num_torgb])
            start += block.num_conv
        return out

    def forward(self, ws, pose_feat, cat_feat, denorm_upper_input, denorm_lower_input, denorm_upper_mask,
                denorm_lower_mask, gt_parsing, **block_kwargs):
        styles = self._block_styles(ws)
        # inference on the GPU: the 23 affine layers of the style and texture branches as one GEMM + one gather (round 5; PG_AFFINE_BATCHED=0 = a launch per layer)
        pre = None
        if ws.is_cuda and not torch.is_grad_enabled() and os.environ.get('PG_AFFINE_BATCHED', '1') != '0':
            entries, start = [], 0
            for res in self.block_resolutions:
                block = getattr(self, f'b{res}')
                entries += [(res, m, start + i, g) for m, i, g in block.affine_layers()]
                last_start, start = start, start + block.num_conv
            entries += [('texture', m, last_start + i, g) for m, i, g in self.texture_b512.affine_layers()]
            pre = _batched_affine(self, entries, ws.to(torch.float32), self.num_ws, self.w_dim)
            if os.environ.get('PG_PREP_BATCHED', '1') != '0':
                # ... and the demodulation coefficients of the 15 modulated 3x3 convolutions (networks.py:64-68) as ONE launch instead of one ~6 us launch (+ its
                # launch gap) per layer: each layer's own `modconv_prep` call finds its result waiting (round 5; the 16-bit stack has done this since round 4)
                jobs, seen = [], {}
                for key, m, _, _ in entries:
                    j = seen.get(key, 0)
                    seen[key] = j + 1
                    if isinstance(m, SynthesisLayer) and getattr(m, '_cache', None) is not None:
                        w2 = m._cache.get(('w2',), [m.weight], lambda m=m: conv2d_mfma.modconv_w2(m.weight))
                        jobs.append((w2, pre[key][j], int(m.weight.shape[0]), False, True))
                if 0 < len(jobs) <= conv2d_mfma.PREP_MAX_JOBS:
                    conv2d_mfma.modconv_prep_batched(jobs)
        try:
            return self._forward_body(ws, styles, pre, pose_feat, cat_feat, denorm_upper_input, denorm_lower_input, denorm_upper_mask, denorm_lower_mask, gt_parsing, block_kwargs)
        finally:
            if pre is not None:
                conv2d_mfma.modconv_prep_clear()

    def _forward_body(self, ws, styles, pre, pose_feat, cat_feat, denorm_upper_input, denorm_lower_input, denorm_upper_mask, denorm_lower_mask, gt_parsing, block_kwargs):
        x = img = pred_parsing = None
        kept = {}
        for res, w in zip(self.block_resolutions, styles):
            # (the last style block's feature map is read by nobody -- the texture branch starts from kept[256] --: the block may fold its merge_conv into its heads)
            block = getattr(self, f'b{res}')
            x, img, pred_parsing = block(x, img, w, pose_feat, cat_feat, force_fp32=not self._half_on(block, ws), styles=pre[res] if pre is not None else None,
                                         _feat_unused=(res == self.block_resolutions[-1]), **block_kwargs)
            kept[res] = (x, img)       # neither is modified in place afterwards: no clone needed
        x_256, img_256 = kept[self.block_resolutions[-2]]

        if gt_parsing is not None:
            parsing_index = gt_parsing
        else:   # softmax is monotone per pixel: argmax(softmax(p)) == argmax(p) (reference :2301-2302)
            parsing_index = pred_parsing.detach().argmax(dim=1, keepdim=True).float()
        upper_mask = ((parsing_index == 1) | (parsing_index == 4)).float()
        lower_mask = ((parsing_index == 2) | (parsing_index == 3)).float()

        if _fast_ok(x_256, denorm_upper_input, denorm_lower_input, denorm_upper_mask, denorm_lower_mask) and denorm_upper_mask.dtype == torch.float32:
            # inference route: encoder inputs as in get_spade_feat, then the inpainting + merge of both branches in three launches
            feat_u = self.spade_encoder(torch.where(upper_mask > 0.9, denorm_upper_input, -1.0))
            feat_l = self.spade_encoder(torch.where(lower_mask > 0.9, denorm_lower_input, -1.0))
            spade_feat = conv2d_mfma.spade_feat_assemble(feat_u, feat_l, upper_mask, lower_mask, denorm_upper_mask, denorm_lower_mask)
        else:
            spade_feat = (self.get_spade_feat(upper_mask.detach(), denorm_upper_mask, denorm_upper_input) * (_half_nearest(upper_mask) > 0.9)
                          + self.get_spade_feat(lower_mask.detach(), denorm_lower_mask, denorm_lower_input) * (_half_nearest(lower_mask) > 0.9))

        if x_256.dtype != torch.float32:       # half mode: the 128-channel garment features are cast once for the six norm blocks that read them
            spade_feat = spade_feat.to(dtype=x_256.dtype, memory_format=torch.channels_last)
        x_spade = self.spade_b256_2(self.spade_b256_1(x_256, spade_feat), spade_feat)
        # (the texture block's feature map is read by nobody: the block may fold the tail of its SPADE block into its image head)
        _, finetune_img, _ = self.texture_b512(x_spade, img_256, styles[-1], pose_feat, cat_feat, parsing_index, force_fp32=not self._half_on(self.texture_b512, ws),
                                               styles=pre['texture'] if pre is not None else None, _feat_unused=True, **block_kwargs)
        return img, finetune_img, pred_parsing


class SynthesisStackBlock(nn.Module):
    """One resolution of the plain StyleGAN2 stack: [conv0 up=2] -> conv1, skip image = upsample2d(img) + ToRGB(x)."""

    def __init__(self, in_channels, out_channels, w_dim, resolution, img_channels, resample_filter=[1, 3, 3, 1], conv_clamp=None,
                 half_dtype=None, **layer_kwargs):
        super().__init__()
        self.in_channels, self.w_dim, self.resolution, self.img_channels, self.half_dtype = in_channels, w_dim, resolution, img_channels, half_dtype
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        layer = dict(w_dim=w_dim, resolution=resolution, conv_clamp=conv_clamp, **layer_kwargs)
        if in_channels == 0:
            self.const = nn.Parameter(torch.randn([out_channels, resolution, resolution]))
        else:
            self.conv0 = SynthesisLayer(in_channels, out_channels, up=2, resample_filter=resample_filter, **layer)
        self.conv1 = SynthesisLayer(out_channels, out_channels, **layer)
        self.torgb = ToRGBLayerFull_v1_v5(out_channels, img_channels, w_dim=w_dim, conv_clamp=conv_clamp)
        self.num_conv = 1 if in_channels == 0 else 2
        self.num_torgb = 1

    def affine_layers(self):
        """(layer, index of its w within the block's ws, gain folded into its styles) in call order."""
        convs = [self.conv1] if self.in_channels == 0 else [self.conv0, self.conv1]
        return [(m, i, 1.0) for i, m in enumerate(convs)] + [(self.torgb, self.num_conv, self.torgb.weight_gain)]

    def forward(self, x, img, ws, force_fp32=False, styles=None, **layer_kwargs):
        misc.assert_shape(ws, [None, self.num_conv + self.num_torgb, self.w_dim])
        half = self.half_dtype is not None and not force_fp32
        fmt = dict(dtype=self.half_dtype if half else torch.float32, memory_format=torch.channels_last if half else torch.contiguous_format)
        st = list(styles) if styles is not None else [None] * (self.num_conv + self.num_torgb)
        if self.in_channels == 0:
            x = self.const.to(fmt['dtype'])[None].expand(ws.shape[0], -1, -1, -1).contiguous(memory_format=fmt['memory_format'])
            x = self.conv1(x, ws[:, 0], styles=st[0], **layer_kwargs)
        else:
            x = self.conv1(self.conv0(x.to(**fmt), ws[:, 0], styles=st[0], **layer_kwargs), ws[:, 1], styles=st[1], **layer_kwargs)
        # img + torgb(x): the half-resolution image is handed over as it is; the head up-samples it in its own pass where it can (16-bit inference)
        rgb, _ = self.torgb(x, ws[:, self.num_conv], skip_img=img, styles=st[self.num_conv], skip_up2_filter=self.resample_filter if img is not None else None)
        return x, rgb.to(dtype=torch.float32, memory_format=torch.contiguous_format)


class SynthesisStack(nn.Module):
    """The StyleGAN2 block stack the PASTA-GAN++ style branch derives from (SynthesisLayer x2 + ToRGB + skip-image upsample per
    resolution; no pose / garment / SPADE inputs), at any power-of-two resolution and with the `num_fp16_res` highest
    resolutions in `half_dtype` (bf16 or fp16) -- BASELINE config 5 runs it at 1024^2 entirely in bf16.  The reference class
    is hard-wired to 512^2 float32, so this is an extension built from the same layers."""

    def __init__(self, w_dim, img_resolution, img_channels=3, channel_base=32768, channel_max=512, num_fp16_res=0, half_dtype=torch.float16,
                 conv_clamp=None, **block_kwargs):
        assert img_resolution >= 8 and img_resolution & (img_resolution - 1) == 0
        super().__init__()
        self.w_dim, self.img_resolution, self.img_channels = w_dim, img_resolution, img_channels
        log2 = int(np.log2(img_resolution))
        self.block_resolutions = [1 << e for e in range(3, log2 + 1)]
        width = lambda res: min(channel_base // res, channel_max)
        half_from = max(1 << (log2 + 1 - num_fp16_res), 8) if num_fp16_res > 0 else (img_resolution * 2)
        self.num_ws = 0
        for res in self.block_resolutions:
            block = SynthesisStackBlock(width(res // 2) if res > 8 else 0, width(res), w_dim=w_dim, resolution=res, img_channels=img_channels,
                                        conv_clamp=conv_clamp, half_dtype=half_dtype if res >= half_from else None, **block_kwargs)
            setattr(self, f'b{res}', block)
            self.num_ws += block.num_conv + (block.num_torgb if res == img_resolution else 0)

    def all_styles(self, ws):
        """Inference: every affine layer of the stack as ONE GEMM + one gather (`_batched_affine`).  Returns {resolution: [styles of conv0?, conv1, torgb]};
        the ToRGB weight gain is folded in."""
        entries, start = [], 0          # (resolution, layer, absolute w index, gain)
        for res in self.block_resolutions:
            block = getattr(self, f'b{res}')
            entries += [(res, m, start + i, g) for m, i, g in block.affine_layers()]
            start += block.num_conv
        return _batched_affine(self, entries, ws, self.num_ws, self.w_dim)

    def forward(self, ws, **block_kwargs):
        misc.assert_shape(ws, [None, self.num_ws, self.w_dim])
        ws = ws.to(torch.float32)
        x = img = None
        start = 0
        styles = self.all_styles(ws) if (ws.is_cuda and not torch.is_grad_enabled() and os.environ.get('PG_AFFINE_BATCHED', '1') != '0') else None
        try:
            if styles is not None and os.environ.get('PG_PREP_BATCHED', '1') != '0':
                self._prepare_all(styles, bool(block_kwargs.get('force_fp32', False)))
            for res in self.block_resolutions:
                block = getattr(self, f'b{res}')
                x, img = block(x, img, ws[:, start:start + block.num_conv + block.num_torgb], styles=styles[res] if styles is not None else None, **block_kwargs)
                start += block.num_conv
        finally:
            conv2d_mfma.modconv_prep_clear()
            conv2d_mfma16.pack_clear()
        return img

    def _prepare_all(self, styles, force_fp32):
        """Inference: the style preparation of every modulated 3x3 convolution of the stack (demodulation coefficients; for the layers that share one
        weight pack also the per-sample normalised styles in 16 bits, networks.py:57-59) as ONE launch instead of one ~8 us launch per layer
        (`pg_modconv_prep_batched`); each layer's own `modconv_prep` call then finds its result waiting.  Each 16-bit layer is prepared for the
        `_modconv16_route` it will take: the route says whether it shares a pack, and `_modconv16_pack_source` what its per-sample pack is built from."""
        jobs, per_sample, half_dtype = [], [], None
        for res in self.block_resolutions:
            block = getattr(self, f'b{res}')
            half = block.half_dtype is not None and not force_fp32
            for k, (m, _, _) in enumerate(block.affine_layers()[:block.num_conv]):
                route = _modconv16_route(m.weight.shape, (res // m.up, res // m.up), m.up, m.padding, m.resample_filter) if half else None
                half_dtype = block.half_dtype if half else half_dtype
                w2 = m._cache.get(('w2',), [m.weight], lambda m=m: conv2d_mfma.modconv_w2(m.weight.detach().float()))
                jobs.append((w2, styles[res][k], int(m.weight.shape[0]), half and route.shared, True))
                # (the batched pack kernel has the 3x3 and 3x2 layouts, not the 2x2 one of the merged-t form)
                if half and not route.shared and route.form != R16_MERGED_T and tuple(m.weight.shape[2:]) == (3, 3) and m.weight.dtype == torch.float32:
                    per_sample.append((m, styles[res][k], route))
        if not (jobs and len(jobs) <= conv2d_mfma.PREP_MAX_JOBS and len({j[1].shape[0] for j in jobs}) == 1):
            return
        conv2d_mfma.modconv_prep_batched(jobs, half_dtype=half_dtype)
        if half_dtype is None or os.environ.get('PG_PACK_BATCHED', '1') == '0':
            return
        # ... and the per-sample weight packs of the layers that run on one pack of their own (T(w * styles * dcoefs), networks.py:85-94), also one launch: each
        # layer's `pack_lookup` finds its pack waiting.  The demodulation coefficients are the ones the launch above is producing (same stream: ordered).
        packs = []
        for m, s, route in per_sample:
            dcoefs = conv2d_mfma.modconv_prep_peek(s)
            src = _modconv16_pack_source(m._cache, m.weight, m.up == 1, m.resample_filter, route) if dcoefs is not None else None       # (flip_weight as SynthesisLayer.forward passes it)
            if src is not None:
                packs.append((src.w, src.flip, src.transpose_oi, s, dcoefs))
        if 0 < len(packs) <= conv2d_mfma16.PACK_MAX_JOBS:
            conv2d_mfma16.pack_weight_batched(packs, half_dtype)


# ============================================================================
# Upstream of synthesis in test.py:151-153 / loss_fullbody.py:75-98: the pose ("const")
# encoder, the garment-part style encoder with its 4-scale feature pyramid, the mapping MLP and the full generator.
# They are built from the same ops, so every convolution below is the MFMA kernel with its bias/activation folded in.

class MappingNetwork(nn.Module):
    """Latent / condition -> per-layer style vectors (reference networks.py:184-259).  PASTA-GAN++ runs it with z_dim=0,
    c_dim=512 (the garment style code) and one layer."""

    def __init__(self, z_dim, c_dim, w_dim, num_ws, num_layers=8, embed_features=None, layer_features=None,
                 activation='lrelu', lr_multiplier=0.01, w_avg_beta=0.995):
        super().__init__()
        self.z_dim, self.c_dim, self.w_dim, self.num_ws, self.num_layers, self.w_avg_beta = z_dim, c_dim, w_dim, num_ws, num_layers, w_avg_beta
        embed = 0 if c_dim == 0 else (w_dim if embed_features is None else embed_features)
        hidden = w_dim if layer_features is None else layer_features
        widths = [z_dim + embed] + [hidden] * (num_layers - 1) + [w_dim]
        if c_dim > 0:
            self.embed = FullyConnectedLayer(c_dim, embed)
        for i, (fan_in, fan_out) in enumerate(zip(widths[:-1], widths[1:])):
            setattr(self, f'fc{i}', FullyConnectedLayer(fan_in, fan_out, activation=activation, lr_multiplier=lr_multiplier))
        if num_ws is not None and w_avg_beta is not None:
            self.register_buffer('w_avg', torch.zeros([w_dim]))

    def _inputs(self, z, c):
        parts = []
        if self.z_dim > 0:
            misc.assert_shape(z, [None, self.z_dim])
            parts.append(normalize_2nd_moment(z.to(torch.float32)))
        if self.c_dim > 0:
            misc.assert_shape(c, [None, self.c_dim])
            parts.append(normalize_2nd_moment(self.embed(c.to(torch.float32))))
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)

    def forward(self, z, c, truncation_psi=1, truncation_cutoff=None, skip_w_avg_update=False):
        w = self._inputs(z, c)
        for i in range(self.num_layers):
            w = getattr(self, f'fc{i}')(w)
        track = self.w_avg_beta is not None and self.training and not skip_w_avg_update
        if track:       # running mean of w, the truncation anchor
            self.w_avg.copy_(torch.lerp(w.detach().mean(dim=0), self.w_avg, self.w_avg_beta))
        if self.num_ws is not None:
            w = w[:, None, :].repeat(1, self.num_ws, 1)
        if truncation_psi != 1:
            assert self.w_avg_beta is not None
            if self.num_ws is None or truncation_cutoff is None:
                w = torch.lerp(self.w_avg, w, truncation_psi)
            else:
                head = w[:, :truncation_cutoff]
                head.copy_(torch.lerp(self.w_avg, head, truncation_psi))
        return w


class ConstEncoderNetwork(nn.Module):
    """reference networks.py:357-375: pose map [N,5,512,512] -> [N,512,8,8]."""

    def __init__(self, input_nc, output_nc, ngf=64, n_downsampling=4):
        super().__init__()
        encoder = [Conv2dLayer(input_nc, ngf, kernel_size=1)]
        mult_ins, mult_outs = [1, 2, 4, 4, 4, 8], [2, 4, 4, 4, 8, 8]
        for i in range(n_downsampling):
            encoder += [Conv2dLayer(ngf * mult_ins[i], ngf * mult_outs[i], kernel_size=3, down=2)]
        self.model = nn.Sequential(*encoder)

    def forward(self, x):
        return self.model(x)


class Dense(nn.Module):
    """reference networks.py:391-408: per-pixel Linear -> InstanceNorm2d -> LeakyReLU (slope 0.01).  The Linear is a
    1x1 convolution: on the inference route it runs the MFMA kernel with the bias in its epilogue."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.bn = nn.InstanceNorm2d(out_channels)
        self.activation = nn.LeakyReLU()
        self.linear = nn.Linear(in_channels, out_channels)
        self._cache = _PackCache()

    def forward(self, x):
        if _fast_ok(x, self.linear.weight, self.linear.bias):
            w = self.linear.weight
            packed = self._cache.get('w', [w], lambda: conv2d_mfma.pack_weight(w.detach().reshape(self.out_channels, self.in_channels, 1, 1)))
            out = conv2d_mfma.conv2d_forward(x, packed, self.out_channels, 1, 1, bias=self.linear.bias)
        else:
            out = self.linear(x.permute((0, 2, 3, 1))).permute((0, 3, 1, 2))
        return self.activation(self.bn(out))


class StyleEncoderNetworkV18(nn.Module):
    """reference networks.py:1727-1774."""

    def __init__(self, input_nc, output_nc, ngf=64, n_downsampling=4):
        super().__init__()
        encoder = [Conv2dLayer(input_nc, ngf, kernel_size=1)]
        for mult_in, mult_out in zip([1, 2, 4], [2, 4, 8]):
            encoder += [Dense(ngf * mult_in, ngf * mult_in), Conv2dLayer(ngf * mult_in, ngf * mult_out, kernel_size=3, down=2)]
        for mult_in, mult_out in zip([8, 8, 8], [8, 8, 8]):
            encoder += [Dense(ngf * mult_in, ngf * mult_in), Conv2dLayer(ngf * mult_in, ngf * mult_out, kernel_size=3)]
        encoder += [nn.AdaptiveAvgPool2d(1)]
        self.model = nn.Sequential(*encoder)
        self.fc = FullyConnectedLayer(output_nc, output_nc)
        feat_enc = [Conv2dLayer(6, ngf, kernel_size=3)]
        for _ in range(3):
            feat_enc += [Conv2dLayer(ngf, ngf, kernel_size=3, down=2)]
        self.feat_enc = nn.Sequential(*feat_enc)

    def forward(self, x, const_input):
        const_feats = []
        for module in self.feat_enc:
            const_input = module(const_input)
            const_feats.append(const_input)
        for module in self.model:
            x = module(x)
        x = self.fc(x.view(x.size(0), -1))
        return x, const_feats


class GeneratorFull_v20(nn.Module):
    """reference networks.py:2330-2366."""

    def __init__(self, z_dim, c_dim, w_dim, img_resolution, img_channels, mapping_kwargs={}, synthesis_kwargs={}):
        super().__init__()
        self.z_dim, self.c_dim, self.w_dim, self.img_resolution, self.img_channels = z_dim, c_dim, w_dim, img_resolution, img_channels
        self.synthesis = SynthesisNetworkFull_v18(w_dim=w_dim, img_resolution=img_resolution, img_channels=img_channels, **synthesis_kwargs)
        self.num_ws = self.synthesis.num_ws
        self.mapping = MappingNetwork(z_dim=z_dim, c_dim=c_dim, w_dim=w_dim, num_ws=self.num_ws, **mapping_kwargs)
        self.const_encoding = ConstEncoderNetwork(input_nc=3 + 2, output_nc=512, ngf=64, n_downsampling=6)
        self.style_encoding = StyleEncoderNetworkV18(input_nc=(10 * 3 + 5 * 3), output_nc=512, ngf=64, n_downsampling=6)

    def set_half(self, dtype, from_res=64):
        """`SynthesisNetworkFull_v18.set_half`: the synthesis blocks at resolution >= `from_res` in bf16 / fp16 on the GPU's inference route (None: float32);
        mapping and both encoders stay float32.  Returns self."""
        self.synthesis.set_half(dtype, from_res=from_res)
        return self

    def forward(self, z, c, retain, pose, denorm_upper_input, denorm_lower_input, denorm_upper_mask, denorm_lower_mask,
                gt_parsing=None, truncation_psi=1, truncation_cutoff=None, **synthesis_kwargs):
        pose_feat = self.const_encoding(pose)
        stylecode, feats = self.style_encoding(c, retain)
        ws = self.mapping(z, stylecode, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff)
        cat_feats = {str(feat.shape[2]): feat for feat in feats}
        return self.synthesis(ws, pose_feat, cat_feats, denorm_upper_input, denorm_lower_input, denorm_upper_mask,
                              denorm_lower_mask, gt_parsing, **synthesis_kwargs)


# ============================================================================
# Downstream of synthesis in the training step: the two discriminators
# (image+pose, 6 channels; parsing+pose, 10 channels).  Same ops again; fp16 blocks (num_fp16_res > 0) run their convolutions --
# forward, input gradients and the R1 double backward -- on the 16-bit MFMA kernel (conv2d_mfma16, channels-last); their weight
# gradients take aten::convolution_backward; bias_act / upfirdn2d are this package's HIP kernels in every precision.

class DiscriminatorBlock(nn.Module):
    """One resolution of the discriminator (reference networks.py:444-523): [fromrgb] -> conv0 -> conv1 (down 2), with
    a 1x1 down-sampling shortcut in the 'resnet' form.  Half-precision blocks keep their activations channels-last: the
    layout of the 16-bit MFMA convolution (a storage choice only; the reference leaves it to --nhwc)."""

    def __init__(self, in_channels, tmp_channels, out_channels, resolution, img_channels, first_layer_idx, architecture='resnet',
                 activation='lrelu', resample_filter=[1, 3, 3, 1], conv_clamp=None, use_fp16=False, fp16_channels_last=False, freeze_layers=0):
        assert in_channels in [0, tmp_channels]
        assert architecture in ['orig', 'skip', 'resnet']
        super().__init__()
        self.in_channels, self.resolution, self.img_channels = in_channels, resolution, img_channels
        self.first_layer_idx, self.architecture, self.use_fp16 = first_layer_idx, architecture, use_fp16
        self.channels_last = (use_fp16 and fp16_channels_last)
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        self.num_layers = 0

        def layer(cin, cout, k, **kw):      # layers are numbered in creation order; the first `freeze_layers` stay fixed
            idx = self.first_layer_idx + self.num_layers
            self.num_layers += 1
            return Conv2dLayer(cin, cout, kernel_size=k, trainable=idx >= freeze_layers, channels_last=self.channels_last, **kw)
        self.has_fromrgb = in_channels == 0 or architecture == 'skip'
        if self.has_fromrgb:
            self.fromrgb = layer(img_channels, tmp_channels, 1, activation=activation, conv_clamp=conv_clamp)
        self.conv0 = layer(tmp_channels, tmp_channels, 3, activation=activation, conv_clamp=conv_clamp)
        self.conv1 = layer(tmp_channels, out_channels, 3, activation=activation, down=2, resample_filter=resample_filter, conv_clamp=conv_clamp)
        if architecture == 'resnet':
            self.skip = layer(tmp_channels, out_channels, 1, bias=False, down=2, resample_filter=resample_filter)

    def forward(self, x, img, force_fp32=False):
        half = self.use_fp16 and not force_fp32
        fmt = dict(dtype=torch.float16 if half else torch.float32,
                   memory_format=torch.channels_last if (half or (self.channels_last and not force_fp32)) else torch.contiguous_format)
        if x is not None:
            misc.assert_shape(x, [None, self.in_channels, self.resolution, self.resolution])
            x = x.to(**fmt)
        if self.has_fromrgb:
            misc.assert_shape(img, [None, self.img_channels, self.resolution, self.resolution])
            img = img.to(**fmt)
            feat = self.fromrgb(img)
            x = feat if x is None else x + feat
            img = upfirdn2d.downsample2d(img, self.resample_filter) if self.architecture == 'skip' else None
        if self.architecture == 'resnet':    # shortcut + conv1(conv0(x)), both scaled by sqrt(1/2); the add rides in conv1
            x = self.conv1(self.conv0(x), gain=SQRT_HALF, residual=self.skip(x, gain=SQRT_HALF))
        else:
            x = self.conv1(self.conv0(x))
        assert x.dtype == fmt['dtype']
        return x, img


class MinibatchStdLayer(nn.Module):
    """Appends, per group of `group_size` samples, the mean standard deviation over the group as extra feature maps
    (reference networks.py:528-549)."""

    def __init__(self, group_size, num_channels=1):
        super().__init__()
        self.group_size, self.num_channels = group_size, num_channels

    def forward(self, x):
        n, c, h, w = x.shape
        group = n if self.group_size is None else min(int(self.group_size), int(n))
        feats = self.num_channels
        split = x.reshape(group, n // group, feats, c // feats, h, w)        # [group member, group, stat channel, c, h, w]
        std = (split.var(dim=0, unbiased=False) + 1e-8).sqrt()               # spread of each value across its group
        stat = std.mean(dim=[2, 3, 4])                                       # [groups, feats]
        stat_map = stat.reshape(n // group, feats, 1, 1).repeat(group, 1, h, w)
        return torch.cat([x, stat_map], dim=1)


class DiscriminatorEpilogue(nn.Module):
    """4x4 head (reference networks.py:554-607): minibatch-std -> conv -> two dense layers -> projection on the
    conditioning vector."""

    def __init__(self, in_channels, cmap_dim, resolution, img_channels, architecture='resnet', mbstd_group_size=4, mbstd_num_channels=1,
                 activation='lrelu', conv_clamp=None):
        assert architecture in ['orig', 'skip', 'resnet']
        super().__init__()
        self.in_channels, self.cmap_dim, self.resolution, self.img_channels, self.architecture = in_channels, cmap_dim, resolution, img_channels, architecture
        if architecture == 'skip':
            self.fromrgb = Conv2dLayer(img_channels, in_channels, kernel_size=1, activation=activation)
        self.mbstd = MinibatchStdLayer(group_size=mbstd_group_size, num_channels=mbstd_num_channels) if mbstd_num_channels > 0 else None
        self.conv = Conv2dLayer(in_channels + mbstd_num_channels, in_channels, kernel_size=3, activation=activation, conv_clamp=conv_clamp)
        self.fc = FullyConnectedLayer(in_channels * (resolution ** 2), in_channels, activation=activation)
        self.out = FullyConnectedLayer(in_channels, 1 if cmap_dim == 0 else cmap_dim)

    def forward(self, x, img, cmap, force_fp32=False):
        misc.assert_shape(x, [None, self.in_channels, self.resolution, self.resolution])
        fp32 = dict(dtype=torch.float32, memory_format=torch.contiguous_format)      # the head always runs in float32
        x = x.to(**fp32)
        if self.architecture == 'skip':
            misc.assert_shape(img, [None, self.img_channels, self.resolution, self.resolution])
            x = x + self.fromrgb(img.to(**fp32))
        if self.mbstd is not None:
            x = self.mbstd(x)
        score = self.out(self.fc(self.conv(x).flatten(1)))
        if self.cmap_dim > 0:
            misc.assert_shape(cmap, [None, self.cmap_dim])
            score = (score * cmap).sum(dim=1, keepdim=True) / np.sqrt(self.cmap_dim)
        return score


class Discriminator(nn.Module):
    """Reference networks.py:612-666.  Two instances in the training step: image + pose (6 channels) and parsing + pose (10)."""

    def __init__(self, c_dim, img_resolution, img_channels, architecture='resnet', channel_base=32768, channel_max=512, num_fp16_res=0,
                 conv_clamp=None, cmap_dim=None, block_kwargs={}, mapping_kwargs={}, epilogue_kwargs={}):
        super().__init__()
        self.c_dim, self.img_resolution, self.img_channels = c_dim, img_resolution, img_channels
        self.img_resolution_log2 = int(np.log2(img_resolution))
        self.block_resolutions = [1 << e for e in range(self.img_resolution_log2, 2, -1)]
        width = lambda res: min(channel_base // res, channel_max)
        fp16_from = max(1 << (self.img_resolution_log2 + 1 - num_fp16_res), 8)        # blocks at this resolution and above run in fp16
        cmap_dim = 0 if c_dim == 0 else (width(4) if cmap_dim is None else cmap_dim)
        shared = dict(img_channels=img_channels, architecture=architecture, conv_clamp=conv_clamp)
        layer_idx = 0
        for res in self.block_resolutions:
            block = DiscriminatorBlock(width(res) if res < img_resolution else 0, width(res), width(res // 2), resolution=res,
                                       first_layer_idx=layer_idx, use_fp16=(res >= fp16_from), **block_kwargs, **shared)
            setattr(self, f'b{res}', block)
            layer_idx += block.num_layers
        if c_dim > 0:
            self.mapping = MappingNetwork(z_dim=0, c_dim=c_dim, w_dim=cmap_dim, num_ws=None, w_avg_beta=None, **mapping_kwargs)
        self.b4 = DiscriminatorEpilogue(width(4), cmap_dim=cmap_dim, resolution=4, **epilogue_kwargs, **shared)

    def forward(self, img, c, **block_kwargs):
        x = None
        for res in self.block_resolutions:
            x, img = getattr(self, f'b{res}')(x, img, **block_kwargs)
        return self.b4(x, img, self.mapping(None, c) if self.c_dim > 0 else None)
