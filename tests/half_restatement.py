"""Test-side 16-bit restatement of the try-on generator's half mode (``SynthesisNetworkFull_v18.set_half``).

The float32 CPU oracle's composition (oracle/network_ref.py) in plain torch, run in float32, with tensors rounded to the 16-bit type at exactly the points
where the native route stores 16-bit tensors: the inputs of the first 16-bit block and of ``merge_conv`` / the SPADE blocks, every convolution output (after
its epilogue), every combine output, and the cast weights (shared weights times their gain; the per-sample weights w * styles * dcoefs of the modulated
convolutions).  The ToRGB heads, the skip image, the statistics (from the rounded tensor) and everything below ``from_res`` stay float32, as in the product.
Nothing here touches the product's code."""

import math

import torch
import torch.nn.functional as F

from oracle import network_ref as NR
from oracle import ops_ref as R

SQRT_HALF = math.sqrt(0.5)


def rounder(dtype):
    return lambda t: t.to(dtype).to(torch.float32)


def stats(x, eps=1e-5):
    mean = x.mean(dim=(2, 3), keepdim=True)
    var = (x - mean).square().mean(dim=(2, 3), keepdim=True)
    return mean, 1 / torch.sqrt(var + eps)


def spade_conv(layer, x, rd, relu=False, residual=None, round_weight=True):
    """Spade_Conv2dLayer(no_act=True) as one 16-bit launch: accumulate in float32, ReLU / residual in the epilogue, one rounding."""
    w = layer.weight * layer.weight_gain
    y = F.conv2d(x, rd(w) if round_weight else w, padding=layer.padding)
    if relu:
        y = torch.relu(y)
    if residual is not None:
        y = y + residual
    return rd(y)


def norm_block(nb, x, feat, st, post, rd):
    """Spade_Norm_Block + the consumer's pre-activation `post` = (act, gain).  `feat` with one channel is the float32 parsing map (float32 stencil, output
    cast); otherwise the 16-bit garment features."""
    mean, rstd = st
    actv = spade_conv(nb.conv_mlp, feat, rd, relu=True, round_weight=feat.shape[1] != 1)
    c = nb.conv_gamma.weight.shape[0]
    w = torch.cat([nb.conv_gamma.weight * nb.conv_gamma.weight_gain, nb.conv_beta.weight * nb.conv_beta.weight_gain])
    gb = rd(F.conv2d(actv, rd(w), padding=1))
    y = (x - mean) * rstd * (1 + gb[:, :c]) + gb[:, c:]
    act, gain = post
    return rd(R.bias_act(y, None, act=act, gain=gain))


def spade_res_block(blk, x, feat, rd):
    """Spade_ResBlockV4_512 on a 16-bit x (already rounded): the inference route's call structure."""
    x = spade_conv(blk.conv, x, rd)
    st = stats(x)
    g = blk.skip.act_gain
    y = spade_conv(blk.skip, norm_block(blk.spade_skip, x, feat, st, (blk.skip.activation, g * SQRT_HALF), rd), rd)
    x = spade_conv(blk.conv0, norm_block(blk.spade0, x, feat, st, (blk.conv0.activation, blk.conv0.act_gain), rd), rd)
    st1 = stats(x)
    return spade_conv(blk.conv1, norm_block(blk.spade1, x, feat, st1, (blk.conv1.activation, blk.conv1.act_gain * SQRT_HALF), rd), rd, residual=y)


def synthesis_layer(layer, x, w, rd, noise_mode='const'):
    """SynthesisLayer with per-sample 16-bit weights (the reference's fused form, networks.py:85-94), noise / bias / lrelu / clamp in the epilogue."""
    styles = layer.affine(w)
    n, cin = styles.shape
    cout, _, kh, kw = layer.weight.shape
    ws = layer.weight[None] * styles[:, None, :, None, None]
    ws = rd(ws * (ws.square().sum(dim=(2, 3, 4), keepdim=True) + 1e-8).rsqrt())
    y = R.conv2d_resample(x.reshape(1, n * cin, *x.shape[2:]), ws.reshape(n * cout, cin, kh, kw), f=layer.resample_filter, up=layer.up, padding=layer.padding,
                          groups=n, flip_weight=(layer.up == 1))
    y = y.reshape(n, cout, *y.shape[2:])
    if layer.use_noise and noise_mode == 'const':
        y = y + layer.noise_const * layer.noise_strength
    return rd(R.bias_act(y, layer.bias, act=layer.activation, gain=layer.act_gain, clamp=layer.conv_clamp))


def block(blk, x, img, ws, cat_feat, parsing, rd, noise_mode='const'):
    """SynthesisBlockFull in half mode (in_channels > 0)."""
    x = rd(x)
    x = synthesis_layer(blk.conv0, x, ws[:, 0], rd, noise_mode)
    x = synthesis_layer(blk.conv1, x, ws[:, 1], rd, noise_mode)
    if x.shape[2] > 32:
        m = blk.merge_conv
        x = torch.cat([x, rd(cat_feat[str(x.shape[2])])], dim=1)
        x = rd(F.conv2d(x, rd(m.weight * m.weight_gain)) + m.bias[None, :, None, None])
    if blk.texture:
        x = spade_res_block(blk.spade_b512, x, parsing, rd)
    img = R.upsample2d(img, blk.resample_filter)
    y, pred_parsing = blk.torgb(x, ws[:, 2])                 # float32 heads on the 16-bit features
    return x, img + y, pred_parsing


def synthesis(syn, dtype, ws, pose_feat, cat_feat, du, dl, mu, ml, gt_parsing, from_res=64, noise_mode='const'):
    """oracle SynthesisNetworkFull_v18.forward with the blocks at resolution >= from_res restated in `dtype`."""
    rd = rounder(dtype)
    ws = ws.to(torch.float32)
    block_ws, idx = [], 0
    for res in syn.block_resolutions:
        b = getattr(syn, f'b{res}')
        block_ws.append(ws.narrow(1, idx, b.num_conv + b.num_torgb))
        idx += b.num_conv
    x = img = None
    mid = syn.block_resolutions[-2]
    for res, cur in zip(syn.block_resolutions, block_ws):
        b = getattr(syn, f'b{res}')
        if res >= from_res:
            x, img, pred_parsing = block(b, x, img, cur, cat_feat, None, rd, noise_mode)
        else:
            x, img, pred_parsing = b(x, img, cur, pose_feat, cat_feat, noise_mode=noise_mode)
        if res == mid:
            x_mid, img_mid = x, img
    parsing_index = gt_parsing if gt_parsing is not None else torch.argmax(pred_parsing, dim=1)[:, None].float()
    upper = (parsing_index == 1).float() + (parsing_index == 4).float()
    lower = (parsing_index == 2).float() + (parsing_index == 3).float()
    feat = (syn.get_spade_feat(upper, mu, du) * (NR.nearest_half(upper) > 0.9).float()
            + syn.get_spade_feat(lower, ml, dl) * (NR.nearest_half(lower) > 0.9).float())
    if mid >= from_res:
        y = spade_res_block(syn.spade_b256_2, spade_res_block(syn.spade_b256_1, x_mid, rd(feat), rd), rd(feat), rd)
    else:
        y = syn.spade_b256_2(syn.spade_b256_1(x_mid, feat), feat)
    _, finetune_img, _ = block(syn.texture_b512, y, img_mid, block_ws[-1], cat_feat, parsing_index, rd, noise_mode)
    return img, finetune_img, pred_parsing


def generator_front(G, z, c, retain, pose):
    """The float32 part in front of the synthesis network, shared by the oracle and the restatement: (ws, pose_feat, cat_feats)."""
    pose_feat = G.const_encoding(pose)
    stylecode, feats = G.style_encoding(c, retain)
    ws = G.mapping(z, stylecode)
    return ws, pose_feat, {str(f.shape[2]): f for f in feats}


def deviations(got, want):
    """max-abs deviation per output (img, finetune_img, pred_parsing)."""
    return [float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max()) for a, b in zip(got, want)]
