"""The folded tail of the texture block (csrc/conv3x3_fold.hip, networks._SynthesisBlockBase._tail_folded): the last two convolutions of spade_b512,
conv1 (3x3) over h' plus skip (1x1) over s', and the ToRGB head that alone reads their sum, computed as one per-sample linear map of (h', s') in one
streaming pass.

Reference everywhere: the UNFUSED composition in float64 (3x3 with zero padding + 1x1 -> modulated 1x1 head -> bias, clamp, skip image).  Bound (the project's
rule for reassociated kernels): the folded path's max error against float64 may be at most 2x the error of the unfused float32 path (the two convolutions as
the block launches them at that shape, then pg_conv1x1_small) against the same float64 values; both are measured here and printed.  Run with ``-m gpu`` on an
MI355X."""

import pytest
import torch

from detgen import det_tensor, fill_module_

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import conv2d_mfma
    assert conv2d_mfma._init() is not None   # native code loaded, or fail loudly


def _block(c, clamp, tag):
    """A texture block of c -> c channels at resolution 64; the kernel tests use only its spade_b512.conv1 / .skip and its torgb."""
    from training import networks as PN
    b = PN.SynthesisBlockFull_v1_v4(c, c, w_dim=32, resolution=64, img_channels=3, is_last=True, is_style=False, conv_clamp=clamp)
    return fill_module_(b, tag).to(DEV).eval()


def _inputs(tag, n, c, h, w, skip):
    hh, ss = det_tensor(tag + 'h', [n, c, h, w]).to(DEV), det_tensor(tag + 's', [n, c, h, w]).to(DEV)
    styles = (1.0 + det_tensor(tag + 'st', [n, c], scale=0.3)).to(DEV) / float(c) ** 0.5      # affine(w) * weight_gain of a ToRGB layer
    img = det_tensor(tag + 'img', [n, 3, h, w]).to(DEV) if skip else None
    return hh, ss, styles, img


def tail_f64(block, h, s, styles, img):
    """conv1 (3x3, zero padding) over h + skip (1x1) over s, then the block's ToRGB head, layer by layer in float64 (on the CPU).  Returns (rgb, the head's
    values in front of its clamp)."""
    sb, tr = block.spade_b512, block.torgb
    d = lambda t: t.detach().double().cpu()
    x = (torch.nn.functional.conv2d(d(h), d(sb.conv1.weight) * sb.conv1.weight_gain, padding=1)
         + torch.nn.functional.conv2d(d(s), d(sb.skip.weight) * sb.skip.weight_gain))
    cm = tr.weight.shape[1]
    pre = torch.einsum('noc,nchw->nohw', d(tr.weight).reshape(1, -1, cm) * d(styles)[:, None, :], x) + d(tr.bias)[None, :, None, None]
    cl = float(tr.conv_clamp) if tr.conv_clamp is not None else float('inf')
    rgb = pre.clamp(-cl, cl)
    return (rgb + d(img) if img is not None else rgb), pre


def _unfused(block, h, s, styles, img):
    """The launches the block runs without the fold: skip, conv1 with the residual add, the streaming ToRGB head."""
    x = block.spade_b512.tail(h, s)
    return block.torgb(x, None, skip_img=img, styles=styles)[0]


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max())


# (id, N, C, H, W, skip image, clamp)
CASES = [('n2_c64_16x16', 2, 64, 16, 16, False, None),
         ('n3_c32_8x12_skip_clamp', 3, 32, 8, 12, True, 256.0),
         ('n2_c64_16x16_clamp_bites', 2, 64, 16, 16, False, 0.5),
         ('n1_c64_6x260', 1, 64, 6, 260, False, None),          # more than one wave per row, W % 256 != 0
         ('n1_c11_1x4', 1, 11, 1, 4, False, None)]              # one row, a channel count that is no multiple of the unroll


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_folded_tail_vs_float64(case, monkeypatch):
    """Kernel against float64: folded error <= 2 x the unfused float32 path's error."""
    tag, n, c, h, w, skip, clamp = case
    monkeypatch.delenv('PG_TEX_FOLD', raising=False)
    block = _block(c, clamp, f'tex.{tag}.')
    hh, ss, styles, img = _inputs(f'tex.{tag}.', n, c, h, w, skip)
    with torch.no_grad():
        ref, pre = tail_f64(block, hh, ss, styles, img)
        rgb_u = _unfused(block, hh, ss, styles, img)
        rgb_f = block._tail_folded(hh, ss, None, styles, img)
    assert rgb_f is not None, 'the folded route did not run'
    assert rgb_f.shape == rgb_u.shape == (n, 3, h, w) and rgb_f.is_contiguous()
    if clamp is not None and clamp < 1:        # the clamp must actually bite, and not everywhere
        hit = float(((pre.abs() >= clamp).double()).mean())
        print(f'{tag}: {hit:.3f} of the reference values are clamped')
        assert 0.05 < hit < 0.95, hit
    ef, eu = _err(rgb_f, ref), _err(rgb_u, ref)
    print(f'{tag}: folded {ef:.3e}, unfused {eu:.3e} (max |ref| {float(ref.abs().max()):.3e})')
    assert ef <= 2 * eu, f'{tag}: folded error {ef:.3e} > 2 x unfused {eu:.3e}'


@pytest.mark.parametrize('shape', [(2, 64, 16, 16), (1, 64, 6, 260)], ids=['n2_c64_16x16', 'n1_c64_6x260'])
def test_folded_tail_border(shape, monkeypatch):
    """Inputs that are non-zero only in the outermost rows and columns: the results along the image border (and everywhere else) stay within the bound of
    the float64 composition -- padding and neighbour-lane mistakes that random interiors hide show here."""
    n, c, h, w = shape
    monkeypatch.delenv('PG_TEX_FOLD', raising=False)
    tag = f'tex.border.{h}x{w}.'
    block = _block(c, None, tag)
    hh, ss, styles, img = _inputs(tag, n, c, h, w, True)
    ring = torch.zeros([1, 1, h, w], device=DEV)
    ring[..., 0, :] = ring[..., -1, :] = ring[..., :, 0] = ring[..., :, -1] = 1.0
    hh, ss = hh * ring, ss * ring
    with torch.no_grad():
        ref, _ = tail_f64(block, hh, ss, styles, img)
        rgb_u = _unfused(block, hh, ss, styles, img)
        rgb_f = block._tail_folded(hh, ss, None, styles, img)
    assert rgb_f is not None, 'the folded route did not run'
    m = ring.bool().cpu().expand_as(ref)
    eu = _err(rgb_u, ref)
    ef_border, ef_all = float((rgb_f.double().cpu() - ref)[m].abs().max()), _err(rgb_f, ref)
    print(f'border {h}x{w}: folded {ef_border:.3e} on the border, {ef_all:.3e} anywhere, unfused {eu:.3e}')
    assert ef_border <= 2 * eu and ef_all <= 2 * eu


def _block_inputs(tag, n, c, res, h=None, w=None):
    """Inputs of `_spade_heads`: the features in front of spade_b512, a parsing map with the labels 0..6, a style vector, the up-sampled skip image."""
    h, w = h or res, w or res
    x = det_tensor(tag + 'x', [n, c, h, w]).to(DEV)
    parsing = (torch.arange(n * h * w).reshape(n, 1, h, w) // 3 % 7).float().to(DEV)
    wv = det_tensor(tag + 'w', [n, 32]).to(DEV)
    img = det_tensor(tag + 'img', [n, 3, h, w]).to(DEV)
    return x, parsing, wv, img


def test_folded_tail_decline_falls_back(monkeypatch):
    """W % 4 != 0: the kernel answers PG_ERR_UNSUPPORTED and the block runs its three launches one after the other -- the same launches, hence the same bits,
    as with the fold switched off -- and returns its feature map."""
    from torch_utils.ops import _native as nat
    from torch_utils.ops import conv2d_mfma
    monkeypatch.delenv('PG_TEX_FOLD', raising=False)
    block = _block(64, 256.0, 'tex.odd.')
    hh, ss, styles, img = _inputs('tex.odd.', 2, 64, 6, 6, True)
    wn = det_tensor('tex.odd.wn', [2, 3, 640]).to(DEV)
    bn = det_tensor('tex.odd.bn', [2, 3]).to(DEV)
    with pytest.raises(nat.NativeNotCovered):
        conv2d_mfma.conv3x3_fold_head(hh, ss, wn, bn)
    x, parsing, wv, img = _block_inputs('tex.odd.', 2, 64, 64, h=6, w=6)
    with torch.no_grad():
        assert block._tail_folded(hh, ss, None, styles, img) is None
        xa, rgb_a, _ = block._spade_heads(x, parsing, wv, None, img, True, feat_unused=True)
        monkeypatch.setenv('PG_TEX_FOLD', '0')
        xb, rgb_b, _ = block._spade_heads(x, parsing, wv, None, img, True, feat_unused=True)
    assert xa is not None and torch.equal(xa, xb) and torch.equal(rgb_a, rgb_b)


@pytest.fixture(scope='module')
def routed():
    """One small texture block (64 -> 64 channels, resolution 64, N = 2) run with `_feat_unused=True`, without the flag, with the flag under PG_TEX_FOLD=0,
    under autograd and in bf16; the tensors `_tail_folded` received are kept, and its calls counted."""
    import os
    from training import networks as PN
    block = _block(64, 256.0, 'tex.route.')
    n, res = 2, 64
    x = det_tensor('tex.route.x', [n, 64, res // 2, res // 2]).to(DEV)
    img = det_tensor('tex.route.img', [n, 3, res // 2, res // 2]).to(DEV)
    ws = det_tensor('tex.route.ws', [n, 3, 32]).to(DEV)
    cat_feat = {str(res): det_tensor('tex.route.feat', [n, 64, res, res]).to(DEV)}
    parsing = (torch.arange(n * res * res).reshape(n, 1, res, res) // 5 % 7).float().to(DEV)
    seen = []
    inner = block._tail_folded

    def tail_folded(h, s, w, styles, im):
        r = inner(h, s, w, styles, im)
        seen.append((h, s, w, styles, im, r is not None))
        return r
    block._tail_folded = tail_folded
    run = lambda **kw: block(x, img, ws, None, cat_feat, parsing, noise_mode='const', **kw)
    old = os.environ.pop('PG_TEX_FOLD', None)
    out = {}
    try:
        with torch.no_grad():
            out['folded'] = run(force_fp32=True, _feat_unused=True)
            out['calls_folded'] = len(seen)
            out['plain'] = run(force_fp32=True)
            out['calls_plain'] = len(seen)
            os.environ['PG_TEX_FOLD'] = '0'
            out['off'] = run(force_fp32=True, _feat_unused=True)
            del os.environ['PG_TEX_FOLD']
            out['calls_off'] = len(seen)
            h, s, w, styles, im, _ = seen[0]
            styles = block.torgb.affine(w) * block.torgb.weight_gain if styles is None else styles
            out['ref'] = tail_f64(block, h, s, styles, im)[0]
        with torch.enable_grad():
            out['grad'] = tuple(t.detach() if t is not None else None for t in run(force_fp32=True, _feat_unused=True))
        out['calls_grad'] = len(seen)
        block.half_dtype = torch.bfloat16
        with torch.no_grad():
            out['half'] = run(_feat_unused=True)
        block.half_dtype = None
        out['calls_half'] = len(seen)
    finally:
        if old is not None:
            os.environ['PG_TEX_FOLD'] = old
    out['seen'] = seen
    return out


def test_block_routing_folds(routed):
    """With `_feat_unused=True` the block returns no feature map and its image is within the bound of the float64 composition of the tail, taken from the
    very tensors the fold received (everything in front of them is the same launches on both routes)."""
    x, rgb, pp = routed['folded']
    assert routed['calls_folded'] == 1 and routed['seen'][0][5], 'the folded route did not run'
    assert x is None and pp is None and rgb.shape == (2, 3, 64, 64)
    ef, eu = _err(rgb, routed['ref']), _err(routed['plain'][1], routed['ref'])
    print(f'block: folded {ef:.3e}, plain {eu:.3e} (max |ref| {float(routed["ref"].abs().max()):.3e})')
    assert ef <= 2 * eu, f'folded error {ef:.3e} > 2 x plain {eu:.3e}'


def test_block_routing_plain_unchanged(routed):
    """Without the flag the fold is not even asked, the feature map comes back, and the results are those of the three launches (PG_TEX_FOLD=0) bit for bit."""
    assert routed['calls_plain'] == routed['calls_folded'] and routed['calls_off'] == routed['calls_plain']
    (xp, rgbp, _), (xo, rgbo, _) = routed['plain'], routed['off']
    assert xp is not None and xo is not None and torch.equal(xp, xo) and torch.equal(rgbp, rgbo)


def test_block_routing_not_under_autograd_or_half(routed):
    """Under torch.enable_grad() and in the 16-bit mode the fold does not run: the feature map comes back."""
    assert routed['calls_grad'] == routed['calls_off'] and routed['calls_half'] == routed['calls_off']
    assert routed['grad'][0] is not None and routed['half'][0] is not None
    assert routed['half'][0].dtype == torch.bfloat16 and routed['half'][1].dtype == torch.float32
    assert float((routed['grad'][1] - routed['plain'][1]).abs().max()) < 1e-3      # the autograd route computes the same image from the same inputs


def test_folded_tail_repeatable(monkeypatch):
    """Three launches on the same inputs: bit-identical (no atomics, fixed summation order)."""
    monkeypatch.delenv('PG_TEX_FOLD', raising=False)
    block = _block(64, 256.0, 'tex.rep.')
    hh, ss, styles, img = _inputs('tex.rep.', 2, 64, 40, 260, True)
    with torch.no_grad():
        a, b, c = (block._tail_folded(hh, ss, None, styles, img) for _ in range(3))
    assert a is not None and torch.equal(a, b) and torch.equal(a, c)
