"""The folded heads of the last style block (csrc/conv1x1_fold.hip, networks._SynthesisBlockBase._heads_folded): merge_conv (a linear 1x1 convolution over
[x ; cat_feat]) and the ToRGB / parsing heads behind it computed as one per-sample linear map of the merge inputs, in one streaming pass.

Reference everywhere: the UNFUSED composition in float64 (merge 1x1 -> modulated 1x1 heads -> bias, clamp, skip image).  Bound (the project's rule for
reassociated kernels): the folded path's max error against float64 may be at most 2x the error of the unfused float32 path (merge_conv on the MFMA / streaming
kernel, then pg_conv1x1_small per head) against the same float64 values; both are measured here and printed.  Run with ``-m gpu`` on an MI355X."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases as C
from detgen import det_tensor, fill_module_
from head_fold_worker import heads_f64

pytestmark = pytest.mark.gpu

DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'head_fold_worker.py')


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import conv2d_mfma
    assert conv2d_mfma._init() is not None   # native code loaded, or fail loudly


def _block(c1, parsing, clamp, tag):
    """A style block whose merge_conv takes c1 + 64 channels; only its merge_conv / torgb are used here."""
    from training import networks as PN
    b = PN.SynthesisBlockFull_v1_v6(c1, c1, w_dim=32, resolution=64, img_channels=3, is_last=parsing, is_style=True, conv_clamp=clamp)
    return fill_module_(b, tag).to(DEV).eval()


def _inputs(tag, n, c1, h, w, skip):
    x = det_tensor(tag + 'x', [n, c1, h, w]).to(DEV)
    feat = det_tensor(tag + 'feat', [n, 64, h, w]).to(DEV)
    styles = (1.0 + det_tensor(tag + 's', [n, c1], scale=0.3)).to(DEV) / float(np.sqrt(c1))      # affine(w) * weight_gain of a ToRGB layer
    img = det_tensor(tag + 'img', [n, 3, h, w]).to(DEV) if skip else None
    return x, feat, styles, img


def _err(got, ref):
    return float((got.double() - ref).abs().max())


# (id, N, C1, H, W, parsing head, skip image, clamp)
CASES = [('n2_64+64_16x16_3+7', 2, 64, 16, 16, True, False, None),
         ('n3_128+64_8x12_3', 3, 128, 8, 12, False, False, None),
         ('n2_64+64_16x16_3+7_skip_clamp', 2, 64, 16, 16, True, True, 256.0),
         ('n2_64+64_16x16_3+7_skip_clamp_bites', 2, 64, 16, 16, True, True, 0.5)]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_folded_heads_vs_float64(case, monkeypatch):
    """Kernel against float64: folded error <= 2 x the unfused float32 path's error, per head."""
    tag, n, c1, h, w, parsing, skip, clamp = case
    monkeypatch.delenv('PG_HEAD_FOLD', raising=False)
    block = _block(c1, parsing, clamp, f'fold.{tag}.')
    x, feat, styles, img = _inputs(f'fold.{tag}.', n, c1, h, w, skip)
    with torch.no_grad():
        ref = heads_f64(block, x, feat, styles, img)
        xm, rgb_u, pp_u = block._merge_heads(x, feat, None, styles, img, True, feat_unused=False)
        xf, rgb_f, pp_f = block._merge_heads(x, feat, None, styles, img, True, feat_unused=True)
    assert xm is not None and xf is None, 'the folded route did not run (or the plain one did not return its feature map)'
    assert rgb_f.shape == rgb_u.shape == (n, 3, h, w) and rgb_f.is_contiguous()
    assert (pp_f is None) == (not parsing) and (pp_u is None) == (not parsing)
    if clamp is not None and clamp < 1:        # the clamp must actually bite, and not everywhere
        hit = float(((ref[1].abs() >= clamp).double()).mean())
        assert 0.05 < hit < 0.95, hit
    for name, f, u, r in (('rgb', rgb_f, rgb_u, ref[0]), ('parsing', pp_f, pp_u, ref[1])):
        if r is None:
            continue
        ef, eu = _err(f, r), _err(u, r)
        print(f'{tag} {name}: folded {ef:.3e}, unfused {eu:.3e} (max |ref| {float(r.abs().max()):.3e})')
        assert ef <= 2 * eu, f'{tag} {name}: folded error {ef:.3e} > 2 x unfused {eu:.3e}'


def test_folded_heads_decline_falls_back(monkeypatch):
    """H * W not a multiple of 4: the kernel answers PG_ERR_UNSUPPORTED, and the block runs the two layers one after the other -- the same launches, hence
    the same bits, as with the fold switched off."""
    from torch_utils.ops import _native as nat
    from torch_utils.ops import conv2d_mfma
    monkeypatch.delenv('PG_HEAD_FOLD', raising=False)
    block = _block(64, True, 256.0, 'fold.odd.')
    x, feat, styles, img = _inputs('fold.odd.', 2, 64, 5, 5, True)
    wn, bn = conv2d_mfma.conv1x1_fold_prep(torch.randn(64, 128, device=DEV), None, torch.randn(10, 64, device=DEV), None, styles)
    assert wn.shape == (2, 10, 128) and bn.shape == (2, 10)
    with pytest.raises(nat.NativeNotCovered):
        conv2d_mfma.conv1x1_fold_heads(x, feat, wn, bn, 3)
    with torch.no_grad():
        assert block._heads_folded(x, feat, None, styles, img) is None
        xa, rgb_a, pp_a = block._merge_heads(x, feat, None, styles, img, True, feat_unused=True)
        monkeypatch.setenv('PG_HEAD_FOLD', '0')
        xb, rgb_b, pp_b = block._merge_heads(x, feat, None, styles, img, True, feat_unused=True)
        ref = heads_f64(block, x, feat, styles, img)
    assert xa is not None and torch.equal(xa, xb) and torch.equal(rgb_a, rgb_b) and torch.equal(pp_a, pp_b)
    assert _err(rgb_a, ref[0]) < 1e-4 and _err(pp_a, ref[1]) < 1e-4      # float32 sums of 128 + 64 O(1) terms


def test_fold_kernel_edges():
    """The entry points alone, on what the block shapes do not reach: channel counts that are no multiple of the 8-plane unroll (11 + 2), one output tensor
    (c_a == Cout = 5: 8 accumulator rows), a skip image on the first 2 channels only, no styles / merge bias, and an image with more pixel quads than the
    grid has threads (N = 4: 513 workgroups x 256 quads < 1024 x 516 / 4), so the grid-stride loop runs.  Against float64."""
    from torch_utils.ops import conv2d_mfma
    n, c1, c2, cm, cout, h, w = 4, 11, 2, 6, 5, 1024, 516
    x, x2 = det_tensor('fold.e.x', [n, c1, h, w]).to(DEV), det_tensor('fold.e.x2', [n, c2, h, w]).to(DEV)
    skip = det_tensor('fold.e.skip', [n, 2, h, w]).to(DEV)
    wm, bm = det_tensor('fold.e.wm', [cm, c1 + c2]).to(DEV), det_tensor('fold.e.bm', [cm]).to(DEV)
    wh, bh = det_tensor('fold.e.wh', [cout, cm]).to(DEV), det_tensor('fold.e.bh', [cout]).to(DEV)
    styles = det_tensor('fold.e.s', [n, cm]).to(DEV)
    wn, bn = conv2d_mfma.conv1x1_fold_prep(wm, bm, wh, bh, styles)
    mod = wh.double()[None] * styles.double()[:, None, :]
    w64, b64 = mod @ wm.double(), mod @ bm.double() + bh.double()
    assert _err(wn, w64) <= 2.0 ** -23 * float(w64.abs().max()) and _err(bn, b64) <= 2.0 ** -23 * float(b64.abs().max())     # correctly rounded float32
    ya, yb = conv2d_mfma.conv1x1_fold_heads(x, x2, wn, bn, cout, skip=skip, clamp=2.0)
    assert yb is None and ya.shape == (n, cout, h, w)
    worst = bound = 0.0
    for i in range(n):      # float64 one sample at a time (the whole batch in float64 would be 0.3 GB of temporaries)
        xi = torch.cat([x[i], x2[i]]).double()
        r = torch.einsum('oc,chw->ohw', wn[i].double(), xi).add(bn[i].double()[:, None, None]).clamp(-2.0, 2.0)
        r[:2] += skip[i].double()
        worst = max(worst, _err(ya[i], r))
        mag = torch.einsum('oc,chw->ohw', wn[i].double().abs(), xi.abs()).add(bn[i].double().abs()[:, None, None])
        mag[:2] += skip[i].double().abs()
        bound = max(bound, float(mag.max()))
    # forward error of a float32 sum of C products + bias + skip image in any order: (C + 2) roundings of 2^-24 relative to the sum of magnitudes
    bound *= (c1 + c2 + 2) * 2.0 ** -24
    print(f'edges: max error {worst:.3e} (bound {bound:.3e})')
    assert worst <= bound
    w0, b0 = conv2d_mfma.conv1x1_fold_prep(wm, None, wh, None, torch.ones_like(styles))
    assert _err(w0, (wh.double() @ wm.double())[None].expand(n, -1, -1)) <= 2.0 ** -23 * float(w64.abs().max()) and float(b0.abs().max()) == 0.0


@pytest.fixture(scope='module')
def routed(tmp_path_factory):
    """The reduced-width network once with PG_HEAD_FOLD=1 and once with 0, each in a fresh child process (both at once)."""
    tmp = tmp_path_factory.mktemp('head_fold')
    procs = {}
    for flag in ('1', '0'):
        out = str(tmp / f'fold{flag}.npz')
        procs[flag] = (out, subprocess.Popen([sys.executable, WORKER, out], env=dict(os.environ, PG_HEAD_FOLD=flag), stdout=subprocess.PIPE,
                                             stderr=subprocess.STDOUT, text=True))
    res = {}
    for flag, (out, p) in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, f'PG_HEAD_FOLD={flag} child failed:\n{log[-3000:]}'
        res[flag] = dict(np.load(out))
    return res


def test_network_routing_fold_vs_plain(routed):
    """SynthesisNetworkFull_v18 (reduced width, cases.G6_KW; the labelled parsing map is given, so finetune_img does not hang on argmax ties) under
    PG_HEAD_FOLD=1 and =0.  img and pred_parsing are the last style block's heads: each setting is measured against the float64 composition of those heads
    from the block's own input tensors (bit-identical under both settings, checked), folded <= 2 x plain.  finetune_img never sees the block's
    heads on this route: bit-identical.  pred_parsing.argmax(1) agrees on >= 99.9 % of the pixels."""
    on, off = routed['1'], routed['0']
    assert int(on['folded_calls']) == 2 and int(off['folded_calls']) == 0, 'PG_HEAD_FOLD did not switch the route'
    for name in ('ref_img', 'ref_pred_parsing'):
        assert np.array_equal(on[name], off[name]), f'{name}: the block inputs differ between the two settings'
    for name in ('img', 'pred_parsing'):
        ref = on['ref_' + name]
        ef, eu = float(np.abs(on[name] - ref).max()), float(np.abs(off[name] - ref).max())
        print(f'network {name}: folded {ef:.3e}, plain {eu:.3e}, folded vs plain {float(np.abs(on[name].astype(np.float64) - off[name]).max()):.3e} (max |ref| {float(np.abs(ref).max()):.3e})')
        assert ef <= 2 * eu, f'{name}: folded error {ef:.3e} > 2 x plain {eu:.3e}'
    assert np.array_equal(on['finetune_img'], off['finetune_img'])
    share = float((on['pred_parsing'].argmax(1) == off['pred_parsing'].argmax(1)).mean())
    print(f'network argmax agreement: {share:.6f}')
    assert share >= 0.999, share


def test_network_routing_repeatable(routed):
    """Two runs of the folded path in one process: bit-identical outputs (no atomics, fixed summation order)."""
    assert routed['1']['repeat_identical'].all() and routed['0']['repeat_identical'].all()
