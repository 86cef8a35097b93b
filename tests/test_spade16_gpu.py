"""The 16-bit channels-last SPADE kernels (csrc/spade16.hip) on the MI355X: pg_instance_norm_stats_cl16 and pg_spade_combine_cl16 against float64 on the
same 16-bit inputs, and ``Spade_ResBlockV4_512`` on the 16-bit route against the float32 module within twice the error of the test-side 16-bit restatement
(tests/half_restatement.py)."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.bfloat16, torch.float16]
NC = [(2, 16), (1, 48), (2, 128)]
HW = [(5, 7), (33, 65), (96, 96)]          # a plane smaller than a wave; odd extents; a plane spanning several workgroup chunks
# unit roundoff (half an ulp, relative) of the 16-bit types, and half the spacing of their subnormals
ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUBNORMAL_HALF = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _check_stats(x16, eps=1e-5):
    """mean rtol / atol 1e-6, rstd rtol 2e-5: the bars of the float32 kernel's parity tests (tests/test_hip_parity.py: test_support_kernels_vs_oracle,
    test_conv2d_winograd4_output_statistics); float64 reads the same 16-bit values, so input rounding is no part of the error."""
    from torch_utils.ops import conv2d_mfma16
    n, c = x16.shape[:2]
    mean, rstd = conv2d_mfma16.instance_norm_stats16(_cl(x16), eps=eps)
    again = conv2d_mfma16.instance_norm_stats16(_cl(x16), eps=eps)
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (n * c,) and tuple(rstd.shape) == (n * c,)
    assert torch.equal(mean, again[0]) and torch.equal(rstd, again[1])            # fixed reduction order, no atomics
    xd = x16.double()
    want_mean = xd.mean([2, 3]).reshape(-1).numpy()
    want_rstd = (xd.var([2, 3], unbiased=False) + eps).rsqrt().reshape(-1).numpy()
    print(f'stats {tuple(x16.shape)} {x16.dtype}: mean max-abs {np.abs(mean.cpu().numpy() - want_mean).max():.2e}, '
          f'rstd max-rel {np.abs(rstd.cpu().numpy() / want_rstd - 1).max():.2e}')
    np.testing.assert_allclose(mean.cpu().double().numpy(), want_mean, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(rstd.cpu().double().numpy(), want_rstd, rtol=2e-5, atol=0)
    return mean, rstd


@pytest.mark.parametrize('hw', HW, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('nc', NC, ids=lambda v: f'N{v[0]}C{v[1]}')
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_instance_norm_stats16(dtype, nc, hw):
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn([*nc, *hw], generator=gen) * torch.rand([1, nc[1], 1, 1], generator=gen).add(0.2) + torch.randn([1, nc[1], 1, 1], generator=gen)).to(dtype)
    _check_stats(x)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_instance_norm_stats16_constant_and_offset_planes(dtype):
    eps = 1e-5
    const = torch.full([2, 16, 33, 65], 3.25).to(dtype)
    const[1] = -100.0
    _, rstd = _check_stats(const, eps)
    assert float((rstd.cpu().double() * math.sqrt(eps) - 1).abs().max()) <= 2e-5       # rstd = 1 / sqrt(eps)
    gen = torch.Generator().manual_seed(6)
    # |mean| >> spread: a raw E[x^2] - E[x]^2 in float32 would lose the variance (1e-7 * 100^2 against 0.1^2)
    _check_stats((100.0 + 0.1 * torch.randn([2, 48, 96, 96], generator=gen)).to(dtype), eps)


POSTS = {'none': dict(act='linear', gain=1.0, clamp=None), 'relu_sqrt2': dict(act='relu', gain=math.sqrt(2), clamp=None),
         'relu_clamp': dict(act='relu', gain=1.0, clamp=256 * math.sqrt(0.5))}


@pytest.mark.parametrize('post', list(POSTS))
@pytest.mark.parametrize('hw', HW, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('nc', NC, ids=lambda v: f'N{v[0]}C{v[1]}')
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_spade_combine16(dtype, nc, hw, post):
    """Against the float64 formula on the same inputs (the float32 gain and clamp the C ABI receives included): the stored value is that number rounded
    once, i.e. within the type's unit roundoff of it (half an ulp; half a subnormal step below the normal range).  Elements whose unclamped value lies
    within one ulp of the clamp are left out (fewer than 0.1 %); the output's guard bands must stay intact."""
    from torch_utils.ops import conv2d_mfma16
    (n, c), (h, w) = nc, hw
    kw = POSTS[post]
    gen = torch.Generator().manual_seed(17)
    x = (torch.randn([n, c, h, w], generator=gen) * 2 + 0.5).to(dtype)
    mean = torch.randn([n * c], generator=gen) * 0.5
    rstd = torch.rand([n * c], generator=gen) + 0.25
    # gamma, beta: most elements O(1), a few per cent large enough to reach the clamp (181)
    big = (torch.rand([n, 2 * c, h, w], generator=gen) < 0.03).float() * 300
    gb = (torch.randn([n, 2 * c, h, w], generator=gen) * (1 + big)).to(dtype)
    guard = 1024
    flat = torch.full([n * h * w * c + 2 * guard], 7.5, dtype=dtype, device=DEV)
    y = flat[guard:guard + n * h * w * c].view(n, h, w, c).permute(0, 3, 1, 2)
    out = conv2d_mfma16.spade_combine16(_cl(x), mean.to(DEV), rstd.to(DEV), _cl(gb), y=y, **kw)
    assert out.data_ptr() == y.data_ptr()
    assert bool((flat[:guard] == 7.5).all()) and bool((flat[guard + n * h * w * c:] == 7.5).all())
    got = y.cpu().double()
    v = (x.double() - mean.double().view(n, c, 1, 1)) * rstd.double().view(n, c, 1, 1) * (1 + gb[:, :c].double()) + gb[:, c:].double()
    if kw['act'] == 'relu':
        v = v.clamp(min=0)
    v = v * float(np.float32(kw['gain']))
    keep = torch.ones_like(v, dtype=torch.bool)
    if kw['clamp'] is not None:
        cl = float(np.float32(kw['clamp']))
        ulp = 2 * ROUNDOFF[dtype] * 2.0 ** math.floor(math.log2(cl))
        keep = (v.abs() - cl).abs() > ulp
        assert int((v.abs() > cl + ulp).sum()) > 0, 'the clamp is never hit'
        v = v.clamp(-cl, cl)
    left_out = 1 - float(keep.float().mean())
    err = (got - v).abs()
    bound = torch.maximum(v.abs() * ROUNDOFF[dtype], torch.full_like(v, SUBNORMAL_HALF[dtype]))
    worst = float((err / bound)[keep].max())
    print(f'combine {dtype} N{n} C{c} {h}x{w} {post}: worst error {worst:.3f} of the unit roundoff, {left_out:.2e} of the elements within one ulp of the clamp')
    assert left_out < 1e-3
    assert worst <= 1.0


def test_new_ops_reject_what_they_do_not_cover():
    from torch_utils.ops import conv2d_mfma16
    from torch_utils.ops._native import NativeOpError
    x = torch.zeros([1, 16, 4, 4], dtype=torch.bfloat16, device=DEV)
    s = torch.zeros([16], device=DEV)
    with pytest.raises(NativeOpError):
        conv2d_mfma16.instance_norm_stats16(x.float())
    with pytest.raises(NativeOpError):
        conv2d_mfma16.instance_norm_stats16(torch.zeros([1, 8, 4, 4], dtype=torch.bfloat16, device=DEV))
    with pytest.raises(NativeOpError):
        conv2d_mfma16.spade_combine16(x, s, s, torch.zeros([1, 16, 4, 4], dtype=torch.bfloat16, device=DEV))
    with pytest.raises(NativeOpError):
        conv2d_mfma16.spade_combine16(x, s, s, torch.zeros([1, 32, 4, 4], dtype=torch.bfloat16, device=DEV), act='tanh')


@pytest.mark.parametrize('spade_channels,res', [(128, 16), (1, 32)], ids=['feat128_16x16', 'parsing_32x32'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_spade_res_block_half_route(monkeypatch, dtype, spade_channels, res):
    """``Spade_ResBlockV4_512`` (C = 32, N = 2) on 16-bit channels-last input: deviation from the float32 module on the same weights at most twice that of
    the restatement from the float32 oracle; the 16-bit convolution, statistics and combine run, the float32 convolution does not."""
    import half_restatement as HR
    from oracle import network_ref as NR
    from training import networks as PN
    from training.synthetic import det_tensor, fill_module_
    from torch_utils.ops import conv2d_mfma, conv2d_mfma16
    ref = fill_module_(NR.Spade_ResBlockV4_512(32, 32, spade_channels=spade_channels), 'half.spade.').eval()
    net = PN.Spade_ResBlockV4_512(32, 32, spade_channels=spade_channels)
    net.load_state_dict(ref.state_dict(), strict=False)
    net = net.to(DEV).eval()
    x = det_tensor('half.spade.x', [2, 32, res, res])
    feat = (det_tensor('half.spade.feat', [2, spade_channels, res, res]) if spade_channels > 1
            else torch.randint(0, 7, [2, 1, res, res], generator=torch.Generator().manual_seed(3)).float())        # a parsing map: labels 0..6
    rd = HR.rounder(dtype)
    with torch.no_grad():
        want = ref(x, feat)
        restated = HR.spade_res_block(ref, rd(x), rd(feat) if spade_channels > 1 else feat, rd)
        fp32 = net(x.to(DEV), feat.to(DEV))
    e_ref = float((restated - want).abs().max())
    calls = dict(conv16=0, stats16=0, combine16=0, conv32=0)

    def counted(mod, name, key):
        real = getattr(mod, name)

        def wrapper(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(mod, name, wrapper)
    counted(conv2d_mfma16, 'conv2d_forward', 'conv16')
    counted(conv2d_mfma16, 'instance_norm_stats16', 'stats16')
    counted(conv2d_mfma16, 'spade_combine16', 'combine16')
    counted(conv2d_mfma, 'conv2d_forward', 'conv32')
    with torch.no_grad():
        x16 = x.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
        f16 = feat.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last) if spade_channels > 1 else feat.to(DEV)
        got = net(x16, f16)
    assert got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last)
    err = float((got.float().cpu() - fp32.cpu()).abs().max())
    print(f'Spade_ResBlockV4_512 {dtype} spade_channels={spade_channels} {res}x{res}: e_ref {e_ref:.3e}, native vs float32 module {err:.3e} (range {float(want.abs().max()):.2f}); calls {calls}')
    assert calls['conv16'] >= 1 and calls['stats16'] >= 1 and calls['combine16'] >= 1 and calls['conv32'] == 0, calls
    assert err <= 2 * e_ref
