"""GPU parity tests of the 16-bit (bf16 / fp16) MFMA convolution (csrc/conv2d_kernel16.h) through its C ABI.

Two kinds of check:
  * EXACT: small-integer inputs and weights make every product and every partial sum exactly representable in fp32
    (and the 16-bit roundings of inputs lossless), so the float32-output mode must equal an fp64 convolution bit for
    bit -- any indexing slip in the packing, the swizzled LDS image, the split-K slices or the phase decomposition
    shows up as an integer-sized error;
  * TOLERANCE: random inputs against an fp64 convolution of the SAME 16-bit-rounded operands; the only error left is
    the fp32 accumulation order and the final rounding to the output dtype:  |err| <= 2^-8 |ref| + tiny for bf16,
    2^-11 |ref| for fp16 (half an ulp each, doubled for the fused residual add).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.bfloat16, torch.float16]
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


@pytest.fixture(scope='module', autouse=True)
def _native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import conv2d_mfma16
    assert conv2d_mfma16._init() is not None


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _ref_conv(x, w, stride=1, padding=0, transposed=False):
    x, w = x.double().cpu(), w.double().cpu()
    if transposed:
        return F.conv_transpose2d(x, w, stride=stride, padding=padding)
    return F.conv2d(x, w, stride=stride, padding=padding)


GEOMS = [  # (kh, kw, stride, pad)
    (3, 3, 1, 1), (1, 1, 1, 0), (2, 2, 1, 1), (2, 1, 1, 0), (1, 2, 1, 0), (3, 3, 2, 1), (3, 3, 2, 0), (3, 3, 1, 0), (3, 3, 1, 2),
]
SHAPES = [  # (n, cin, cout, h, w): ragged tiles, several m-blocks, partial k chunks, odd sizes
    (2, 32, 64, 33, 45), (1, 48, 40, 17, 17), (3, 16, 24, 8, 70), (1, 80, 136, 20, 33),
]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('geom', GEOMS, ids=[f'k{g[0]}x{g[1]}s{g[2]}p{g[3]}' for g in GEOMS])
@pytest.mark.parametrize('shape', SHAPES, ids=[f'n{s[0]}c{s[1]}o{s[2]}_{s[3]}x{s[4]}' for s in SHAPES])
def test_conv16_exact_f32_out(dtype, geom, shape):
    from torch_utils.ops import conv2d_mfma16 as M
    kh, kw, stride, pad = geom
    n, cin, cout, h, w = shape
    if h + 2 * pad < kh or w + 2 * pad < kw:
        pytest.skip('image smaller than the kernel')
    gen = torch.Generator().manual_seed(hash((geom, shape)) & 0xffff)
    x = _ints(gen, [n, cin, h, w], -3, 3)
    wt = _ints(gen, [cout, cin, kh, kw], -2, 2)
    packed, per, _ = M.pack_weight(wt.to(DEV), dtype)
    y = M.conv2d_forward(x.to(DEV, dtype), packed, cout, kh, kw, stride=stride, pad=(pad, pad), out_dtype=torch.float32)
    ref = _ref_conv(x, wt, stride=stride, padding=pad)
    assert y.shape == ref.shape
    assert torch.equal(y.double().cpu(), ref), float((y.double().cpu() - ref).abs().max())


SMALL_SHAPES = [  # (n, cin, cout, h, w, pad): the low-resolution tiles -- 8 x 8 pixels x 128 couts, 16 x 16 x 64 couts (launch16_mt); with and without split-K
    (3, 64, 136, 8, 8, 1), (2, 48, 128, 7, 5, 1), (2, 32, 192, 16, 16, 1), (1, 80, 136, 13, 16, 1), (4, 512, 256, 8, 8, 1), (2, 256, 128, 16, 16, 1),
    (2, 32, 160, 9, 10, 0), (1, 32, 128, 12, 18, 2), (1, 32, 128, 40, 64, 1), (2, 64, 136, 32, 32, 1), (1, 256, 128, 64, 64, 1),
]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', SMALL_SHAPES, ids=[f'n{s[0]}c{s[1]}o{s[2]}_{s[3]}x{s[4]}p{s[5]}' for s in SMALL_SHAPES])
def test_conv16_small_tiles_exact(dtype, shape):
    """Low-resolution layers run dedicated workgroup tiles: small integers, bit for bit against F.conv2d, float32 and 16-bit outputs
    with the full epilogue (the split-K shapes go through the workspace + finish kernel)."""
    from torch_utils.ops import conv2d_mfma16 as M
    n, cin, cout, h, w, pad = shape
    gen = torch.Generator().manual_seed(hash(shape) & 0xffff)
    x = _ints(gen, [n, cin, h, w], -2, 2)
    wt = _ints(gen, [cout, cin, 3, 3], -1, 1) * (torch.rand([cout, cin, 3, 3], generator=gen) < (16.0 / cin))
    packed, _, _ = M.pack_weight(wt.to(DEV), dtype)
    ref = _ref_conv(x, wt, padding=pad)
    y = M.conv2d_forward(x.to(DEV, dtype), packed, cout, 3, 3, pad=(pad, pad), out_dtype=torch.float32)
    assert y.shape == ref.shape and torch.equal(y.double().cpu(), ref), float((y.double().cpu() - ref).abs().max())
    bias = _ints(gen, [cout], -4, 4)
    res = _ints(gen, list(ref.shape), -8, 8)
    nz = _ints(gen, list(ref.shape[2:]), -2, 2)
    y16 = M.conv2d_forward(x.to(DEV, dtype), packed, cout, 3, 3, pad=(pad, pad), bias=bias.to(DEV), noise=nz.to(DEV), act='relu',
                           residual=res.to(DEV, dtype).contiguous(memory_format=torch.channels_last))
    ref16 = (ref + bias.double().reshape(1, -1, 1, 1) + nz.double()).clamp_min(0) + res.double()
    assert float(ref16.abs().max()) <= 256
    assert torch.equal(y16.double().cpu(), ref16), float((y16.double().cpu() - ref16).abs().max())


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', [(2, 32, 64, 33, 45), (1, 64, 32, 40, 40), (2, 16, 8, 16, 16)], ids=['a', 'b', 'c'])
def test_conv16_vector_epilogue_exact(dtype, shape):
    """Channels-last 16-bit output (16-byte stores after the half-wave exchange): sparse small-integer weights keep every
    result an integer of magnitude <= 256, exact in bf16 and fp16."""
    from torch_utils.ops import conv2d_mfma16 as M
    n, cin, cout, h, w = shape
    gen = torch.Generator().manual_seed(7)
    x = _ints(gen, [n, cin, h, w], -1, 1)
    wt = _ints(gen, [cout, cin, 3, 3], -1, 1) * (torch.rand([cout, cin, 3, 3], generator=gen) < 0.1)
    res = _ints(gen, [n, cout, h, w], -8, 8)
    packed, _, _ = M.pack_weight(wt.to(DEV), dtype)
    bias = _ints(gen, [cout], -4, 4)
    r16 = res.to(DEV, dtype).contiguous(memory_format=torch.channels_last)
    y = M.conv2d_forward(x.to(DEV, dtype), packed, cout, 3, 3, pad=(1, 1), bias=bias.to(DEV), residual=r16)
    assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    ref = _ref_conv(x, wt, padding=1) + bias.double().reshape(1, -1, 1, 1) + res.double()
    assert float(ref.abs().max()) <= 256
    assert torch.equal(y.double().cpu(), ref), float((y.double().cpu() - ref).abs().max())


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_conv16_fused_tail_random(dtype):
    """Per-sample (modulated, demodulated) weights + noise + bias + lrelu + gain + clamp + residual on random data."""
    from torch_utils.ops import conv2d_mfma16 as M
    from torch_utils.ops import conv2d_mfma
    n, cin, cout, h, w = 3, 64, 96, 37, 50
    gen = torch.Generator().manual_seed(11)
    x = torch.randn([n, cin, h, w], generator=gen).to(dtype)
    wt = torch.randn([cout, cin, 3, 3], generator=gen)
    styles = torch.randn([n, cin], generator=gen) + 1
    noise = torch.randn([h, w], generator=gen)
    bias = torch.randn([cout], generator=gen)
    res = torch.randn([n, cout, h, w], generator=gen).to(dtype)
    dco = conv2d_mfma.modconv_dcoefs(wt.to(DEV), styles.to(DEV))
    packed, per, _ = M.pack_weight(wt.to(DEV), dtype, styles=styles.to(DEV), dcoefs=dco)
    assert per > 0
    y = M.conv2d_forward(x.to(DEV), packed, cout, 3, 3, pad=(1, 1), sample_stride=per, noise=noise.to(DEV), noise_gain=0.3, bias=bias.to(DEV),
                         act='lrelu', alpha=0.2, gain=np.sqrt(2), clamp=2.5, residual=res.to(DEV).contiguous(memory_format=torch.channels_last))
    # reference on the same rounded operands: the per-sample weights exactly as the kernel sees them
    wmod = (wt.double()[None] * styles.double()[:, None, :, None, None])
    d = (wmod.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()
    assert torch.allclose(d.float(), dco.cpu(), rtol=1e-5)
    w16 = ((wt[None] * styles[:, None, :, None, None]) * dco.cpu()[:, :, None, None, None]).to(dtype).double()
    ref = torch.stack([F.conv2d(x[i:i + 1].double(), w16[i], padding=1)[0] for i in range(n)])
    ref = ref + noise.double() * 0.3 + bias.double().reshape(1, -1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * 0.2) * np.sqrt(2)
    ref = ref.clamp(-2.5, 2.5) + res.double()
    err = (y.double().cpu() - ref).abs()
    bound = 2 * ULP[dtype] * ref.abs() + 1e-3
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('hw', [(8, 8), (16, 16), (13, 21)], ids=['8', '16', '13x21'])
def test_conv16_transposed_phases_exact(dtype, hw):
    """Stride-2 transposed 3x3 convolution as four gather-form phase launches == conv_transpose2d."""
    from torch_utils.ops import conv2d_mfma16 as M
    n, cin, cout = 2, 32, 48
    h, w = hw
    gen = torch.Generator().manual_seed(3)
    x = _ints(gen, [n, cin, h, w], -3, 3)
    wt = _ints(gen, [cin, cout, 3, 3], -2, 2)          # IOHW
    out_hw = ((h - 1) * 2 + 3, (w - 1) * 2 + 3)
    phases = M.pack_transposed(wt.to(DEV), dtype, 2, (0, 0), (h, w), out_hw)
    assert phases is not None and len(phases) == 4
    # float32 view of the result through the scalar path: run each phase into a float32 NCHW tensor
    y = torch.zeros([n, cout, *out_hw], dtype=torch.float32, device=DEV)
    xd = x.to(DEV, dtype)
    for ph, packed, per in phases:
        M.conv2d_forward(xd, packed, cout, len(ph['ky']), len(ph['kx']), pad=ph['pad'], out_hw=ph['out_hw'], y=y, out_step=(2, 2), out_off=ph['off'],
                         out_dtype=torch.float32)
    ref = _ref_conv(x, wt, stride=2, transposed=True)
    assert torch.equal(y.double().cpu(), ref), float((y.double().cpu() - ref).abs().max())
    # and the 16-bit channels-last form on a value range that stays exact
    y16 = M.conv_transpose2d_forward((x.sign()).to(DEV, dtype), M.pack_transposed((wt.sign() * (wt.abs() > 1)).to(DEV), dtype, 2, (0, 0), (h, w), out_hw), cout, out_hw)
    ref16 = _ref_conv(x.sign(), wt.sign() * (wt.abs() > 1), stride=2, transposed=True)
    assert float(ref16.abs().max()) <= 256
    assert torch.equal(y16.double().cpu(), ref16)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_conv16_splitk_exact(dtype):
    """Low-resolution wide layers take the split-K route (few tiles, long K): same integers, bit for bit."""
    from torch_utils.ops import conv2d_mfma16 as M
    n, cin, cout, h, w = 1, 512, 128, 8, 8
    lib = M._init()
    assert lib.pg_conv2d16_splitk_plan(n, cin, h, w, cout, 3, 3, 1) > 1
    gen = torch.Generator().manual_seed(5)
    x = _ints(gen, [n, cin, h, w], -2, 2)
    wt = _ints(gen, [cout, cin, 3, 3], -1, 1)
    bias = _ints(gen, [cout], -3, 3)
    packed, _, _ = M.pack_weight(wt.to(DEV), dtype)
    y = M.conv2d_forward(x.to(DEV, dtype), packed, cout, 3, 3, pad=(1, 1), bias=bias.to(DEV), out_dtype=torch.float32)
    ref = _ref_conv(x, wt, padding=1) + bias.double().reshape(1, -1, 1, 1)
    assert torch.equal(y.double().cpu(), ref)
    y16 = M.conv2d_forward(x.to(DEV, dtype), packed, cout, 3, 3, pad=(1, 1), bias=bias.to(DEV), act='relu', clamp=200.0)
    ref16 = ref.clamp(0, 200)
    err = (y16.double().cpu() - ref16).abs()
    assert bool((err <= ULP[dtype] * ref16.abs()).all())
    # the vectorised finish with every epilogue stage, written into one phase of a 2x larger channels-last output
    osc = (_ints(gen, [n, cout], 1, 2) / 2)
    nz = _ints(gen, [h, w], -2, 2)
    big = torch.zeros([n, cout, 2 * h, 2 * w], device=DEV, dtype=dtype).contiguous(memory_format=torch.channels_last)
    res = _ints(gen, [n, cout, 2 * h, 2 * w], -4, 4)
    M.conv2d_forward(x.to(DEV, dtype), packed, cout, 3, 3, pad=(1, 1), out_hw=(h, w), y=big, out_step=(2, 2), out_off=(1, 0), out_scale=osc.to(DEV),
                     noise=nz.to(DEV), bias=bias.to(DEV), act='lrelu', alpha=0.25, gain=2.0, clamp=300.0,
                     residual=res.to(DEV, dtype).contiguous(memory_format=torch.channels_last))
    v = _ref_conv(x, wt, padding=1) * osc.double().reshape(n, cout, 1, 1) + nz.double() + bias.double().reshape(1, -1, 1, 1)
    v = (torch.where(v > 0, v, v * 0.25) * 2.0).clamp(-300, 300) + res.double()[:, :, 1::2, 0::2]
    got = big.double().cpu()
    err = (got[:, :, 1::2, 0::2] - v).abs()
    assert bool((err <= 2 * ULP[dtype] * v.abs() + 1e-6).all())
    assert float(got[:, :, 0::2].abs().max()) == 0 and float(got[:, :, 1::2, 1::2].abs().max()) == 0


PHASE_SHAPES = [  # (n, cin, cout, h, w): cout 32 (one 32-cout block per phase), 64 / 128 (64-cout blocks), low resolution (small tiles, split-K), ragged images
    (2, 32, 32, 40, 36), (2, 48, 64, 33, 20), (1, 64, 128, 16, 16), (3, 256, 128, 8, 8), (2, 512, 64, 16, 16), (1, 32, 192, 9, 70),
]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', PHASE_SHAPES, ids=[f'n{s[0]}c{s[1]}o{s[2]}_{s[3]}x{s[4]}' for s in PHASE_SHAPES])
def test_conv16_four_phase_launch(dtype, shape):
    """The four phase kernels of an up-by-2 layer stacked along Cout and launched once (pg_conv2d16_fusion::phase_cout) == four
    launches with out_step / out_off, with per-sample weights, demodulation scale, phase-major noise, bias, lrelu, gain and clamp:
    small integers, so both are exact and must agree bit for bit (also through split-K, whose share count differs)."""
    from torch_utils.ops import conv2d_mfma16 as M
    n, cin, cout, h, w = shape
    gen = torch.Generator().manual_seed(hash(shape) & 0xffff)
    x = _ints(gen, [n, cin, h, w], -2, 2).to(DEV, dtype)
    ws = [_ints(gen, [cin, cout, 3, 3], -1, 1) * (torch.rand([cin, cout, 3, 3], generator=gen) < (12.0 / cin)) for _ in range(4)]
    styles = _ints(gen, [n, cin], 1, 2).to(DEV)
    osc = (_ints(gen, [n, cout], 1, 2) / 2).to(DEV)
    bias = _ints(gen, [cout], -3, 3).to(DEV)
    noise = _ints(gen, [1, 2, 2, h, w], -2, 2).to(DEV)
    ep = dict(bias=bias, act='lrelu', alpha=0.25, gain=2.0, clamp=240.0)
    ref = torch.zeros([n, cout, 2 * h, 2 * w], device=DEV, dtype=dtype).contiguous(memory_format=torch.channels_last)
    for g, (a, b) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        packed, per, _ = M.pack_weight(ws[g].to(DEV), dtype, transpose_oi=True, styles=styles)
        M.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), out_hw=(h, w), y=ref, out_step=(2, 2), out_off=(a, b), sample_stride=per, out_scale=osc,
                         noise=noise[:, a, b].contiguous(), **ep)
    packed, per, _ = M.pack_weight(torch.cat(ws, dim=1).to(DEV), dtype, transpose_oi=True, styles=styles)
    got = torch.full_like(ref, 7.0)
    M.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), out_hw=(h, w), y=got, sample_stride=per, out_scale=osc, noise=noise, phases=True, **ep)
    assert float(ref.float().abs().max()) > 4
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), float((got.float() - ref.float()).abs().max())


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_pack_weight_grouped_matches_single_packs(dtype):
    """One launch for the four composite phase kernels of an up-by-2 modulated convolution == four separate packs, bit for bit."""
    from torch_utils.ops import conv2d_mfma16 as M
    gen = torch.Generator().manual_seed(11)
    g, cin, cout, n = 4, 40, 72, 3
    ws = torch.randn([g, cin, cout, 3, 3], generator=gen).to(DEV)
    styles = torch.randn([n, cin], generator=gen).to(DEV)
    dcoefs = torch.rand([n, cout], generator=gen).to(DEV) + 0.5
    packed, per = M.pack_weight_grouped(ws, dtype, transpose_oi=True, styles=styles, dcoefs=dcoefs)
    for i in range(g):
        single, per1, _ = M.pack_weight(ws[i], dtype, transpose_oi=True, styles=styles, dcoefs=dcoefs)
        assert per1 == per and torch.equal(packed[i].view(torch.int16), single.view(torch.int16))
    packed, per = M.pack_weight_grouped(ws.transpose(1, 2).contiguous(), dtype, flip=True)
    for i in range(g):
        single, per1, _ = M.pack_weight(ws[i].transpose(0, 1).contiguous(), dtype, flip=True)
        assert per == per1 == 0 and torch.equal(packed[i].view(torch.int16), single.view(torch.int16))


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_conv16_full_size_properties(dtype):
    """BASELINE config-5 size (N=4, 32 channels, 1024^2): linearity in the input and the delta-kernel identity, which
    need no reference at that size."""
    from torch_utils.ops import conv2d_mfma16 as M
    n, c, r = 4, 32, 1024
    gen = torch.Generator().manual_seed(9)
    x = _ints(gen, [n, c, r, r], -4, 4).to(DEV, dtype).contiguous(memory_format=torch.channels_last)
    delta = torch.zeros([c, c, 3, 3])
    delta[torch.arange(c), torch.arange(c), 1, 1] = 1
    pk, _, _ = M.pack_weight(delta.to(DEV), dtype)
    y = M.conv2d_forward(x, pk, c, 3, 3, pad=(1, 1))
    assert torch.equal(y, x)
    wt = _ints(gen, [c, c, 3, 3], -1, 1) * (torch.rand([c, c, 3, 3], generator=gen) < 0.15)
    pw, _, _ = M.pack_weight(wt.to(DEV), dtype)
    a = M.conv2d_forward(x, pw, c, 3, 3, pad=(1, 1), out_dtype=torch.float32)
    b = M.conv2d_forward(x + x, pw, c, 3, 3, pad=(1, 1), out_dtype=torch.float32)
    assert torch.equal(b, a + a)
    # a crop against the reference convolution
    ref = _ref_conv(x[:1, :, :40, :40].float(), wt, padding=1)[:, :, :38, :38]
    assert torch.equal(a[:1, :, :38, :38].double().cpu(), ref)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', [(2, 64, 33, 47), (2, 512, 8, 8), (3, 256, 16, 24), (4, 1024, 4, 4), (1, 136, 9, 7),
                                   (2, 32, 256, 260), (1, 64, 300, 256), (1, 128, 320, 258), (1, 256, 200, 200), (1, 512, 128, 130), (2, 1024, 48, 50), (1, 1024, 96, 90), (1, 776, 20, 22),
                                   (4, 32, 62, 66), (4, 1024, 16, 16)],
                         ids=['one_lane', 'sixteen_lanes', 'four_lanes', 'tiny', 'ragged_groups', 'lp4_u4', 'lp8_u8', 'lp16_u16', 'lp32_u16', 'lp64_u16', 'lp64_u4_k2', 'lp64_u8_k2', 'lp64_ragged_k2',
                              'lp4_small_image', 'lp64_u1_k2'])
def test_conv1x1_small_head(dtype, shape):
    """The 16-bit ToRGB / parsing head against float64.  Three output channels run the round-5 form (csrc/conv1x1_head16.hip: Cin / 8 lanes share a pixel, reduce-scatter over
    shuffles, the half-resolution skip's neighbour column from the neighbour lane) -- the `lp*` cases name its (lanes per pixel, pixels per lane group, channel passes) variants, with
    widths that are no multiple of 64 so that wave passes cross image rows; seven channels run the first form (one streaming pass; 1, 4 or 16 lanes per pixel depending on the image size)."""
    from torch_utils.ops import conv2d_mfma16 as M
    n, cin, h, w = shape
    gen = torch.Generator().manual_seed(13)
    x = torch.randn([n, cin, h, w], generator=gen).to(dtype)
    for cout in (3, 7):
        wt = torch.randn([cout, cin, 1, 1], generator=gen)
        styles = torch.randn([n, cin], generator=gen)
        bias = torch.randn([cout], generator=gen)
        skip = torch.randn([n, cout, h, w], generator=gen)
        y = M.conv1x1_small(x.to(DEV), wt.to(DEV), styles.to(DEV), bias.to(DEV), skip.to(DEV), clamp=3.0)
        wm = wt.double()[None, :, :, 0, 0] * styles.double()[:, None, :]
        ref = torch.einsum('nchw,noc->nohw', x.double(), wm) + bias.double().reshape(1, -1, 1, 1)
        ref = ref.clamp(-3, 3) + skip.double()
        assert float((y.double().cpu() - ref).abs().max()) <= 2e-4 * max(1.0, (cin / 64) ** 0.5)
        if h % 2 == 0 and w % 2 == 0:      # the skip image handed over at half resolution, up-sampled in the same pass ([1, 3, 3, 1], as upsample2d does)
            from torch_utils.ops import upfirdn2d
            lo = torch.randn([n, cout, h // 2, w // 2], generator=gen)
            f = upfirdn2d.setup_filter([1, 3, 3, 1])
            up = upfirdn2d.upsample2d(lo, f)                      # the CPU route of the op (pinned against the goldens)
            y2 = M.conv1x1_small(x.to(DEV), wt.to(DEV), styles.to(DEV), bias.to(DEV), lo.to(DEV), clamp=3.0, skip_up2=True)
            ref2 = (ref - skip.double()) + up.double()
            assert float((y2.double().cpu() - ref2).abs().max()) <= 2e-4 * max(1.0, (cin / 64) ** 0.5)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_conv2d_gradfix_16bit_routes_and_grads(dtype):
    """conv2d_gradfix on half-precision tensors: native forward (also for a channel count that needs padding), native
    input gradient, against PyTorch's own convolution in fp32 on the same rounded operands."""
    from torch_utils.ops import conv2d_gradfix
    gen = torch.Generator().manual_seed(17)
    for cin, cout, k, stride, pad, transposed in ((6, 32, 1, 1, 0, False), (32, 48, 3, 1, 1, False), (32, 32, 3, 2, 1, False), (32, 16, 3, 2, 0, True)):
        x = torch.randn([2, cin, 20, 24], generator=gen).to(DEV, dtype).requires_grad_(True)
        wshape = [cin, cout, k, k] if transposed else [cout, cin, k, k]
        wt = (torch.randn(wshape, generator=gen) / np.sqrt(cin * k * k)).to(DEV, dtype).requires_grad_(True)
        op = conv2d_gradfix.conv_transpose2d if transposed else conv2d_gradfix.conv2d
        y = op(x, wt, stride=stride, padding=pad)
        x32, w32 = x.detach().float().requires_grad_(True), wt.detach().float().requires_grad_(True)
        ref = (F.conv_transpose2d if transposed else F.conv2d)(x32, w32, stride=stride, padding=pad)
        assert y.dtype == dtype and y.shape == ref.shape
        tol = 2 * ULP[dtype]
        assert float((y.detach().float() - ref.detach()).abs().max()) <= tol * float(ref.abs().max()) + 1e-3
        dy = torch.randn(ref.shape, generator=gen).to(DEV, dtype)
        gx, gw = torch.autograd.grad(y, [x, wt], dy)
        rx, rw = torch.autograd.grad(ref, [x32, w32], dy.float())
        assert float((gx.float() - rx).abs().max()) <= tol * float(rx.abs().max()) + 1e-3
        assert float((gw.float() - rw).abs().max()) <= 4 * tol * float(rw.abs().max()) + 1e-2


# ---------------------------------------------------------------- the half-precision stack (BASELINE config 5) vs the fp32 oracle

@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_synthesis_stack_half_vs_oracle(dtype):
    """SynthesisStack (config 5's network at reduced size: 128^2, channels 256..32) entirely in 16-bit against the float32
    CPU oracle.  Tolerance: every layer rounds its activations to the 16-bit type (2^-8 relative for bf16, 2^-11 for fp16)
    and ~12 layers stack up -> 3e-2 / 4e-3 of the output range ('bf16 tolerance ~1e-2 rel')."""
    from detgen import det_tensor, fill_module_
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(w_dim=64, img_resolution=128, img_channels=3, channel_base=4096, channel_max=256, conv_clamp=256)
    ref = fill_module_(NR.SynthesisStack(**kw), 'stack.').eval()
    net = PN.SynthesisStack(num_fp16_res=5, half_dtype=dtype, **kw)
    missing, unexpected = net.load_state_dict(ref.state_dict(), strict=False)
    assert not unexpected and all('resample_filter' in k for k in missing), (missing, unexpected)
    net = net.to(DEV).eval()
    ws = det_tensor('stack.ws', [2, net.num_ws, 64])
    assert net.num_ws == ref.num_ws
    with torch.no_grad():
        got = net(ws.to(DEV), noise_mode='const').cpu()
        want = ref(ws, noise_mode='const')
    assert got.dtype == torch.float32 and got.shape == want.shape == (2, 3, 128, 128)
    err = float((got - want).abs().max()) / float(want.abs().max())
    assert err <= (3e-2 if dtype == torch.bfloat16 else 4e-3), err
    # and the same network in float32 through the fp32 kernels: tight
    with torch.no_grad():
        got32 = net(ws.to(DEV), noise_mode='const', force_fp32=True).cpu()
    assert float((got32 - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_config5_stack_full_width_prefix_vs_oracle():
    """The network bench.py --mode bf16_1024 times (channel_base 32768, channel_max 1024, bf16 everywhere, N = 4) on its 8^2..256^2
    prefix -- the same blocks with the same channel widths (1024, 1024, 1024, 512, 256, 128) as the 1024^2 stack -- against the
    float32 CPU oracle stack (the benched widths were only covered at 128^2 / <= 256 channels).  Same bar as the
    reduced-size test: bf16 rounds every activation to 2^-8 relative, ~12 layers deep -> 3e-2 of the output range; the fp32 route
    of the same network must be tight."""
    from detgen import fill_module_
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(w_dim=512, img_resolution=256, img_channels=3, channel_base=32768, channel_max=1024, conv_clamp=256)
    ref = fill_module_(NR.SynthesisStack(**kw), 'cfg5.').eval()
    net = PN.SynthesisStack(num_fp16_res=8, half_dtype=torch.bfloat16, **kw)
    missing, unexpected = net.load_state_dict(ref.state_dict(), strict=False)
    assert not unexpected and all('resample_filter' in k for k in missing), (missing, unexpected)
    net = net.to(DEV).eval()
    assert [net.block_resolutions[0], net.block_resolutions[-1]] == [8, 256] if hasattr(net, 'block_resolutions') else True
    n = 4
    ws = torch.randn([n, net.num_ws, 512], generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        got = net(ws.to(DEV), noise_mode='const').cpu()
        got32 = net(ws.to(DEV), noise_mode='const', force_fp32=True).cpu()
        want = ref(ws, noise_mode='const')
    assert got.shape == want.shape == (n, 3, 256, 256)
    rng = float(want.abs().max())
    err16, err32 = float((got - want).abs().max()) / rng, float((got32 - want).abs().max()) / rng
    print(f'config 5 prefix (8^2..256^2, channel_max 1024, N=4): bf16 {err16:.2e}, fp32 route {err32:.2e} of the output range {rng:.1f}')
    assert err16 <= 3e-2, err16
    assert err32 <= 1e-4, err32


UP2F_SHAPES = [  # (n, cin, cout, h, w): one tile; ragged tiles in both axes (W not a multiple of 30, H not of 16); several cout blocks; wider than two tiles
    (1, 32, 32, 16, 30), (2, 48, 64, 21, 37), (1, 64, 96, 9, 64), (2, 32, 32, 40, 95),
]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', UP2F_SHAPES, ids=[f'n{s[0]}c{s[1]}o{s[2]}_{s[3]}x{s[4]}' for s in UP2F_SHAPES])
@pytest.mark.parametrize('taps', [[1, 3, 3, 1], [1, 2, 4, 1]], ids=['f1331', 'fasym'])      # (tap sums are powers of two: the normalised taps stay exact)
def test_up2_fused_x_kernel_vs_float64(dtype, shape, taps):
    """pg_conv2d16_up2_fused (csrc/conv2d_up2f16.h: y half of the FIR in the weights, x half in the epilogue over DPP wave shifts) against the reference's
    two-step form in float64 -- conv_transpose2d(stride 2) -> (2H+1) x (2W+1), then upfirdn2d(f, padding 1, gain 4) (conv2d_resample.py:125-142) -- on
    small-integer operands: every product and partial sum of the kernel is exact in fp32, so the only error left is the final rounding to 16 bits
    (half an ulp).  The asymmetric filter pins the orientation of both filter halves; with noise, bias, demodulation scale, lrelu, gain and clamp."""
    from torch_utils.ops import conv2d_mfma16 as M
    from training import networks as PN
    from oracle import ops_ref
    n, cin, cout, h, w = shape
    gen = torch.Generator().manual_seed(17)
    x = _ints(gen, [n, cin, h, w], -2, 2)
    wt = _ints(gen, [cin, cout, 3, 3], -2, 2)                     # IOHW: what conv_transpose2d takes
    f1 = torch.tensor(taps, dtype=torch.float64)
    f2d = torch.outer(f1, f1) / f1.sum() ** 2                      # upfirdn2d.setup_filter's normalised outer product
    fy, fx = PN._separable_taps(f2d.float())
    stack = PN._up2_fused_weights(wt.to(DEV), fy)
    assert tuple(stack.shape) == (cin, 4 * cout, 3, 2)
    packed, per, _ = M.pack_weight(stack, dtype, transpose_oi=True)
    scale = (_ints(gen, [n, cout], 1, 4) / 4).to(DEV)
    bias = _ints(gen, [cout], -3, 3).to(DEV)
    noise = _ints(gen, [1, 1, 2 * h, 2 * w], -2, 2)
    noise_ph = noise.reshape(1, h, 2, w, 2).permute(0, 2, 4, 1, 3).contiguous().to(DEV)
    y = M.conv_up2_fused(x.to(DEV, dtype), packed, cout, [2.0 * float(v) for v in fx], sample_stride=per, out_scale=scale, noise=noise_ph, noise_gain=0.5,
                         bias=bias, act='lrelu', alpha=0.25, gain=2.0, clamp=64.0)
    assert tuple(y.shape) == (n, cout, 2 * h, 2 * w) and y.is_contiguous(memory_format=torch.channels_last)
    z = _ref_conv(x, wt, stride=2, transposed=True)                # [n, cout, 2h+1, 2w+1] float64
    ref = ops_ref.upfirdn2d(z, f2d, padding=1, gain=4)
    ref = ref * scale.double().cpu()[:, :, None, None] + 0.5 * noise.double() + bias.double().cpu()[None, :, None, None]
    ref = torch.where(ref > 0, ref, 0.25 * ref) * 2.0
    ref = ref.clamp(-64.0, 64.0)
    err = (y.double().cpu() - ref).abs()
    bound = ULP[dtype] * ref.abs() + 1e-6
    assert bool((err <= bound).all()), (float((err - bound).max()), float(ref.abs().max()))
    # per-sample packs (the fused modulated convolution, networks.py:85-94): styles * dcoefs folded into the pack == the same result with the scale in the weights
    styles = (_ints(gen, [n, cin], 1, 2)).to(DEV)
    packed_n, per_n, _ = M.pack_weight(stack, dtype, transpose_oi=True, styles=styles)
    y2 = M.conv_up2_fused(x.to(DEV, dtype), packed_n, cout, [2.0 * float(v) for v in fx], sample_stride=per_n)
    z2 = torch.stack([_ref_conv(x[i:i + 1], wt * styles.cpu()[i][:, None, None, None], stride=2, transposed=True)[0] for i in range(n)])
    ref2 = ops_ref.upfirdn2d(z2, f2d, padding=1, gain=4)
    err2 = (y2.double().cpu() - ref2).abs()
    assert bool((err2 <= ULP[dtype] * ref2.abs() + 1e-6).all()), float(err2.max())


@pytest.mark.parametrize('policy', ['composite', 'merged', 'auto', 'fusedx'])
def test_up2_layer_routes_vs_oracle(policy, monkeypatch):
    """The three routes of a weight-dominated 16-bit `up = 2` SynthesisLayer (1024 -> 512 at 32^2 -> 64^2, N = 2, bf16): composite 6x6 kernels (round 2),
    the transposed convolution's phases as ONE launch of 2x2 kernels + the channels-last FIR on a pitched view (round 4, `merged`), four phase launches +
    FIR (`auto`) -- each against the float32 oracle layer (networks.py:73-94 + conv2d_resample.py:125-142).  bf16 bar: 2e-2 of the output range."""
    from detgen import det_tensor, fill_module_
    from training import networks as PN
    from oracle import network_ref as NR
    monkeypatch.setenv('PG_UP2_POLICY', 'composite' if policy == 'fusedx' else policy)
    monkeypatch.setenv('PG_UP2_FUSEDX', '1' if policy == 'fusedx' else '0')         # round 5: y half of the FIR in the weights, x half in the epilogue (one launch)
    kw = dict(w_dim=64, resolution=64, up=2, conv_clamp=256)
    ref = fill_module_(NR.SynthesisLayer(1024, 512, **kw), 'up2r.').eval()
    net = PN.SynthesisLayer(1024, 512, **kw)
    net.load_state_dict(ref.state_dict(), strict=False)
    net = net.to(DEV).eval()
    x = det_tensor('up2r.x', [2, 1024, 32, 32])
    ws = det_tensor('up2r.ws', [2, 64])
    with torch.no_grad():
        want = ref(x, ws, noise_mode='const')
        got = net(x.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last), ws.to(DEV), noise_mode='const').float().cpu()
    assert got.shape == want.shape == (2, 512, 64, 64)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f'up=2 layer 1024->512 32^2, bf16, route {policy}: {err:.2e} of the output range')
    assert err <= 2e-2, err


@pytest.mark.parametrize('n', [1, 4], ids=['n1', 'benched_batch_n4'])
def test_config5_stack_full_1024_vs_oracle(n):
    """(`benched_batch_n4`, round 5 -- VERDICT r4: the benched batch was only compared up to 256^2: four samples with their own latents, i.e. the per-sample and the shared
    weight-pack routes as the bench runs them.)  The WHOLE network of bench.py --mode bf16_1024 -- 8^2 .. 1024^2, channel_base 32768, channel_max 1024, i.e. including the 512^2 (64-channel)
    and 1024^2 (32-channel) blocks that carry ~60 % of its flops and that the prefix test above stops short of -- at N = 1
    against the float32 CPU oracle stack run right here (340 GFLOP: seconds on the GPU box's host; the oracle, not the reference, is the source
    because the reference's class is hard-wired to 512^2).  bf16 everywhere: 3e-2 of the output range (the bar of the
    reduced-size tests: ~16 layers each rounding to 2^-8); the fp32 route of the same network: 1e-4."""
    import os
    from detgen import fill_module_
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(w_dim=512, img_resolution=1024, img_channels=3, channel_base=32768, channel_max=1024, conv_clamp=256)
    ref = fill_module_(NR.SynthesisStack(**kw), 'cfg5.').eval()
    net = PN.SynthesisStack(num_fp16_res=8, half_dtype=torch.bfloat16, **kw)
    missing, unexpected = net.load_state_dict(ref.state_dict(), strict=False)
    assert not unexpected and all('resample_filter' in k for k in missing), (missing, unexpected)
    net = net.to(DEV).eval()
    ws = torch.randn([n, net.num_ws, 512], generator=torch.Generator().manual_seed(1))
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    with torch.no_grad():
        got = net(ws.to(DEV), noise_mode='const').cpu()
        got32 = net(ws.to(DEV), noise_mode='const', force_fp32=True).cpu()
        want = ref(ws, noise_mode='const')
    assert got.shape == want.shape == (n, 3, 1024, 1024)
    rng = float(want.abs().max())
    err16, err32 = float((got - want).abs().max()) / rng, float((got32 - want).abs().max()) / rng
    print(f'config 5 full stack (8^2..1024^2, channel_max 1024, N={n}): bf16 {err16:.2e}, fp32 route {err32:.2e} of the output range {rng:.1f}')
    assert err16 <= 3e-2, err16
    assert err32 <= 1e-4, err32


def test_upfirdn2d_channels_last_kernel():
    """The channels-last FIR (blur / 2x decimation / 2x zero-insertion up-sampling, with and without the fused tail) against the NCHW kernel's result."""
    from torch_utils.ops import upfirdn2d
    gen = torch.Generator().manual_seed(21)
    f = upfirdn2d.setup_filter([1, 3, 3, 1]).to(DEV)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        x = torch.randn([2, 16, 37, 45], generator=gen).to(DEV, dtype)
        xcl = x.contiguous(memory_format=torch.channels_last)
        for kw in (dict(padding=[1, 1, 1, 1], gain=4), dict(down=2, padding=[1, 1, 1, 1]), dict(padding=[2, 2, 2, 2]), dict(down=2, padding=[0, 1, 2, 0]),
                   dict(up=2, padding=[2, 1, 2, 1], gain=4), dict(up=2, padding=[1, 2, 0, 3], flip_filter=True), dict(up=2, padding=[3, 3, 3, 3])):     # up = 2: the gradient of the 2x decimation
            a = upfirdn2d.upfirdn2d(xcl, f, **kw)
            b = upfirdn2d.upfirdn2d(x.float(), f, **kw)
            assert a.is_contiguous(memory_format=torch.channels_last) and a.shape == b.shape
            tol = 0 if dtype == torch.float32 else ULP[dtype]
            assert float((a.float() - b).abs().max()) <= tol * float(b.abs().max()) + 1e-5
        noise, bias = torch.randn([37 - 1, 45 - 1], generator=gen).to(DEV), torch.randn([16], generator=gen).to(DEV)
        fused = upfirdn2d.upfirdn2d_bias_act(xcl, f, padding=[1, 1, 1, 1], gain=4, noise=noise, b=bias, act='lrelu', alpha=0.2, act_gain=1.4, clamp=3.0)
        ref = upfirdn2d.upfirdn2d(x.float(), f, padding=[1, 1, 1, 1], gain=4) + noise + bias.reshape(1, -1, 1, 1)
        ref = (torch.where(ref > 0, ref, ref * 0.2) * 1.4).clamp(-3, 3)
        assert fused is not None and fused.dtype == dtype
        assert float((fused.float() - ref).abs().max()) <= (1e-5 if dtype == torch.float32 else ULP[dtype] * 3.0 + 1e-5)


@pytest.mark.gpu
def test_graphed_forward_replays_the_stack():
    """training/graphed.py: one hipGraph replay == the eager forward, bit for bit, also for inputs the graph was not captured with
    (per-sample weight packing and demodulation are kernels of the graph, not baked constants)."""
    from training import networks
    from training.graphed import GraphedForward
    from detgen import fill_module_
    net = fill_module_(networks.SynthesisStack(w_dim=64, img_resolution=64, img_channels=3, channel_base=1024, channel_max=64, num_fp16_res=4,
                                               half_dtype=torch.bfloat16, conv_clamp=256), 'graph.').to(DEV).eval()
    gen = torch.Generator().manual_seed(5)
    ws_a = torch.randn([2, net.num_ws, 64], generator=gen).to(DEV)
    ws_b = torch.randn([2, net.num_ws, 64], generator=gen).to(DEV)
    with torch.no_grad():
        eager_a, eager_b = net(ws_a, noise_mode='const').clone(), net(ws_b, noise_mode='const').clone()
    fwd = GraphedForward(lambda w_: net(w_, noise_mode='const'), [ws_a])
    assert torch.equal(fwd(ws_a), eager_a)
    assert torch.equal(fwd(ws_b), eager_b)
    assert torch.equal(fwd(ws_a), eager_a)
    assert not torch.equal(eager_a, eager_b)


# (layer, form, shared) of the 128^2 stack below, worked out on the CPU from the 16-bit route rules: the low resolutions share one weight pack, the high ones pack per sample
_BATCH_PLAN = [('b8.conv1', 'up1', True), ('b16.conv0', 'composite x1', True), ('b16.conv1', 'up1', True), ('b32.conv0', 'composite x1', True), ('b32.conv1', 'up1', False),
               ('b64.conv0', 'fused-x', True), ('b64.conv1', 'up1', False), ('b128.conv0', 'fused-x', False), ('b128.conv1', 'up1', False)]


@pytest.mark.parametrize('fusedx', ['1', '0'], ids=['fusedx', 'composite'])
def test_stack_batched_preparation_matches_the_layers(fusedx, monkeypatch):
    """SynthesisStack._prepare_all packs the per-sample weights of the whole stack in one launch, by its own reading of each layer's route; a layer whose reading
    differs packs again and nothing else notices.  On a 128^2 bf16 stack (widths 64, 64, 64, 64, 32; N = 2) that holds every batched kind -- shared-pack layers,
    per-sample up = 1 layers, a per-sample fused-x layer (b128.conv0: 32 * 24 <= 64 * 64) and, with PG_UP2_FUSEDX=0, the same layer as a per-sample composite in
    one launch (32 * 36 <= 64 * 64) --:  the plan the layers follow when they pack for themselves is the one worked out above; the batch holds exactly its
    per-sample layers; no layer packs a 3x3 / 3x2 kernel per sample during the batched forward; both registries are empty when the forward clears them; and the
    image equals the unbatched one bit for bit (same kernels, same operands)."""
    from detgen import fill_module_
    from training import networks as PN
    from torch_utils.ops import conv2d_mfma, conv2d_mfma16 as M
    monkeypatch.setenv('PG_UP2_FUSEDX', fusedx)
    net = fill_module_(PN.SynthesisStack(w_dim=64, img_resolution=128, channel_base=4096, channel_max=64, num_fp16_res=5, half_dtype=torch.bfloat16,
                                         conv_clamp=256), 'plan.').to(DEV).eval()
    ws = torch.randn([2, net.num_ws, 64], generator=torch.Generator().manual_seed(9)).to(DEV)
    current, packs, batches, left = [None], [], [], []
    for name, m in net.named_modules():
        if isinstance(m, PN.SynthesisLayer):
            m.register_forward_pre_hook(lambda mod, args, name=name: current.__setitem__(0, name))
    pack_weight, pack_weight_grouped, pack_weight_batched, pack_clear, prep_clear = M.pack_weight, M.pack_weight_grouped, M.pack_weight_batched, M.pack_clear, conv2d_mfma.modconv_prep_clear

    def form(w, transpose_oi, grouped):
        k = tuple(w.shape[-2:])
        return 'composite x4' if grouped else {(3, 2): 'fused-x', (2, 2): 'merged-t', (3, 3): 'composite x1' if transpose_oi else 'up1'}.get(k, f'{k[0]}x{k[1]}')

    def spy_pack(w, dtype, *args, **kw):
        packs.append((current[0], form(w, kw.get('transpose_oi', False), False), kw.get('styles') is None))
        return pack_weight(w, dtype, *args, **kw)

    def spy_grouped(ws_, dtype, *args, **kw):
        packs.append((current[0], form(ws_, True, True), kw.get('styles') is None))
        return pack_weight_grouped(ws_, dtype, *args, **kw)

    def spy_batched(jobs, dtype):
        batches.append(len(jobs))
        return pack_weight_batched(jobs, dtype)

    def spy_clear(clear):
        def run():
            left.append((len(conv2d_mfma._prep_registry), len(M._pack_registry)))
            return clear()
        return run
    monkeypatch.setattr(M, 'pack_weight', spy_pack)
    monkeypatch.setattr(M, 'pack_weight_grouped', spy_grouped)
    monkeypatch.setattr(M, 'pack_weight_batched', spy_batched)
    monkeypatch.setattr(M, 'pack_clear', spy_clear(pack_clear))
    monkeypatch.setattr(conv2d_mfma, 'modconv_prep_clear', spy_clear(prep_clear))
    k3 = ('up1', 'fused-x', 'composite x1', 'composite x4')         # the forms with 3x3 / 3x2 kernels (the ToRGB heads are 1x1)

    # every layer packs for itself (cold caches: the shared packs show too): the plan
    monkeypatch.setenv('PG_PACK_BATCHED', '0')
    monkeypatch.setenv('PG_PREP_BATCHED', '0')
    with torch.no_grad():
        want = net(ws, noise_mode='const').clone()
    plan = [p for p in packs if p[1] in k3]
    for name, kind, shared in plan:
        print(f'{name}: {kind}, {"shared" if shared else "per-sample"}')
    expected = [(n_, 'composite x1' if (fusedx == '0' and k == 'fused-x') else k, s) for n_, k, s in _BATCH_PLAN]
    assert plan == expected and not batches
    per_sample = [p for p in plan if not p[2] and p[1] != 'composite x4']
    assert len(per_sample) >= 4

    # the stack prepares them in one batch
    del packs[:], left[:]
    monkeypatch.setenv('PG_PACK_BATCHED', '1')
    monkeypatch.setenv('PG_PREP_BATCHED', '1')
    with torch.no_grad():
        got = net(ws, noise_mode='const').clone()
    print(f'batched: {batches} jobs; packs by layers during the forward: {packs}; registries (prep, pack) at the clears: {left}')
    assert batches == [len(per_sample)]
    assert not [p for p in packs if not p[2] and p[1] in k3]
    assert left and left[0] == (0, 0)
    assert torch.equal(got, want)
