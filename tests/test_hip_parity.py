"""GPU parity tests: the HIP path (through the C ABI) against (a) the golden vectors made by the
reference itself and (b) the CPU oracle on seeded inputs, plus size-independent properties
(linearity, adjointness) at full BASELINE sizes.  Run with ``-m gpu`` on an MI355X.

Tolerances (float32): ops that only reorder a short sum are held to 2e-5 rel / 2e-6 abs of the
output scale; convolutions (K up to 4608 products, different summation order than oneDNN) to
2e-4 of the output scale; the stacked network to north_star's bound scaled to the output range
(1e-3 of max|out|, see test_synthesis_*)."""

import math

import numpy as np
import pytest
import torch

import cases as C
from detgen import det_tensor, fill_module_, synthesis_inputs

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import bias_act, upfirdn2d, conv2d_mfma
    assert bias_act._init() and upfirdn2d._init() and conv2d_mfma._init() is not None   # native code loaded, or fail loudly


def close(a, b, rtol, atol):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def scale_of(t):
    t = t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return max(1.0, float(np.abs(t).max()))


def _filter(spec, name):
    from torch_utils.ops import upfirdn2d
    if spec is None:
        return None
    kind, v = spec
    return upfirdn2d.setup_filter(v) if kind == 'taps' else det_tensor(name + '.f', v, 'uniform')


# =============================================================== upfirdn2d

@pytest.mark.parametrize('case', C.UPFIRDN2D_CASES, ids=[c[0] for c in C.UPFIRDN2D_CASES])
def test_upfirdn2d_golden(golden, case):
    from torch_utils.ops import upfirdn2d
    g = golden('g1_upfirdn2d.npz')
    name, xs, fspec, up, down, pad, flip, gain = case
    f = _filter(fspec, name)
    fd = f.to(DEV) if f is not None else None
    x = det_tensor(name + '.x', xs).to(DEV).requires_grad_(True)
    y = upfirdn2d.upfirdn2d(x, fd, up=up, down=down, padding=pad, flip_filter=flip, gain=gain)
    s = scale_of(g[f'{name}/y'])
    close(y, g[f'{name}/y'], 2e-5, 3e-6 * s)
    dx, = torch.autograd.grad(y, x, det_tensor(name + '.dy', y.shape).to(DEV))
    close(dx, g[f'{name}/dx'], 2e-5, 3e-6 * s)
    if name in C.UPFIRDN2D_DTYPE_CASES:
        for dt, tag, tol in ((torch.float64, 'f64', 1e-9), (torch.float16, 'f16', 4e-3), (torch.bfloat16, 'bf16', 3e-2)):
            yd = upfirdn2d.upfirdn2d(x.detach().to(dt), fd, up=up, down=down, padding=pad, flip_filter=flip, gain=gain)
            assert yd.dtype == dt
            close(yd, g[f'{name}/y_{tag}'], tol, tol * s)


@pytest.mark.parametrize('shape,up,down,pad,gain', [
    ([2, 8, 129, 129], 1, 1, [1, 1, 1, 1], 4),      # odd 2H+1 -> 2H blur (the 513 -> 512 case in small)
    ([1, 3, 64, 64], 2, 1, [2, 1, 2, 1], 4),
    ([2, 5, 130, 70], 1, 2, [1, 1, 1, 1], 1),
    ([1, 4, 64, 200], 1, 1, [2, 2, 2, 2], 1),
])
def test_upfirdn2d_vs_oracle_multi_tile(shape, up, down, pad, gain):
    """Shapes that span several 64x16 tiles with ragged edges, against the CPU oracle."""
    from torch_utils.ops import upfirdn2d
    from oracle import ops_ref as R
    f = upfirdn2d.setup_filter(C.FIR_1331)
    x = det_tensor(f'mt.{shape}.{up}.{down}', shape)
    ref = R.upfirdn2d(x, f, up=up, down=down, padding=pad, gain=gain)
    y = upfirdn2d.upfirdn2d(x.to(DEV), f.to(DEV), up=up, down=down, padding=pad, gain=gain)
    close(y, ref, 2e-5, 3e-6 * scale_of(ref))
    # channels_last input takes the generic kernel and keeps its layout
    xcl = x.to(DEV).contiguous(memory_format=torch.channels_last)
    ycl = upfirdn2d.upfirdn2d(xcl, f.to(DEV), up=up, down=down, padding=pad, gain=gain)
    assert ycl.is_contiguous(memory_format=torch.channels_last)
    close(ycl, ref, 2e-5, 3e-6 * scale_of(ref))


def test_upfirdn2d_helpers_and_separable_vs_oracle():
    from torch_utils.ops import upfirdn2d
    from oracle import ops_ref as R
    x = det_tensor('helpers.x', [2, 3, 40, 36])
    f2, f12 = upfirdn2d.setup_filter(C.FIR_1331), upfirdn2d.setup_filter(C.FIR_12)
    for f in (f2, f12):
        close(upfirdn2d.upsample2d(x.to(DEV), f.to(DEV)), R.upsample2d(x, f), 3e-5, 3e-5)
        close(upfirdn2d.downsample2d(x.to(DEV), f.to(DEV)), R.downsample2d(x, f), 3e-5, 3e-5)
        close(upfirdn2d.filter2d(x.to(DEV), f.to(DEV)), R.filter2d(x, f), 3e-5, 3e-5)
    close(upfirdn2d.downsample2d(x.to(DEV), f12.to(DEV), padding=-6, flip_filter=True), R.downsample2d(x, f12, padding=-6, flip_filter=True), 3e-5, 3e-5)


def test_upfirdn2d_full_size_properties():
    """[8,64,513,513] -> 512 blur (config 2's hottest FIR): linearity and adjointness <Ax, y> = <x, A^T y>,
    where A^T is the op's own backward (upfirdn2d.py:245-264)."""
    from torch_utils.ops import upfirdn2d
    f = upfirdn2d.setup_filter(C.FIR_1331).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    x1 = torch.randn([8, 64, 513, 513], device=DEV, generator=gen)
    x2 = torch.randn([8, 64, 513, 513], device=DEV, generator=gen)
    op = lambda t: upfirdn2d.upfirdn2d(t, f, padding=[1, 1, 1, 1], gain=4)
    y1, y2 = op(x1), op(x2)
    assert y1.shape == (8, 64, 512, 512)
    lin = op(x1 * 0.5 + x2 * 2.0)
    assert float((lin - (y1 * 0.5 + y2 * 2.0)).abs().max()) < 1e-4
    x1r = x1[:1].clone().requires_grad_(True)
    yy = op(x1r)
    v = torch.randn(yy.shape, device=DEV, generator=gen)
    aty, = torch.autograd.grad(yy, x1r, v)
    lhs, rhs = float((yy.double() * v.double()).sum()), float((x1r.double() * aty.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))
    # a constant image stays constant away from the border (unit DC gain x gain 4)
    c = op(torch.ones([1, 1, 513, 513], device=DEV))
    assert float((c[:, :, 4:-4, 4:-4] - 4.0).abs().max()) < 1e-5


def test_upfirdn2d_argument_errors():
    from torch_utils.ops import upfirdn2d
    from torch_utils.ops._native import NativeOpError
    x = torch.zeros([1, 1, 4, 4], device=DEV)
    f = upfirdn2d.setup_filter(C.FIR_1331).to(DEV)
    with pytest.raises(NativeOpError):
        upfirdn2d.upfirdn2d(x, f, padding=-3)                 # output smaller than 1x1
    with pytest.raises(NativeOpError):
        upfirdn2d.upfirdn2d(x, f.cpu())                       # filter on another device
    with pytest.raises(AssertionError):
        upfirdn2d.upfirdn2d(x, f.double())                    # filter must be float32
    with pytest.raises(AssertionError):
        upfirdn2d.upfirdn2d(x[0], f)                          # rank 4 only


# =============================================================== bias_act

@pytest.mark.parametrize('act', C.ACTS)
def test_bias_act_golden(golden, act):
    from torch_utils.ops import bias_act
    g = golden('g2_bias_act.npz')
    for vname, has_b, gain, clamp, dim, xs in C.BIAS_ACT_VARIANTS:
        name = f'{act}.{vname}'
        x = det_tensor(name + '.x', xs, scale=2.0).to(DEV).requires_grad_(True)
        b = det_tensor(name + '.b', [xs[dim]]).to(DEV).requires_grad_(True) if has_b else None
        y = bias_act.bias_act(x, b, dim=dim, act=act, gain=gain, clamp=clamp)
        close(y, g[f'{name}/y'], 2e-5, 2e-6)
        dy = det_tensor(name + '.dy', xs).to(DEV).requires_grad_(True)
        grads = torch.autograd.grad(y, [x] + ([b] if has_b else []), dy, create_graph=True)
        close(grads[0], g[f'{name}/dx'], 3e-5, 3e-6)
        if has_b:
            close(grads[1], g[f'{name}/db'], 1e-4, 1e-5)
        if f'{name}/d_dy' in g and grads[0].requires_grad:
            v = det_tensor(name + '.v', xs).to(DEV)
            g2 = torch.autograd.grad(grads[0], [dy, x], v, allow_unused=True)
            close(g2[0], g[f'{name}/d_dy'], 3e-5, 3e-6)
            d_x = g2[1] if g2[1] is not None else torch.zeros(xs)
            close(d_x, g[f'{name}/d_x'], 1e-4, 1e-5)
        if vname in ('bias', 'bias_clamp'):
            for dt, tag, tol in ((torch.float64, 'f64', 1e-7), (torch.float16, 'f16', 4e-3), (torch.bfloat16, 'bf16', 3e-2)):
                yd = bias_act.bias_act(x.detach().to(dt), b.detach().to(dt), dim=dim, act=act, gain=gain, clamp=clamp)
                close(yd, g[f'{name}/y_{tag}'], tol, tol)


@pytest.mark.parametrize('shape', [[2, 7, 33, 17], [1, 64, 128, 128], [3, 5, 1, 1], [4, 9]])
def test_bias_act_vs_oracle_layouts(shape):
    """Odd sizes (scalar tail, bias runs not a multiple of the vector width), channels_last, views."""
    from torch_utils.ops import bias_act
    from oracle import ops_ref as R
    x = det_tensor(f'ba.{shape}', shape, scale=3.0)
    b = det_tensor(f'ba.b.{shape}', [shape[1]])
    ref = R.bias_act(x, b, act='lrelu', clamp=2.5)
    close(bias_act.bias_act(x.to(DEV), b.to(DEV), act='lrelu', clamp=2.5), ref, 2e-6, 2e-6)
    if len(shape) == 4:
        xcl = x.to(DEV).contiguous(memory_format=torch.channels_last)
        ycl = bias_act.bias_act(xcl, b.to(DEV), act='lrelu', clamp=2.5)
        assert ycl.stride() == xcl.stride()
        close(ycl, ref, 2e-6, 2e-6)
        xv = torch.cat([x, x], dim=3).to(DEV)[:, :, :, :shape[3]]         # non-dense view -> densified by the op
        close(bias_act.bias_act(xv, b.to(DEV), act='lrelu', clamp=2.5), ref, 2e-6, 2e-6)
    off = torch.zeros(x.numel() + 1, device=DEV)                          # 4-byte-offset storage -> unaligned path
    off[1:] = x.flatten().to(DEV)
    xo = off[1:].view(shape)
    close(bias_act.bias_act(xo, b.to(DEV), act='lrelu', clamp=2.5), ref, 2e-6, 2e-6)
    assert bias_act.bias_act(torch.zeros([0, 3], device=DEV), None, act='relu').shape == (0, 3)   # empty input


def test_bias_act_full_size_properties():
    """[8,64,512,512] (config 2's largest bias_act): idempotence of relu, positive homogeneity of lrelu,
    agreement with the torch expression of the same formula on the GPU."""
    from torch_utils.ops import bias_act
    gen = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn([8, 64, 512, 512], device=DEV, generator=gen)
    b = torch.randn([64], device=DEV, generator=gen)
    r = bias_act.bias_act(x, None, act='relu', gain=1)
    assert torch.equal(bias_act.bias_act(r, None, act='relu', gain=1), r)
    l1 = bias_act.bias_act(x, None, act='lrelu', gain=1)
    l3 = bias_act.bias_act(x * 3, None, act='lrelu', gain=1)
    assert float((l3 - 3 * l1).abs().max()) < 1e-5
    y = bias_act.bias_act(x, b, act='lrelu', clamp=256)
    ref = torch.nn.functional.leaky_relu(x + b.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    assert float((y - ref.clamp(-256, 256)).abs().max()) < 1e-5


@pytest.mark.parametrize('case', [
    # name, shape, dim, dtype, channels_last, act, gain, clamp
    ('nchw_lrelu',      [4, 64, 72, 72],  1, torch.float32, False, 'lrelu',  math.sqrt(2), 1.5),
    ('nchw_big_plane',  [2, 16, 260, 252], 1, torch.float32, False, 'relu',   math.sqrt(2), -1),
    ('nchw_tiny_plane', [4, 512, 4, 4],   1, torch.float32, False, 'lrelu',  1.0, -1),
    ('nchw_linear_clamp', [3, 24, 20, 12], 1, torch.float32, False, 'linear', 0.7, 0.9),
    ('fc',              [8, 512],         1, torch.float32, False, 'lrelu',  math.sqrt(2), -1),
    ('cl_f16',          [4, 128, 32, 32], 1, torch.float16, True,  'lrelu',  math.sqrt(2), 256),
    ('cl_bf16',         [2, 64, 24, 40],  1, torch.bfloat16, True, 'relu',   1.0, -1),
    ('nchw_f16',        [2, 32, 48, 48],  1, torch.float16, False, 'lrelu',  math.sqrt(2), 256),
])
def test_bias_act_gradient_with_bias_gradient_in_one_pass(case):
    """pg_bias_act_grad_bias: dx must equal the grad == 1 form bit for bit, db must be the sum of those stored values (fp64 sum as the
    yardstick), identical from run to run; through autograd the bias gradient agrees with the oracle's composition."""
    from torch_utils.ops import bias_act
    from oracle import ops_ref as R
    name, shape, dim, dt, cl, act, gain, clamp = case
    fmt = torch.channels_last if cl else torch.contiguous_format
    y = (det_tensor(f'gb.{name}.y', shape, scale=2.0).to(DEV).to(dt)).contiguous(memory_format=fmt) if len(shape) == 4 else det_tensor(f'gb.{name}.y', shape, scale=2.0).to(DEV).to(dt)
    dy = (det_tensor(f'gb.{name}.dy', shape).to(DEV).to(dt)).contiguous(memory_format=fmt) if len(shape) == 4 else det_tensor(f'gb.{name}.dy', shape).to(DEV).to(dt)
    spec = bias_act.activation_funcs[act]
    alpha = spec.def_alpha
    yref = y if (act != 'linear' or clamp >= 0) else None
    two = bias_act._native_bias_act(dy, None, None, yref, None, 1, dim, spec.cuda_idx, alpha, gain, clamp)
    out = bias_act._native_grad_bias(dy, yref, dim, act, alpha, gain, clamp)
    assert out is not None, 'layout expected to be covered'
    dx, db = out
    assert torch.equal(dx, two) and dx.stride() == dy.stride()
    axes = [i for i in range(len(shape)) if i != dim]
    want = two.double().sum(axes)
    scale = float(two.double().abs().sum(axes).max())
    tol = 2e-6 * scale if dt == torch.float32 else (2e-3 if dt == torch.float16 else 1.6e-2) * max(float(want.abs().max()), 1e-3)
    assert float((db.double() - want).abs().max()) <= tol
    again = bias_act._native_grad_bias(dy, yref, dim, act, alpha, gain, clamp)[1]
    assert torch.equal(db, again)
    only = bias_act._native_grad_bias(dy, yref, dim, act, alpha, gain, clamp, write=False)
    assert only[0] is None and torch.equal(only[1], db)
    # through the op: x -> bias_act -> loss; db against the oracle (float32 cases)
    if dt == torch.float32:
        x = det_tensor(f'gb.{name}.x', shape, scale=2.0)
        b = det_tensor(f'gb.{name}.b', [shape[dim]])
        xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
        R.bias_act(xr, br, dim=dim, act=act, gain=gain, clamp=clamp if clamp >= 0 else None).backward(dy.float().cpu())
        xg, bg = x.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        bias_act.bias_act(xg, bg, dim=dim, act=act, gain=gain, clamp=clamp if clamp >= 0 else None).backward(dy)
        close(xg.grad, xr.grad, 3e-6, 3e-6)
        close(bg.grad, br.grad, 2e-5, 2e-6 * scale)


def test_bias_act_bias_gradient_uncovered_layouts_and_second_order():
    from torch_utils.ops import bias_act
    y = det_tensor('gbu.y', [2, 7, 33, 17]).to(DEV)
    dy = det_tensor('gbu.dy', [2, 7, 33, 17]).to(DEV)
    assert bias_act._native_grad_bias(dy, y, 1, 'lrelu', 0.2, 1.0, -1.0) is None            # plane of 561 floats: not a multiple of 16 bytes
    assert bias_act._native_grad_bias(dy, y, 1, 'tanh', 0.0, 1.0, -1.0) is None             # derivative outside the fused set
    assert torch.allclose(bias_act.channel_sum(dy, 1), dy.sum([0, 2, 3]), rtol=1e-5, atol=1e-5)   # composed instead
    t = det_tensor('gbu.t', [3, 16, 8, 8]).to(DEV)
    close(bias_act.channel_sum(t, 1), t.double().sum([0, 2, 3]).float(), 1e-5, 1e-5)
    close(bias_act.channel_sum(t[:, :, ::2], 1), t[:, :, ::2].double().sum([0, 2, 3]).float(), 1e-5, 1e-5)      # a view: densified first
    # db's own gradient (double backward through the two-output Function): d(db . v)/d(dy) = act'(y) gain v[c]
    x = det_tensor('gbu.x', [2, 8, 4, 4]).to(DEV).requires_grad_(True)
    b = det_tensor('gbu.b', [8]).to(DEV).requires_grad_(True)
    dyy = det_tensor('gbu.dyy', [2, 8, 4, 4]).to(DEV).requires_grad_(True)
    yy = bias_act.bias_act(x, b, act='lrelu')
    gx, gb = torch.autograd.grad(yy, [x, b], dyy, create_graph=True)
    v = det_tensor('gbu.v', [8]).to(DEV)
    (g_dyy,) = torch.autograd.grad(gb, [dyy], v)
    slope = torch.where(yy > 0, 1.0, 0.2) * math.sqrt(2)
    close(g_dyy, (slope * v.view(1, -1, 1, 1)).detach(), 1e-6, 1e-6)


# =============================================================== conv2d (MFMA implicit GEMM)

CONV_CASES = [
    # name, N, Cin, Cout, H, W, k, stride, pad
    ('k3_small',      2, 5, 6, 9, 9, 3, 1, 1),
    ('k3_c64',        2, 64, 64, 40, 33, 3, 1, 1),
    ('k3_c128_odd',   1, 128, 128, 17, 45, 3, 1, 1),
    ('k3_c96',        1, 24, 96, 20, 20, 3, 1, 1),
    ('k3_cin1',       2, 1, 64, 32, 32, 3, 1, 1),
    ('k3_nopad',      1, 8, 16, 12, 12, 3, 1, 0),
    ('k1_torgb',      2, 64, 3, 32, 32, 1, 1, 0),
    ('k1_merge',      1, 192, 128, 24, 24, 1, 1, 0),
    ('k1_c7',         2, 37, 7, 19, 21, 1, 1, 0),
    ('k7_enc',        2, 3, 64, 40, 40, 7, 1, 3),
    ('k3_s2',         2, 64, 128, 35, 35, 3, 2, 0),
    ('k1_s2',         1, 16, 24, 20, 20, 1, 2, 0),
    ('k3_c512_lowres', 2, 512, 512, 8, 8, 3, 1, 1),
]


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv2d_vs_oracle(case):
    from torch_utils.ops import conv2d_gradfix
    import torch.nn.functional as F
    name, n, cin, cout, h, w, k, stride, pad = case
    x = det_tensor(name + '.x', [n, cin, h, w])
    wt = det_tensor(name + '.w', [cout, cin, k, k], scale=1 / math.sqrt(cin * k * k))
    b = det_tensor(name + '.b', [cout])
    ref = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=pad)
    xd, wd = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True)
    y = conv2d_gradfix.conv2d(xd, wd, b.to(DEV), stride=stride, padding=pad)
    close(y, ref, 1e-4, 2e-5 * scale_of(ref))
    # gradients (aten convolution_backward behind the native forward)
    dy = det_tensor(name + '.dy', y.shape)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(xr, wr, stride=stride, padding=pad), [xr, wr], dy.double())
    dx, dw = torch.autograd.grad(y, [xd, wd], dy.to(DEV))
    close(dx, gx, 1e-3, 1e-4 * scale_of(gx))
    close(dw, gw, 1e-3, 1e-4 * scale_of(gw))


@pytest.mark.parametrize('n,cout,h,w,pad,mod,flip', [(2, 64, 37, 70, 3, False, False), (1, 40, 64, 33, 3, False, True), (2, 64, 19, 40, 3, True, False),
                                                    (1, 128, 9, 100, 0, False, False), (3, 64, 8, 32, 2, False, False), (1, 7, 21, 21, 3, True, True)])
def test_conv7x7_three_channel_stem(n, cout, h, w, pad, mod, flip):
    """The 7x7 stem on a 3-channel image (networks.py ResnetGenerator-style encoders): pg_conv2d_pack_weight stores such kernels in the
    row-pair form (channel slot 3 = channel 2 one kernel row down) and the plain launch walks only the even kernel rows in its second
    K chunk; a modulated launch (no row-pair mode) must still be exact with the same pack, as must the flipped pack.  Against float64."""
    from torch_utils.ops import conv2d_mfma
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(7 * cout + h)
    x = torch.randn([n, 3, h, w], generator=gen)
    wt = torch.randn([cout, 3, 7, 7], generator=gen) / math.sqrt(147)
    s_in = torch.randn([n, 3], generator=gen) if mod else None
    b = torch.randn([cout], generator=gen)
    packed = conv2d_mfma.pack_weight(wt.to(DEV), flip=flip)
    y = conv2d_mfma.conv2d_forward(x.to(DEV), packed, cout, 7, 7, pad=(pad, pad), in_scale=s_in.to(DEV) if mod else None, bias=b.to(DEV), act='relu')
    xr = x.double() * (s_in.double()[:, :, None, None] if mod else 1.0)
    ref = F.conv2d(xr, (wt.flip([2, 3]) if flip else wt).double(), b.double(), padding=pad).relu()
    close(y, ref, 1e-5, 3e-6 * scale_of(ref))


@pytest.mark.parametrize('n,cin,cout,h,w,k,pad,opad', [(2, 6, 5, 8, 8, 3, 0, 0), (1, 64, 64, 16, 19, 3, 0, 0), (2, 8, 12, 7, 9, 3, 1, 0), (1, 16, 8, 6, 6, 3, 1, 1)])
def test_conv_transpose2d_vs_oracle(n, cin, cout, h, w, k, pad, opad):
    from torch_utils.ops import conv2d_gradfix
    import torch.nn.functional as F
    x = det_tensor(f'ct.x.{cin}.{h}', [n, cin, h, w])
    wt = det_tensor(f'ct.w.{cin}.{cout}', [cin, cout, k, k], scale=1 / math.sqrt(cin * k * k))
    ref = F.conv_transpose2d(x.double(), wt.double(), stride=2, padding=pad, output_padding=opad)
    y = conv2d_gradfix.conv_transpose2d(x.to(DEV), wt.to(DEV), stride=2, padding=pad, output_padding=opad)
    close(y, ref, 1e-4, 2e-5 * scale_of(ref))


@pytest.mark.parametrize('winograd', [False, True], ids=['direct', 'winograd'])
def test_conv2d_fused_prologue_epilogue_vs_oracle(winograd):
    """Every fused stage of pg_conv2d_forward / pg_conv2d_winograd_forward against the unfused oracle composition."""
    from torch_utils.ops import conv2d_mfma
    from oracle import ops_ref as R
    import torch.nn.functional as F
    n, cin, cout, h, w = 2, 20, 70, 19, 37
    x = det_tensor('fz.x', [n, cin, h, w])
    wt = det_tensor('fz.w', [cout, cin, 3, 3], scale=0.1)
    styles = det_tensor('fz.s', [n, cin]) + 1
    dco = det_tensor('fz.d', [n, cout]).abs() + 0.5
    in_b, out_b = det_tensor('fz.ib', [cin]), det_tensor('fz.ob', [cout])
    noise = det_tensor('fz.noise', [n, 1, h, w])
    res = det_tensor('fz.res', [n, cout, h, w])
    packed = conv2d_mfma.pack_weight(wt.to(DEV), scale=0.5, winograd=winograd)
    y = conv2d_mfma.conv2d_forward(x.to(DEV), packed, cout, 3, 3, pad=(1, 1),
                                   in_scale=styles.to(DEV), in_act='relu', in_gain=1.3, in_clamp=2.0,
                                   out_scale=dco.to(DEV), noise=noise.to(DEV), noise_gain=0.7, bias=out_b.to(DEV), act='lrelu', alpha=0.2,
                                   gain=math.sqrt(2), clamp=3.0, residual=res.to(DEV), winograd=winograd)
    xr = R.bias_act(x * styles[:, :, None, None], None, act='relu', gain=1.3, clamp=2.0)
    ref = F.conv2d(xr, wt * 0.5, padding=1) * dco[:, :, None, None] + noise * 0.7
    ref = R.bias_act(ref, out_b, act='lrelu', gain=math.sqrt(2), clamp=3.0) + res
    close(y, ref, 1e-4, 1e-4)
    # a prologue bias cannot be fused (act(0 + b) != 0 would corrupt the zero padding): rejected, never silently wrong
    from torch_utils.ops._native import NativeOpError
    with pytest.raises(NativeOpError):
        conv2d_mfma.conv2d_forward(x.to(DEV), packed, cout, 3, 3, pad=(1, 1), in_bias=in_b.to(DEV), in_act='relu', winograd=winograd)
    # lrelu prologue with modulation, 1x1 kernel (the SPADE skip path)
    p1 = conv2d_mfma.pack_weight(wt[:, :, :1, :1].contiguous().to(DEV))
    y1 = conv2d_mfma.conv2d_forward(x.to(DEV), p1, cout, 1, 1, in_act='lrelu', in_alpha=0.2, in_gain=math.sqrt(2))
    close(y1, F.conv2d(R.bias_act(x, None, act='lrelu'), wt[:, :, :1, :1]), 1e-4, 1e-4)
    # flipped packing == true convolution
    yf = conv2d_mfma.conv2d_forward(x.to(DEV), conv2d_mfma.pack_weight(wt.to(DEV), flip=True, winograd=winograd), cout, 3, 3, pad=(1, 1), winograd=winograd)
    close(yf, F.conv2d(x, wt.flip([2, 3]), padding=1), 1e-4, 1e-4)
    # IOHW weights (the conv_transpose2d view) pack to the same operand
    yt = conv2d_mfma.conv2d_forward(x.to(DEV), conv2d_mfma.pack_weight(wt.transpose(0, 1).contiguous().to(DEV), transpose_oi=True, winograd=winograd),
                                    cout, 3, 3, pad=(1, 1), winograd=winograd)
    close(yt, F.conv2d(x, wt, padding=1), 1e-4, 1e-4)


@pytest.mark.parametrize('n,cin,cout,h,w,pad', [(1, 16, 64, 8, 64, 1), (2, 20, 70, 9, 71, 1), (1, 3, 3, 5, 7, 1), (2, 48, 128, 33, 130, 0),
                                               (1, 128, 64, 16, 16, 2), (3, 17, 33, 1, 1, 1), (1, 40, 192, 2, 200, 1), (2, 1, 64, 31, 3, 1),
                                               (1, 16, 64, 12, 68, 3), (2, 32, 96, 7, 130, 4)])
def test_conv2d_winograd_vs_oracle_and_direct(n, cin, cout, h, w, pad):
    """pg_conv2d_winograd_forward: F(2x2,3x3) on ragged shapes (odd sizes, partial tiles, pad 0/1/2, Cin/Cout not multiples of
    the tile) against the fp64 convolution; its error must stay at the level of the direct kernel's."""
    from torch_utils.ops import conv2d_mfma
    import torch.nn.functional as F
    x = det_tensor(f'wg.x.{cin}.{h}.{w}', [n, cin, h, w])
    wt = det_tensor(f'wg.w.{cin}.{cout}', [cout, cin, 3, 3], scale=1 / math.sqrt(cin * 9))
    ref = F.conv2d(x.double(), wt.double(), padding=pad)
    yd = conv2d_mfma.conv2d_forward(x.to(DEV), conv2d_mfma.pack_weight(wt.to(DEV)), cout, 3, 3, pad=(pad, pad))
    yw = conv2d_mfma.conv2d_forward(x.to(DEV), conv2d_mfma.pack_weight(wt.to(DEV), winograd=True), cout, 3, 3, pad=(pad, pad), winograd=True)
    close(yw, ref, 1e-4, 1e-5 * scale_of(ref))
    err_d = (yd.double().cpu() - ref).abs().max().item()
    err_w = (yw.double().cpu() - ref).abs().max().item()
    assert err_w <= 4 * err_d + 1e-6 * scale_of(ref)
    # strided output view (channel slice of a wider tensor), as the synthesis blocks use
    big = torch.zeros([n, cout + 3, ref.shape[2], ref.shape[3]], device=DEV)
    conv2d_mfma.conv2d_forward(x.to(DEV), conv2d_mfma.pack_weight(wt.to(DEV), winograd=True), cout, 3, 3, pad=(pad, pad), y=big[:, 2:2 + cout], winograd=True)
    assert torch.equal(big[:, 2:2 + cout], yw) and float(big[:, :2].abs().max()) == 0 and float(big[:, 2 + cout:].abs().max()) == 0


def test_conv2d_empty_batch_returns_empty_like_the_reference():
    """F.conv2d / F.conv_transpose2d on an empty batch return an empty tensor of the right shape (what the reference's
    conv2d_gradfix.py:35-43 forwards to); so do the drop-in ops, and gradients flow."""
    from torch_utils.ops import conv2d_gradfix, conv2d_resample, upfirdn2d
    w = det_tensor('empty.w', [6, 4, 3, 3]).to(DEV).requires_grad_(True)
    x = torch.zeros([0, 4, 9, 9], device=DEV, requires_grad=True)
    y = conv2d_gradfix.conv2d(x, w, padding=1)
    assert tuple(y.shape) == (0, 6, 9, 9)
    y.sum().backward()
    assert float(w.grad.abs().max()) == 0.0
    assert tuple(conv2d_gradfix.conv_transpose2d(x.detach(), w.detach().transpose(0, 1).contiguous(), stride=2).shape) == (0, 6, 19, 19)
    f = upfirdn2d.setup_filter(C.FIR_1331).to(DEV)
    one = conv2d_resample.conv2d_resample(torch.zeros([1, 4, 9, 9], device=DEV), w.detach(), f=f, down=2, padding=1)
    assert tuple(conv2d_resample.conv2d_resample(x.detach(), w.detach(), f=f, down=2, padding=1).shape) == (0,) + tuple(one.shape[1:])


def test_conv2d_winograd_rejects_what_it_cannot_do():
    from torch_utils.ops import conv2d_mfma
    from torch_utils.ops._native import NativeOpError
    x = det_tensor('wgr.x', [1, 16, 8, 8]).to(DEV)
    w3 = det_tensor('wgr.w', [64, 16, 3, 3]).to(DEV)
    with pytest.raises(NativeOpError):
        conv2d_mfma.pack_weight(w3[:, :, :1, :1].contiguous(), winograd=True)                      # 3x3 only
    pw = conv2d_mfma.pack_weight(w3, winograd=True)
    with pytest.raises(NativeOpError):
        conv2d_mfma.conv2d_forward(x, pw, 64, 3, 3, stride=2, winograd=True)                       # stride 1 only
    with pytest.raises(NativeOpError):
        conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(det_tensor('wgr.w2', [64, 32, 3, 3]).to(DEV), winograd=True), 64, 3, 3, pad=(1, 1),
                                   x2=x, winograd=True)                                          # two-source launches: direct kernel
    assert not conv2d_mfma.use_winograd(3, 3, 1, 64, x2=x) and not conv2d_mfma.use_winograd(3, 3, 2, 64) and not conv2d_mfma.use_winograd(1, 1, 1, 64)
    assert conv2d_mfma.use_winograd(3, 3, 1, 64, 16, pad=(9, 4)) and not conv2d_mfma.use_winograd(3, 3, 1, 64, 16, pad=(1, 5))
    with pytest.raises(NativeOpError):
        conv2d_mfma.conv2d_forward(x, pw, 64, 3, 3, pad=(1, 5), winograd=True)                  # halo wider than the LDS row: direct kernel
    from torch_utils.ops import conv2d_gradfix
    import torch.nn.functional as F
    y5 = conv2d_gradfix.conv2d(x, w3, padding=5)                                                 # the operator falls back by itself
    close(y5, F.conv2d(x.double().cpu(), w3.double().cpu(), padding=5), 1e-4, 1e-5)


@pytest.mark.parametrize('n,cin,cout,h,w,pad', [(1, 16, 64, 8, 64, 1), (2, 64, 64, 16, 128, 1), (2, 32, 128, 24, 64, 1), (1, 48, 70, 9, 72, 1), (2, 20, 40, 13, 100, 1),
                                                (1, 128, 128, 40, 192, 1), (3, 64, 64, 64, 64, 2), (3, 64, 64, 40, 64, 3), (2, 16, 64, 7, 8, 1), (1, 80, 64, 32, 64, 3), (2, 16, 64, 12, 62, 2),
                                                (2, 40, 70, 13, 72, 3), (1, 32, 96, 19, 136, 3)])
@pytest.mark.parametrize('form', [2, 3, 4], ids=['one_wg_per_cu', 'two_wg_per_cu', 'one_wg_per_cu_bf16x3'])
def test_conv2d_winograd4_kernel(n, cin, cout, h, w, pad, form):
    """csrc/conv2d_wino4.h (Winograd F(4x4,3x3), round 3: form 2) and csrc/conv2d_wino4b.h (the same algorithm with two workgroups per CU on
    v_mfma_f32_16x16x4_f32, round 4: form 3; 8 x 32-pixel tiles, its own weight stream and SPADE row order) and form 4 (round 6: form 2's kernel with its transform-domain GEMM as six
    bf16 products of exact three-term operand splits on v_mfma_f32_32x32x16_bf16, fp32 accumulation -- same bars) on full, edge and ragged tiles (heights that are no multiple of 8, widths
    no multiple of 64, couts no multiple of 64, channel counts no multiple of 16): plain against the fp64 convolution;
    every fused stage, per-sample noise and SPADE mode against the direct MFMA kernel running the same launch (which meets the oracle in
    test_conv2d_fused_prologue_epilogue_vs_oracle; test_conv2d_winograd4_tails_vs_oracle compares one shape per tail kind with the oracle directly).
    Paddings: the kernel needs W % 4 == 0 AND OW = W + 2 pad - 2 a multiple of 4, i.e. only ODD paddings (1, 3) can run -- the pad = 2 cases
    here assert the decline; the kernels' former pad 0 / 4 staging arithmetic (unreachable through the C ABI, never exercised) is gone since round 5 and the launchers decline every even padding by name.
    pad = 3 also runs with ragged H and Cout % 64 != 0 together.  Tolerance: F(4x4)'s
    transforms cost ~4x the rounding of the direct kernel (tools/f43_error_probe.py): 1e-4 of the output scale."""
    from torch_utils.ops import conv2d_mfma
    import torch.nn.functional as F
    x = det_tensor(f'w4.x.{cin}.{h}.{w}', [n, cin, h, w]).to(DEV)
    wt = det_tensor(f'w4.w.{cin}.{cout}', [cout, cin, 3, 3], scale=1 / (3 * math.sqrt(cin))).to(DEV)

    def run(algo, **kw):
        return conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(wt, winograd=algo), cout, 3, 3, pad=(pad, pad), winograd=algo, **kw)
    ref = F.conv2d(x.double().cpu(), wt.double().cpu(), padding=pad)
    oh, ow = ref.shape[2:]
    if ow % 4 != 0 or w % 4 != 0:         # 16-byte halo words and 16-byte output row segments: such a launch is declined (the policy never asks for it)
        from torch_utils.ops._native import NativeNotCovered
        with pytest.raises(NativeNotCovered):
            run(form)
        return
    close(run(form), ref, 0, 1e-4 * scale_of(ref))
    kw = dict(in_scale=det_tensor('w4.s', [n, cin]).to(DEV) + 1.5, out_scale=det_tensor('w4.d', [n, cout]).abs().to(DEV) + 0.5, noise=det_tensor('w4.nz', [oh, ow]).to(DEV),
              noise_gain=0.3, bias=det_tensor('w4.b', [cout]).to(DEV), act='lrelu', alpha=0.2, gain=1.4, clamp=2.0, residual=det_tensor('w4.r', [n, cout, oh, ow]).to(DEV))
    a, b = run(0, **kw), run(form, **kw)
    close(b, a, 0, 2e-4 * scale_of(ref) * 3)
    kw = dict(noise=det_tensor('w4.nzb', [n, oh, ow]).to(DEV), bias=det_tensor('w4.b', [cout]).to(DEV), act='relu')
    close(run(form, **kw), run(0, **kw), 0, 2e-4 * scale_of(ref))
    if cout % 64 == 0:
        c = cout // 2
        sx, mean, rstd = det_tensor('w4.sx', [n, c, oh, ow]).to(DEV), det_tensor('w4.mu', [n, c]).to(DEV), det_tensor('w4.rs', [n, c]).abs().to(DEV) + 0.5
        outs = []
        for algo in (0, form):
            pk = conv2d_mfma.pack_spade_gamma_beta(wt[:c].contiguous(), wt[c:].contiguous(), winograd=algo)
            outs.append(conv2d_mfma.conv2d_forward(x, pk, cout, 3, 3, pad=(pad, pad), spade=(sx, mean, rstd), winograd=algo, act='lrelu', alpha=0.2, gain=1.4, clamp=3.0))
        close(outs[1], outs[0], 0, 2e-4 * scale_of(outs[0]))
    # flipped / O<->I transposed packs (the input-gradient route): dx of y = conv(x, w) is conv(dy, w^T flipped)
    dy = det_tensor(f'w4.dy.{cout}.{oh}', [n, cout, oh, ow]).to(DEV)
    if 0 <= 2 - pad <= 4 and ow % 4 == 0:
        pk = conv2d_mfma.pack_weight(wt, flip=True, transpose_oi=True, winograd=form)
        dx = conv2d_mfma.conv2d_forward(dy, pk, cin, 3, 3, pad=(2 - pad, 2 - pad), winograd=form)
        want = torch.nn.grad.conv2d_input(x.shape, wt.double().cpu(), dy.double().cpu(), padding=pad)
        close(dx, want, 0, 1e-4 * scale_of(want))


@pytest.mark.parametrize('form', [2, 3, 4], ids=['one_wg_per_cu', 'two_wg_per_cu', 'one_wg_per_cu_bf16x3'])
@pytest.mark.parametrize('n,h,cin,cout', [(8, 512, 64, 64), (8, 256, 128, 128)])
def test_conv2d_winograd4_repeated_launches_are_identical(n, h, cin, cout, form):
    """Full-size launches of the F(4x4) kernel, 60 in a row with other work in between: every result must equal the first one bit for bit
    and match the direct kernel.  (Round 3: the tail's exchange area aliases the V buffer; without the barrier in front of its first write a
    fast wave overwrote operands slower waves were still multiplying -- 20 % of the launches had wrong tiles, none of the small cases did.)"""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(31)
    x = torch.randn([n, cin, h, h], generator=gen).to(DEV)
    other = torch.randn([n, cin, h, h], generator=gen).to(DEV)
    wt = (torch.randn([cout, cin, 3, 3], generator=gen) / (3 * math.sqrt(cin))).to(DEV)
    pk4, pk0 = conv2d_mfma.pack_weight(wt, winograd=form), conv2d_mfma.pack_weight(wt)
    ref = conv2d_mfma.conv2d_forward(x, pk0, cout, 3, 3, pad=(1, 1))
    first = conv2d_mfma.conv2d_forward(x, pk4, cout, 3, 3, pad=(1, 1), winograd=form)
    assert float((first - ref).abs().max()) <= 1e-4 * scale_of(ref)
    for it in range(60):
        if it % 3 == 1:
            conv2d_mfma.conv2d_forward(other, pk0, cout, 3, 3, pad=(1, 1))
        y = conv2d_mfma.conv2d_forward(x, pk4, cout, 3, 3, pad=(1, 1), winograd=form)
        assert torch.equal(y, first), f'launch {it} differs from the first one: max |d| {float((y - first).abs().max()):.3e}'


@pytest.mark.parametrize('form', [2, 3, 4], ids=['one_wg_per_cu', 'two_wg_per_cu', 'one_wg_per_cu_bf16x3'])
@pytest.mark.parametrize('tail', ['plain', 'residual', 'mod_noise', 'spade'])
def test_conv2d_winograd4_tails_vs_oracle(tail, form):
    """One shape per tail kind of the F(4x4) kernel (W4_TAIL_PLAIN / the run-time tail with a residual / modulated + noise / W4_TAIL_SPADE)
    against the UNFUSED oracle composition (oracle.ops_ref + fp64 convolution), not against another HIP kernel ("what's weak")."""
    from torch_utils.ops import conv2d_mfma
    from oracle import ops_ref as R
    from oracle import network_ref as NR
    import torch.nn.functional as F
    n, cin, cout, h, w = 2, 64, 128, 24, 72
    x = det_tensor('w4o.x', [n, cin, h, w])
    wt = det_tensor('w4o.w', [cout, cin, 3, 3], scale=1 / (3 * math.sqrt(cin)))
    b = det_tensor('w4o.b', [cout])
    conv = lambda xx, ww: F.conv2d(xx.double(), ww.double(), padding=1)
    run = lambda pk, **kw: conv2d_mfma.conv2d_forward(x.to(DEV), pk, cout, 3, 3, pad=(1, 1), winograd=form, **kw)
    pk = conv2d_mfma.pack_weight(wt.to(DEV), winograd=form)
    if tail == 'plain':
        y = run(pk, bias=b.to(DEV), act='lrelu', alpha=0.2, gain=math.sqrt(2), clamp=1.5)
        ref = R.bias_act(conv(x, wt), b.double(), act='lrelu', gain=math.sqrt(2), clamp=1.5)
    elif tail == 'residual':
        res = det_tensor('w4o.r', [n, cout, h, w])
        y = run(pk, bias=b.to(DEV), act='relu', gain=0.7, residual=res.to(DEV))
        ref = R.bias_act(conv(x, wt), b.double(), act='relu', gain=0.7) + res.double()
    elif tail == 'mod_noise':      # the non-fused modulated convolution (networks.py:73-82): x * styles -> conv -> fma(dcoefs, noise) -> bias_act
        styles, noise = det_tensor('w4o.s', [n, cin]) + 1.2, det_tensor('w4o.nz', [h, w])
        dco = ((wt.double()[None] * styles.double()[:, None, :, None, None]).square().sum([2, 3, 4]) + 1e-8).rsqrt()
        y = run(pk, in_scale=styles.to(DEV), out_scale=dco.float().to(DEV), noise=noise.to(DEV), noise_gain=0.4, bias=b.to(DEV), act='lrelu', alpha=0.2,
                gain=math.sqrt(2), clamp=256.0)
        ref = R.fma(conv(x.double() * styles.double()[:, :, None, None], wt), dco[:, :, None, None], noise.double() * 0.4)
        ref = R.bias_act(ref, b.double(), act='lrelu', gain=math.sqrt(2), clamp=256.0)
    else:                          # Spade_Norm_Block (networks.py:1715-1723): instance norm of sx, gamma / beta convolutions of x, then a following layer's pre-activation
        c = cout // 2
        sx = det_tensor('w4o.sx', [n, c, h, w]) * 2 + 0.3
        mean = sx.double().mean([2, 3])
        rstd = (sx.double().var([2, 3], unbiased=False) + 1e-5).rsqrt()
        pks = conv2d_mfma.pack_spade_gamma_beta(wt[:c].contiguous().to(DEV), wt[c:].contiguous().to(DEV), winograd=form)
        y = run(pks, spade=(sx.to(DEV), mean.float().to(DEV), rstd.float().to(DEV)), act='relu', gain=math.sqrt(2))
        ref = NR.instance_norm(sx.double()) * (1 + conv(x, wt[:c])) + conv(x, wt[c:])
        ref = R.bias_act(ref, None, act='relu', gain=math.sqrt(2))
    close(y, ref, 0, 1e-4 * scale_of(ref))


@pytest.mark.parametrize('form', [2, 4], ids=['fp32_mfma', 'bf16x3'])
@pytest.mark.parametrize('n,cin,cout,h,w', [(2, 64, 128, 24, 72), (1, 64, 64, 64, 64), (3, 32, 70, 13, 136), (8, 128, 128, 256, 256)])
def test_conv2d_winograd4_output_statistics(n, cin, cout, h, w, form):
    """pg_conv2d_fusion::stats_partial (round 4): the instance-norm statistics of a convolution's output gathered in the F(4x4) kernel's plain tail
    (sum / M2 per workgroup tile and cout, merged pairwise -- Chan -- in float64 in tile order) against (a) float64 torch statistics of the SAME output
    tensor and (b) the separate one-pass kernel (pg_instance_norm_stats) -- full, ragged (H % 8, W % 64, Cout % 64 != 0) and full-size shapes;
    the output itself must be bit-identical to the launch without statistics; launches other than the plain F(4x4) tail decline the request."""
    from torch_utils.ops import conv2d_mfma
    from torch_utils.ops._native import NativeNotCovered
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn([n, cin, h, w], generator=gen) + 0.3).to(DEV)
    wt = (torch.randn([cout, cin, 3, 3], generator=gen) / (3 * math.sqrt(cin))).to(DEV)
    b = torch.randn([cout], generator=gen).to(DEV)
    pk = conv2d_mfma.pack_weight(wt, winograd=form)
    y0 = conv2d_mfma.conv2d_forward(x, pk, cout, 3, 3, pad=(1, 1), winograd=form, bias=b)
    y, (mean, rstd) = conv2d_mfma.conv2d_forward(x, pk, cout, 3, 3, pad=(1, 1), winograd=form, bias=b, stats_eps=1e-5)
    assert torch.equal(y, y0)
    yd = y.double()
    want_mean = yd.mean([2, 3]).reshape(-1)
    want_rstd = (yd.var([2, 3], unbiased=False) + 1e-5).rsqrt().reshape(-1)
    close(mean, want_mean, 0, 2e-6 * scale_of(want_mean))
    close(rstd, want_rstd, 2e-5, 0)
    m2, r2 = conv2d_mfma.instance_norm_stats(y, eps=1e-5)
    close(mean, m2, 0, 2e-6 * scale_of(want_mean))
    close(rstd, r2, 2e-5, 0)
    again = conv2d_mfma.conv2d_forward(x, pk, cout, 3, 3, pad=(1, 1), winograd=form, bias=b, stats_eps=1e-5)[1]
    assert torch.equal(again[0], mean) and torch.equal(again[1], rstd)                       # deterministic: fixed reduction order, no atomics
    # |mean| >> std: a per-channel offset of ~50 on outputs of std ~0.6.  Sums of raw squares lose the variance there (relative error
    # ~1e-7 * mean^2 / var ~ 1e-3); the (sum, M2) pairs merged with Chan's formula stay at the two-pass kernel's accuracy
    b50 = (50.0 + torch.randn([cout], generator=gen)).to(DEV)
    y5, (mean5, rstd5) = conv2d_mfma.conv2d_forward(x, pk, cout, 3, 3, pad=(1, 1), winograd=form, bias=b50, stats_eps=1e-5)
    y5d = y5.double()
    close(mean5, y5d.mean([2, 3]).reshape(-1), 2e-6, 0)
    close(rstd5, (y5d.var([2, 3], unbiased=False) + 1e-5).rsqrt().reshape(-1), 2e-5, 0)
    for kw in (dict(residual=torch.zeros_like(y)), dict(in_scale=torch.ones([n, cin], device=DEV))):
        with pytest.raises(NativeNotCovered):
            conv2d_mfma.conv2d_forward(x, pk, cout, 3, 3, pad=(1, 1), winograd=form, stats_eps=1e-5, **kw)
    with pytest.raises(NativeNotCovered):
        conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(wt, winograd=1), cout, 3, 3, pad=(1, 1), winograd=1, stats_eps=1e-5)


def test_conv2d_winograd4_policy_and_declines():
    from torch_utils.ops import conv2d_mfma
    from torch_utils.ops._native import NativeNotCovered
    F4 = conv2d_mfma.F4_WIDE                      # images at least 64 pixels wide: the one-workgroup form -- 4 (GEMM on the bf16 pipe, three-term splits) unless PG_WINO4_X3=0 (2)
    FN = conv2d_mfma.F4_FORM                      # narrower images: 3 (two workgroups per CU) unless PG_WINO4B=0
    assert FN in (2, 3) and F4 in (2, 4)
    # the tail's max() form of the activation is exact for gain > 0, 0 <= alpha <= 1 only: the policy keeps anything else on F(2x2),
    # the kernel declines it, and the F(2x2) launch of the same request meets the oracle
    geo = dict(pad=(1, 1), hw=(64, 64))
    assert conv2d_mfma.use_winograd(3, 3, 1, 64, 64, ep=dict(act='lrelu', alpha=0.2, gain=1.4), **geo) == F4
    assert conv2d_mfma.use_winograd(3, 3, 1, 64, 64, ep=dict(act='lrelu', alpha=1.5, gain=1.4), **geo) == 1
    assert conv2d_mfma.use_winograd(3, 3, 1, 64, 64, ep=dict(act='relu', gain=-1.0), **geo) == 1
    assert conv2d_mfma.use_winograd(3, 3, 1, 64, 64, ep=dict(act='relu', alpha=None, gain=None), **geo) == F4
    xa = det_tensor('w4d.xa', [1, 64, 32, 64])
    wa = det_tensor('w4d.wa', [64, 64, 3, 3], scale=0.05)
    for kw in (dict(act='lrelu', alpha=1.5, gain=1.4), dict(act='lrelu', alpha=0.2, gain=-0.5), dict(act='relu', gain=-2.0)):
        for form in (2, 3, 4):
            with pytest.raises(NativeNotCovered):
                conv2d_mfma.conv2d_forward(xa.to(DEV), conv2d_mfma.pack_weight(wa.to(DEV), winograd=form), 64, 3, 3, pad=(1, 1), winograd=form, **kw)
        y = conv2d_mfma.conv2d_forward(xa.to(DEV), conv2d_mfma.pack_weight(wa.to(DEV), winograd=1), 64, 3, 3, pad=(1, 1), winograd=1, **kw)
        from oracle import ops_ref as R
        import torch.nn.functional as F
        ref = R.bias_act(F.conv2d(xa.double(), wa.double(), padding=1), None, act=kw['act'], alpha=kw.get('alpha'), gain=kw['gain'])
        close(y, ref, 0, 1e-5 * scale_of(ref))
    assert conv2d_mfma.use_winograd(3, 3, 1, 128, 128, pad=(1, 1), hw=(256, 256)) == F4
    assert conv2d_mfma.use_winograd(3, 3, 1, 128, 128, pad=(1, 1)) == 1                          # no image size: F(2x2)
    assert conv2d_mfma.use_winograd(3, 3, 1, 128, 128, pad=(1, 1), hw=(256, 254)) == 1          # width no multiple of 4
    assert conv2d_mfma.use_winograd(3, 3, 1, 128, 128, pad=(2, 2), hw=(256, 256)) == 1          # output width 258: no 16-byte row segments
    assert conv2d_mfma.use_winograd(3, 3, 1, 128, 128, pad=(1, 1), hw=(256, 256), xf=True) == 1  # input pre-activation: F(2x2) has the prologue
    assert conv2d_mfma.use_winograd(3, 3, 1, 96, 128, pad=(1, 1), hw=(256, 256)) == 1 and conv2d_mfma.use_winograd(3, 3, 1, 128, 32, pad=(1, 1), hw=(256, 256)) == 1
    assert conv2d_mfma.use_winograd(3, 3, 1, 512, 512, pad=(1, 1), hw=(16, 16)) == 1 and conv2d_mfma.use_winograd(3, 3, 1, 512, 512, pad=(1, 1), hw=(8, 8)) == 1 and conv2d_mfma.use_winograd(3, 3, 1, 512, 512, pad=(1, 1), hw=(32, 32)) == FN and conv2d_mfma.use_winograd(3, 3, 1, 16, 16, hw=(256, 256)) == 0
    x = det_tensor('w4d.x', [1, 16, 8, 66]).to(DEV)
    wt = det_tensor('w4d.w', [64, 16, 3, 3]).to(DEV)
    with pytest.raises(NativeNotCovered):
        conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(wt, winograd=2), 64, 3, 3, pad=(1, 1), winograd=2)        # W % 4 != 0
    with pytest.raises(NativeNotCovered):
        conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(wt, winograd=3), 64, 3, 3, pad=(1, 1), winograd=3)
    with pytest.raises(NativeNotCovered):
        conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(wt, winograd=4), 64, 3, 3, pad=(1, 1), winograd=4)
    # a form outside PG_WINO_*: the C entry points return PG_ERR_INVALID_ARG before anything is launched (valid pointers, an accepted geometry)
    import ctypes
    from torch_utils.ops import _native as nat
    lib = conv2d_mfma._init().lib
    xs = xa.to(DEV)
    pk = torch.zeros([lib.pg_conv2d_winograd_packed_size(conv2d_mfma.WINO_F4X3, 64, 64)], device=DEV)
    ys = torch.zeros([1, 64, 32, 64], device=DEV)
    for bad in (0, 5):
        with torch.cuda.device(xs.device):
            assert lib.pg_conv2d_winograd_pack_weight(bad, nat.ptr(wa.to(DEV)), nat.ptr(pk), 64, 64, 1.0, 0, 0, nat.stream_of(xs)) == -1
            assert lib.pg_conv2d_winograd_forward(bad, nat.ptr(xs), nat.ptr(pk), nat.ptr(ys), 1, 64, 32, 64, 64, 1, 1, 32, 64,
                                                  nat.i64arr(ys.stride()), ctypes.byref(conv2d_mfma.Fusion()), nat.stream_of(xs)) == -1
    torch.cuda.synchronize()
    assert not pk.any() and not ys.any()


def _winograd_exact_u(form, k, mult, scale, flip, transpose_oi):
    """U = G g G^T [co][ci][a][b] of the weight `mult * k` (`k` integers) as `pack_weight(..., scale, flip, transpose_oi)` reads it, exactly: G = GI / den with
    an integer GI, so U = (GI k GI^T) * (mult * scale / den^2) is integer arithmetic in float64."""
    g = k.double()
    if transpose_oi:                                  # the tensor is IOHW
        g = g.transpose(0, 1)
    if flip:
        g = g.flip(2, 3)
    if form == 1:
        GI, den = torch.tensor([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], dtype=torch.float64), 2
    else:
        GI, den = torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=torch.float64), 24
    return torch.einsum('ak,oikl,bl->oiab', GI, g, GI) * (mult * scale / den ** 2)


def _winograd_host_stream(form, U):
    """The operand stream of form `form` for the exact transformed weights U, from the layout comments of include/pasta_gan_ops.h / csrc/conv2d.hip: float32
    words (forms 1-3) or 16-bit words (form 4); rows and channels beyond Cout / Cin are zero."""
    cout, cin = U.shape[:2]
    coutp, cinp = -(-cout // 64) * 64, -(-cin // 16) * 16
    Up = torch.zeros([coutp, cinp, *U.shape[2:]], dtype=torch.float64)
    Up[:cout, :cin] = U
    if form == 1:        # [a][co / 32][ci / 2][ci & 1][co & 31][b]
        return Up.view(coutp // 32, 32, cinp // 2, 2, 4, 4).permute(4, 0, 2, 3, 1, 5).reshape(-1).float()
    if form == 2:        # [m-block 64][mt][a][chunk][jg][quad][jj][lane = (h, co & 31)][s]: b = 3 jg + jj, channel = 16 chunk + 2 (4 quad + s) + h
        return Up.view(coutp // 64, 2, 32, cinp // 16, 2, 4, 2, 6, 2, 3).permute(0, 1, 7, 3, 8, 4, 9, 6, 2, 5).reshape(-1).float()
    if form == 3:        # [m-block 64][cb 4][ah 2][chunk][e = 6 a' + b][lane = (kq, m 16)][j 4]: a = 3 ah + a', cout = 64 mb + 16 cb + m, channel = 16 chunk + 4 j + kq
        return Up.view(coutp // 64, 4, 16, cinp // 16, 4, 4, 2, 3, 6).permute(0, 1, 6, 3, 7, 8, 5, 2, 4).reshape(-1).float()
    # form 4: [m-block 64][mt][a][chunk][b 6][plane 3][lane = (h, co & 31)][j 8] 16-bit words, channel = 16 chunk + 2 j + h; planes = the truncation split of float32(U)
    u = Up.float()
    p0 = (u.view(torch.int32) & -65536).view(torch.float32)
    r = u - p0
    p1 = (r.view(torch.int32) & -65536).view(torch.float32)
    p2 = ((r - p1).view(torch.int32) & -65536).view(torch.float32)
    assert torch.equal(p0.double() + p1.double() + p2.double(), Up)                       # three bf16 planes hold it exactly
    planes = (torch.stack([p0, p1, p2], dim=-1).view(torch.int32) >> 16).to(torch.int16)  # [co][ci][a][b][plane]
    return planes.view(coutp // 64, 2, 32, cinp // 16, 8, 2, 6, 6, 3).permute(0, 1, 6, 3, 7, 8, 5, 2, 4).reshape(-1)


@pytest.mark.parametrize('form', [1, 2, 3, 4])
def test_winograd_pack_streams_equal_the_documented_layout(form):
    """The packed operand stream of every Winograd form, word for word against a host build of the documented layout (the convolution tests reach the streams
    only through their tolerances).  Exact by choice of input: weights of 576 x integers in [-8, 8] (F(2x2): 4 x) make every transformed weight an integer
    below 2^24; the kernel's float64 value is that integer up to ~2^-32 (G's sixths are not exact), so its ONE rounding to float32 gives the integer whatever
    the contraction of the arithmetic, and the three-plane bf16 split of it is exact.  Two things that premise needs, both asserted here:
      * the transformed weights are integer-valued (under scale = 0.5 the integers are the even ones of the range for that reason);
      * none of them is 0 inside Cout x Cin: where the exact value is 0 the float64 residue (~1e-14) is what float32 keeps, and no host build can predict
        it -- a 3x3 kernel whose transform has a zero is drawn again (about half of them).  The padded rows and channels are true zeros (of either sign: the
        16-bit words of form 4 are compared as the bf16 values they are).
    Shapes: one block; both paddings; several m-blocks and chunks.  Each plain, as a flipped IOHW weight, and scaled."""
    from torch_utils.ops import conv2d_mfma
    mult = 4.0 if form == 1 else 576.0
    gen = torch.Generator().manual_seed(1000 + form)
    for cout, cin in ((64, 16), (70, 20), (128, 48)):
        for scale, flip_t in ((1.0, False), (1.0, True), (0.5, False)):
            step = 1 if scale == 1.0 else 2

            def draw(shape):
                return torch.randint(-8 // step, 8 // step + 1, shape, generator=gen) * step

            k = draw([cin, cout, 3, 3] if flip_t else [cout, cin, 3, 3])
            for _ in range(64):
                U = _winograd_exact_u(form, k, mult, scale, flip_t, flip_t)
                redo = (U == 0).flatten(2).any(2)                   # [co][ci]
                if not redo.any():
                    break
                redo = redo.t() if flip_t else redo
                k[redo] = draw([int(redo.sum()), 3, 3])
            assert torch.equal(U, U.round()) and bool((U != 0).all()) and float(U.abs().max()) < 2 ** 24, 'the premise of the exact comparison'
            want = _winograd_host_stream(form, U)
            got = conv2d_mfma.pack_weight((k.float() * mult).to(DEV), scale=scale, flip=flip_t, transpose_oi=flip_t, winograd=form).cpu()
            if form == 4:
                got, want = got.view(torch.bfloat16), want.view(torch.bfloat16)
            assert got.shape == want.shape and torch.equal(got, want), (form, cout, cin, scale, flip_t)


@pytest.mark.parametrize('n,cin,cout,h,w', [(8, 128, 128, 256, 256), (8, 64, 64, 512, 512), (2, 512, 512, 64, 64), (2, 80, 70, 24, 72)])
def test_conv2d_winograd4_bf16x3_is_float32_class(n, cin, cout, h, w):
    """Form 4: F(4x4,3x3) with the 36 transform-domain GEMMs on v_mfma_f32_32x32x16_bf16 as the six largest plane products of exact three-term
    splits (u = u0 + u1 + u2, v = v0 + v1 + v2, 8 + 8 + 8 significand bits by truncation; dropped: u1 v2, u2 v1, u2 v2 < 2^-24 of the product), fp32 accumulation.
    Admissible as float32 only if it IS float32-class, so the referee is float64: the error of form 4 must stay within 2x the fp32-MFMA form's (form 2) on the same
    launch -- measured: 0.7-0.9x, the bf16 products are exact and only the accumulation rounds -- and within 1e-4 of the output scale like every F(4x4) launch;
    the two forms differ from each other by rounding only; repeated launches are bit-identical (fixed summation order, no atomics)."""
    from torch_utils.ops import conv2d_mfma
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(41)
    x = torch.randn([n, cin, h, w], generator=gen).to(DEV)
    wt = (torch.randn([cout, cin, 3, 3], generator=gen) / (3 * math.sqrt(cin))).to(DEV)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    sc = float(ref.abs().max())
    y2 = conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(wt, winograd=2), cout, 3, 3, pad=(1, 1), winograd=2)
    pk4 = conv2d_mfma.pack_weight(wt, winograd=4)
    y4 = conv2d_mfma.conv2d_forward(x, pk4, cout, 3, 3, pad=(1, 1), winograd=4)
    e2, e4 = float((y2.double() - ref).abs().max()), float((y4.double() - ref).abs().max())
    assert e4 <= 2 * e2 and e4 <= 1e-4 * sc, f'bf16x3 form {e4 / sc:.2e} of the output scale, fp32-MFMA form {e2 / sc:.2e}'
    assert float((y4 - y2).abs().max()) <= 4 * e2
    for _ in range(3):
        assert torch.equal(conv2d_mfma.conv2d_forward(x, pk4, cout, 3, 3, pad=(1, 1), winograd=4), y4)
    # the weight planes: 54 * CinP * CoutP float32 units = three bf16 planes of the 36 transformed weights; their sum is the fp32 form's transformed weight bit for bit
    cinp, coutp = -(-cin // 16) * 16, -(-cout // 64) * 64
    assert pk4.numel() == 54 * cinp * coutp
    u16 = pk4.view(torch.int16).view(-1, 6, 3, 64, 8).to(torch.int32)          # [unit = (m-block, mt, a, chunk)][b][plane][lane = (h, co & 31)][j]
    planes = (u16 << 16).view(torch.float32)
    usum = planes[:, :, 0].double() + planes[:, :, 1].double() + planes[:, :, 2].double()            # exact in float64
    assert torch.equal(usum.float().double(), usum)                                                    # ... and representable in float32: the split is exact
    pk2 = conv2d_mfma.pack_weight(wt, winograd=2).view(-1, 2, 2, 3, 64, 4)                             # [unit][jg][quad][jj][lane][s]: b = 3 jg + jj, channel pair = 4 quad + s
    u2 = pk2.permute(0, 1, 3, 4, 2, 5).reshape(-1, 6, 64, 8)                                           # [unit][b][lane][j = 4 quad + s]
    assert torch.equal(usum.float(), u2)


@pytest.mark.parametrize('n,cin,cout,h,w,kh,kw,pad,step', [(8, 512, 512, 8, 8, 2, 2, 1, 2), (4, 512, 96, 16, 16, 1, 1, 0, 1), (2, 256, 512, 32, 32, 3, 3, 1, 1),
                                                          (8, 512, 3, 16, 16, 1, 1, 0, 1), (3, 144, 40, 9, 13, 1, 2, 0, 2)])
def test_conv2d_split_k_matches_single_pass(n, cin, cout, h, w, kh, kw, pad, step, monkeypatch):
    """pg_conv2d_forward_splitk (low-resolution layers: several workgroups share a tile's K loop, fixed-order reduction + epilogue
    pass) against the fp64 convolution and against the single-pass kernel, with every epilogue stage and a strided phase write."""
    from torch_utils.ops import conv2d_mfma
    import torch.nn.functional as F
    lib = conv2d_mfma._init().lib
    oh, ow = h + 2 * pad - kh + 1, w + 2 * pad - kw + 1
    assert lib.pg_conv2d_splitk_plan(n, cin, oh, ow, cout, kh, kw, 1) > 1            # these shapes are the ones the planner splits
    x = det_tensor(f'sk.x.{cin}.{h}', [n, cin, h, w])
    wt = det_tensor(f'sk.w.{cin}.{cout}.{kh}{kw}', [cout, cin, kh, kw], scale=1 / math.sqrt(cin * kh * kw))
    styles = det_tensor(f'sk.s.{cin}', [n, cin]) + 1
    dco = det_tensor(f'sk.d.{cout}', [n, cout]).abs() + 0.5
    b = det_tensor(f'sk.b.{cout}', [cout])
    noise = det_tensor(f'sk.nz.{oh}', [oh, ow])
    big = det_tensor(f'sk.big.{cout}.{oh}', [n, cout, oh * step + 1, ow * step + 1])       # residual == output buffer layout (phase write)
    packed = conv2d_mfma.pack_weight(wt.to(DEV))
    kw_ = dict(in_scale=styles.to(DEV), out_scale=dco.to(DEV), noise=noise.to(DEV), noise_gain=0.7, bias=b.to(DEV), act='lrelu', alpha=0.2,
               gain=math.sqrt(2), clamp=3.0, out_hw=(oh, ow), out_step=(step, step), out_off=(step - 1, 0))
    outs = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('PG_CONV_SPLITK', mode)
        y = big.to(DEV).clone()
        conv2d_mfma.conv2d_forward(x.to(DEV), packed, cout, kh, kw, pad=(pad, pad), y=y, residual=y, **kw_)
        outs[mode] = y
    ref = F.conv2d((x * styles[:, :, None, None]).double(), wt.double(), padding=pad) * dco[:, :, None, None].double() + noise.double() * 0.7
    ref = torch.clamp(F.leaky_relu(ref + b.double()[None, :, None, None], 0.2) * math.sqrt(2), -3.0, 3.0)
    want = big.double().clone()
    want[:, :, step - 1::step, 0::step][:, :, :oh, :ow] += ref
    close(outs['1'], want, 1e-4, 1e-5 * scale_of(want))
    close(outs['1'], outs['0'], 1e-4, 5e-5)               # two fp32 summation orders of a K = Cin*taps dot product
    untouched = torch.ones_like(big, dtype=torch.bool)
    untouched[:, :, step - 1::step, 0::step][:, :, :oh, :ow] = False
    assert torch.equal(outs['1'].cpu()[untouched], big[untouched])                   # nothing outside the phase is written


def test_conv2d_two_source_equals_concat():
    """x2 / cin_split: conv over channels of two tensors == conv of their concatenation (merge_conv, networks.py:2179-2181)."""
    from torch_utils.ops import conv2d_mfma
    import torch.nn.functional as F
    for c1, c2, k in ((64, 64, 1), (128, 64, 1), (32, 5, 3), (16, 40, 3)):
        a, b = det_tensor(f'ts.a.{c1}', [2, c1, 19, 37]), det_tensor(f'ts.b.{c2}', [2, c2, 19, 37])
        w = det_tensor(f'ts.w.{c1}.{c2}', [70, c1 + c2, k, k], scale=0.1)
        s = det_tensor(f'ts.s.{c1}', [2, c1 + c2]) + 1
        y = conv2d_mfma.conv2d_forward(a.to(DEV), conv2d_mfma.pack_weight(w.to(DEV)), 70, k, k, pad=(k // 2, k // 2), x2=b.to(DEV), in_scale=s.to(DEV))
        ref = F.conv2d(torch.cat([a, b], 1) * s[:, :, None, None], w, padding=k // 2)
        close(y, ref, 1e-4, 1e-4)


def test_upfirdn2d_bias_act_fused_tail():
    from torch_utils.ops import upfirdn2d
    from oracle import ops_ref as R
    f = upfirdn2d.setup_filter(C.FIR_1331)
    x = det_tensor('ft.x', [2, 6, 33, 65])
    noise, noise_n = det_tensor('ft.n', [32, 64]), det_tensor('ft.nn', [2, 1, 32, 64])
    b = det_tensor('ft.b', [6])
    for nz in (None, noise, noise_n):
        for act, clamp in (('lrelu', 0.9), ('linear', None), ('relu', None)):
            y = upfirdn2d.upfirdn2d_bias_act(x.to(DEV), f.to(DEV), padding=[1, 1, 1, 1], gain=4, noise=None if nz is None else nz.to(DEV), b=b.to(DEV),
                                             act=act, alpha=0.2, act_gain=1.3, clamp=clamp)
            ref = R.upfirdn2d(x, f, padding=[1, 1, 1, 1], gain=4)
            if nz is not None:
                ref = ref + nz
            ref = R.bias_act(ref, b, act=act, alpha=0.2, gain=1.3, clamp=clamp)
            close(y, ref, 2e-5, 2e-5)
    assert upfirdn2d.upfirdn2d_bias_act(x.to(DEV), f.to(DEV), act='tanh') is None          # not fusable -> caller composes


@pytest.mark.parametrize('algo', ['direct', 'winograd'])
def test_conv2d_full_size_linearity_and_delta(algo, monkeypatch):
    """config-2 hottest conv shape, [8,64,512,512] * [64,64,3,3]: linearity in x and a delta-kernel identity (bit-exact on
    the direct kernel; to rounding of the transforms on the Winograd kernel)."""
    from torch_utils.ops import conv2d_gradfix
    monkeypatch.setenv('PG_CONV_ALGO', algo)
    same = torch.equal if algo == 'direct' else (lambda a, b: float((a - b).abs().max()) <= 2e-6 * float(b.abs().max()))
    gen = torch.Generator(device=DEV).manual_seed(3)
    x1 = torch.randn([8, 64, 512, 512], device=DEV, generator=gen)
    x2 = torch.randn([8, 64, 512, 512], device=DEV, generator=gen)
    w = torch.randn([64, 64, 3, 3], device=DEV, generator=gen) / 24
    y1, y2 = conv2d_gradfix.conv2d(x1, w, padding=1), conv2d_gradfix.conv2d(x2, w, padding=1)
    y12 = conv2d_gradfix.conv2d(x1 + 2 * x2, w, padding=1)
    assert float((y12 - (y1 + 2 * y2)).abs().max()) < 2e-4
    delta = torch.zeros([64, 64, 3, 3], device=DEV)
    delta[torch.arange(64), torch.arange(64), 1, 1] = 1
    assert same(conv2d_gradfix.conv2d(x1, delta, padding=1), x1)
    shift = torch.zeros([64, 64, 3, 3], device=DEV)
    shift[torch.arange(64), torch.arange(64), 0, 2] = 1        # y[oy,ox] = x[oy-1, ox+1]
    ys = conv2d_gradfix.conv2d(x1, shift, padding=1)
    assert same(ys[:, :, 1:, :-1], x1[:, :, :-1, 1:])


@pytest.mark.parametrize('n,c,h,w,sparse', [(2, 8, 16, 16, False), (1, 128, 64, 48, False), (3, 5, 9, 7, True)])
def test_spade_feat_assemble_vs_unfused_composition(n, c, h, w, sparse):
    """pg_spade_masked_sums + pg_spade_feat_assemble against the reference's elementwise composition
    (get_spade_feat, networks.py:2253-2276, and the merge, :2311-2316) evaluated on the CPU."""
    from torch_utils.ops import conv2d_mfma
    fu, fl = det_tensor(f'sfa.fu.{c}', [n, c, h, w]), det_tensor(f'sfa.fl.{c}', [n, c, h, w])
    thr = 1.2 if sparse else 0.0                 # sparse: almost no valid pixels -> the count <= 10 branch (divide by 256 * 256)
    mk = lambda name: (det_tensor(f'sfa.{name}.{c}', [n, 1, 2 * h, 2 * w]) > thr).float()
    mu, ml, du, dl = mk('mu'), mk('ml') * (1 - mk('mu')), mk('du'), mk('dl')

    def branch(feat, mask_512, denorm_mask):
        mask_256 = (mask_512[:, :, ::2, ::2] > 0.9).float()
        denorm_256 = (denorm_mask[:, :, ::2, ::2] > 0.9).float()
        valid = ((mask_256 + denorm_256) == 2.0).float()
        res = mask_256 - valid
        vsum = torch.sum(feat * valid, dim=(2, 3), keepdim=True)
        cnt = torch.sum(valid, dim=(2, 3), keepdim=True)
        idx = (cnt > 10).float()
        cnt = cnt * idx + (256 * 256) * (1 - idx)
        return feat * (1 - res) + (vsum / cnt) * res, mask_256
    bu, m_u = branch(fu, mu, du)
    bl, m_l = branch(fl, ml, dl)
    want = bu * m_u + bl * m_l
    got = conv2d_mfma.spade_feat_assemble(fu.to(DEV), fl.to(DEV), mu.to(DEV), ml.to(DEV), du.to(DEV), dl.to(DEV))
    close(got, want, 1e-5, 1e-6)
    untouched = ((m_u + m_l) == 0).expand_as(want)
    assert float(got.cpu()[untouched].abs().max()) == 0.0          # outside both masks the result is exactly zero


def test_support_kernels_vs_oracle():
    from torch_utils.ops import conv2d_mfma
    from oracle import network_ref as NR
    x = det_tensor('in.x', [2, 6, 37, 41], scale=3.0) + 5.0
    gamma, beta = det_tensor('in.g', x.shape), det_tensor('in.b', x.shape)
    mean, rstd = conv2d_mfma.instance_norm_stats(x.to(DEV))
    y = conv2d_mfma.spade_norm(x.to(DEV), mean, rstd, gamma.to(DEV), beta.to(DEV))
    close(y, NR.instance_norm(x) * (1 + gamma) + beta, 2e-5, 2e-5)
    close(mean.view(2, 6), x.mean(dim=(2, 3)), 1e-6, 1e-6)
    w = det_tensor('dc.w', [10, 7, 3, 3])
    s = det_tensor('dc.s', [3, 7]) + 1
    d = conv2d_mfma.modconv_dcoefs(w.to(DEV), s.to(DEV))
    ref = ((w[None] * s[:, None, :, None, None]).square().sum(dim=(2, 3, 4)) + 1e-8).rsqrt()
    close(d, ref, 1e-5, 1e-6)
    # the cached-tap-energy form used by the network routes, plain and with the half-precision pre-normalisation
    w2 = conv2d_mfma.modconv_w2(w.to(DEV))
    close(w2, w.square().sum(dim=(2, 3)), 1e-6, 1e-6)
    d2, none_a, none_b = conv2d_mfma.modconv_prep(w2, s.to(DEV), 10)
    assert none_a is None and none_b is None
    close(d2, ref, 1e-5, 1e-6)
    wide_w, wide_s = det_tensor('dc.ww', [70, 300, 3, 3]), det_tensor('dc.ws', [5, 300], scale=4.0)
    smax = wide_s.abs().amax(dim=1, keepdim=True)
    sn = wide_s / smax
    for dt in (torch.bfloat16, torch.float16):
        out, s_norm, s16 = conv2d_mfma.modconv_prep(conv2d_mfma.modconv_w2(wide_w.to(DEV)), wide_s.to(DEV), 70, normalize=True, half_dtype=dt)
        close(s_norm, sn, 1e-6, 1e-7)
        assert s16.dtype == dt and torch.equal(s16.cpu(), sn.to(dt))
        close(out, ((wide_w[None] * sn[:, None, :, None, None]).square().sum(dim=(2, 3, 4)) + 1e-8).rsqrt(), 1e-5, 1e-6)
    out, s_norm, s16 = conv2d_mfma.modconv_prep(None, wide_s.to(DEV), 70, normalize=True, demodulate=False, half_dtype=torch.bfloat16)
    close(out, smax.expand(5, 70), 0, 0)


# =============================================================== conv2d_resample / modulated_conv2d

@pytest.mark.parametrize('case', C.CONV2D_RESAMPLE_CASES, ids=[c[0] for c in C.CONV2D_RESAMPLE_CASES])
def test_conv2d_resample_golden(golden, case):
    from torch_utils.ops import conv2d_resample, upfirdn2d
    g = golden('g3_conv2d_resample.npz')
    name, xs, wsh, taps, up, down, pad, groups, flipw = case
    f = upfirdn2d.setup_filter(taps).to(DEV)
    x = det_tensor(name + '.x', xs).to(DEV).requires_grad_(True)
    w = det_tensor(name + '.w', wsh, scale=1 / math.sqrt(wsh[1] * wsh[2] * wsh[3])).to(DEV).requires_grad_(True)
    y = conv2d_resample.conv2d_resample(x, w, f=f, up=up, down=down, padding=pad, groups=groups, flip_weight=flipw)
    close(y, g[f'{name}/y'], 1e-4, 2e-5)
    dx, dw = torch.autograd.grad(y, [x, w], det_tensor(name + '.dy', y.shape).to(DEV))
    close(dx, g[f'{name}/dx'], 1e-3, 5e-5)
    close(dw, g[f'{name}/dw'], 1e-3, 1e-4)


@pytest.mark.parametrize('grad', [False, True], ids=['inference_route', 'graph_route'])
@pytest.mark.parametrize('case', C.MODCONV_CASES, ids=[c[0] for c in C.MODCONV_CASES])
def test_modulated_conv2d_golden(golden, case, grad):
    from training import networks
    from torch_utils.ops import upfirdn2d
    g = golden('g4_modconv.npz')
    name, n, cin, cout, k, h, up, demod, fused, noise_kind = case
    f = upfirdn2d.setup_filter(C.FIR_1331).to(DEV)
    x = det_tensor(name + '.x', [n, cin, h, h]).to(DEV)
    w = det_tensor(name + '.w', [cout, cin, k, k]).to(DEV).requires_grad_(grad)
    s = (det_tensor(name + '.s', [n, cin]) + 1.0).to(DEV)
    hh = h * up
    noise = {'none': None, 'const': det_tensor(name + '.noise', [hh, hh]) * 0.1,
             'per_sample': det_tensor(name + '.noise', [n, 1, hh, hh]) * 0.1}[noise_kind]
    noise = noise.to(DEV) if noise is not None else None
    y = networks.modulated_conv2d(x=x.clone(), weight=w, styles=s, noise=noise, up=up, padding=k // 2, resample_filter=f,
                                  demodulate=demod, flip_weight=(up == 1), fused_modconv=fused)
    close(y, g[f'{name}/y'], 2e-4, 5e-5)


# =============================================================== blocks and the synthesis network

def _load(mod_cls, ref_mod):
    """Build the product module with the oracle module's parameters/buffers (same names)."""
    missing, unexpected = mod_cls.load_state_dict(ref_mod.state_dict(), strict=False)
    assert not [m for m in missing if 'resample_filter' not in m], missing
    assert not unexpected, unexpected
    return mod_cls.to(DEV).eval()


def test_blocks_golden(golden):
    from training import networks as PN
    from oracle import network_ref as NR
    g = golden('g5_blocks.npz')
    tol = dict(rtol=3e-4, atol=5e-5)
    with torch.no_grad():
        blk = _load(PN.Spade_ResBlockV4_512(8, 8, spade_channels=5), fill_module_(NR.Spade_ResBlockV4_512(8, 8, spade_channels=5), 'g5.spade.'))
        close(blk(det_tensor('g5.spade.x', [2, 8, 24, 24]).to(DEV), det_tensor('g5.spade.feat', [2, 5, 24, 24]).to(DEV)), g['spade/y'], **tol)
        rb = _load(PN.ResBlock(6, 10, kernel_size=4, activation='relu', down=2), fill_module_(NR.ResBlock(6, 10, activation='relu', down=2), 'g5.resdown.'))
        close(rb(det_tensor('g5.resdown.x', [2, 6, 32, 32]).to(DEV)), g['resdown/y'], **tol)
        rb1 = _load(PN.ResBlock(6, 6, kernel_size=4, activation='relu'), fill_module_(NR.ResBlock(6, 6, activation='relu'), 'g5.res.'))
        close(rb1(det_tensor('g5.res.x', [2, 6, 20, 20]).to(DEV)), g['res/y'], **tol)
        c7 = _load(PN.Conv2dLayer(3, 8, kernel_size=7, activation='relu'), fill_module_(NR.Conv2dLayer(3, 8, kernel_size=7, activation='relu'), 'g5.conv7.'))
        close(c7(det_tensor('g5.conv7.x', [2, 3, 20, 20]).to(DEV)), g['conv7/y'], **tol)
        cup = _load(PN.Conv2dLayer(4, 6, kernel_size=3, activation='lrelu', up=2, conv_clamp=0.5),
                    fill_module_(NR.Conv2dLayer(4, 6, kernel_size=3, activation='lrelu', up=2, conv_clamp=0.5), 'g5.convup.'))
        close(cup(det_tensor('g5.convup.x', [2, 4, 8, 8]).to(DEV), gain=math.sqrt(0.5)), g['convup/y'], **tol)
        fc = _load(PN.FullyConnectedLayer(12, 7, bias_init=1), fill_module_(NR.FullyConnectedLayer(12, 7, bias_init=1), 'g5.fc.'))
        close(fc(det_tensor('g5.fc.x', [3, 12]).to(DEV)), g['fc/y'], **tol)
        fca = _load(PN.FullyConnectedLayer(12, 7, activation='lrelu', lr_multiplier=0.01),
                    fill_module_(NR.FullyConnectedLayer(12, 7, activation='lrelu', lr_multiplier=0.01), 'g5.fca.'))
        close(fca(det_tensor('g5.fca.x', [3, 12]).to(DEV)), g['fca/y'], **tol)
        sl = _load(PN.SynthesisLayer(5, 6, w_dim=12, resolution=16, up=2, conv_clamp=256),
                   fill_module_(NR.SynthesisLayer(5, 6, w_dim=12, resolution=16, up=2, conv_clamp=256), 'g5.synup.'))
        xw = det_tensor('g5.synup.x', [2, 5, 8, 8]).to(DEV), det_tensor('g5.synup.w', [2, 12]).to(DEV)
        close(sl(*xw, noise_mode='const', fused_modconv=True), g['synup_fused/y'], **tol)
        close(sl(*xw, noise_mode='const', fused_modconv=False, gain=math.sqrt(0.5)), g['synup_nonfused/y'], **tol)
        tr = _load(PN.ToRGBLayerFull_v1_v5(6, 3, w_dim=12, conv_clamp=256, is_last=True, is_style=True),
                   fill_module_(NR.ToRGBLayerFull(6, 3, w_dim=12, conv_clamp=256, is_last=True, is_style=True), 'g5.torgb.'))
        yi, yp = tr(det_tensor('g5.torgb.x', [2, 6, 16, 16]).to(DEV), det_tensor('g5.torgb.w', [2, 12]).to(DEV))
        close(yi, g['torgb/img'], **tol)
        close(yp, g['torgb/parsing'], **tol)


@pytest.mark.parametrize('algo', ['direct', 'winograd'])
@pytest.mark.parametrize('c,feat_c,h,w', [(64, 5, 24, 40), (128, 16, 17, 33), (32, 1, 32, 32)])
def test_spade_norm_block_fused_gamma_beta(c, feat_c, h, w, algo, monkeypatch):
    """C % 32 == 0 takes the single-launch gamma/beta convolution with the SPADE combine epilogue (both conv kernels)."""
    from training import networks as PN
    from oracle import network_ref as NR
    monkeypatch.setenv('PG_CONV_ALGO', algo)
    ref = fill_module_(NR.Spade_Norm_Block(feat_c, c), f'snb.{c}.')
    net = _load(PN.Spade_Norm_Block(feat_c, c), ref)
    x = det_tensor(f'snb.x.{c}', [2, c, h, w], scale=2.0) + 0.5
    feat = det_tensor(f'snb.f.{c}', [2, feat_c, h, w])
    with torch.no_grad():
        y = net(x.to(DEV), feat.to(DEV))
        want = ref(x, feat)
    close(y, want, 2e-4, 2e-5 * scale_of(want))
    assert ('gamma_beta', algo == 'winograd') in net._cache._store        # the fused route really ran, on the requested kernel


def test_blocks_graph_route_matches_inference_route():
    """The differentiable composition and the fused single-launch route agree, and gradients flow."""
    from training import networks as PN
    blk = fill_module_(PN.Spade_ResBlockV4_512(8, 8, spade_channels=5), 'gr.spade.').to(DEV)
    x, feat = det_tensor('gr.x', [2, 8, 24, 24]).to(DEV), det_tensor('gr.f', [2, 5, 24, 24]).to(DEV)
    with torch.no_grad():
        y_fast = blk(x, feat)
    y_graph = blk(x.clone().requires_grad_(True), feat)
    close(y_graph, y_fast, 2e-4, 5e-5)
    y_graph.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in blk.parameters())
    sl = fill_module_(PN.SynthesisLayer(5, 6, w_dim=12, resolution=16, up=2, conv_clamp=256), 'gr.syn.').to(DEV)
    xw = det_tensor('gr.sx', [2, 5, 8, 8]).to(DEV), det_tensor('gr.sw', [2, 12]).to(DEV)
    with torch.no_grad():
        a = sl(*xw, noise_mode='const')
    b = sl(*xw, noise_mode='const', fused_modconv=False)
    close(b, a, 2e-4, 5e-5)
    b.sum().backward()
    assert sl.weight.grad is not None and sl.affine.weight.grad is not None


@pytest.mark.parametrize('variant,labels', [('labels', True), ('argmax', False)])
def test_synthesis_reduced_golden(golden, variant, labels):
    """512x512, reduced-width SynthesisNetworkFull_v18 on the GPU vs the REFERENCE's own classes (G6)."""
    from training import networks as PN
    from oracle import network_ref as NR
    g = golden('g6_synthesis.npz')
    torch.manual_seed(0)
    ref_net = fill_module_(NR.SynthesisNetworkFull_v18(**C.G6_KW), 'g6.')
    net = _load(PN.SynthesisNetworkFull_v18(**C.G6_KW), ref_net)
    assert sorted(n for n, _ in net.named_parameters()) == list(g['param_names'])
    inp = synthesis_inputs(1, w_dim=C.G6_KW['w_dim'], num_ws=net.num_ws, feat_ch=C.G6_FEAT_CH, seed_tag='g6', labels=labels)
    to = lambda t: t.to(DEV) if t is not None else None
    with torch.no_grad():
        img, fimg, pp = net(to(inp['ws']), to(inp['pose_feat']), {k: v.to(DEV) for k, v in inp['cat_feat'].items()},
                            to(inp['denorm_upper_input']), to(inp['denorm_lower_input']), to(inp['denorm_upper_mask']),
                            to(inp['denorm_lower_mask']), to(inp['gt_parsing']), noise_mode='const')
    y0, y1, x0, x1 = C.G6_CROP
    for nm, t in (('img', img), ('finetune_img', fimg), ('pred_parsing', pp)):
        s = scale_of(g[f'{variant}/{nm}_sub'])
        close(t[..., ::C.G6_SUB, ::C.G6_SUB], g[f'{variant}/{nm}_sub'], 1e-3, 1e-3 * s)     # north_star: <= 1e-3 of the pixel range
        close(t[..., y0:y1, x0:x1], g[f'{variant}/{nm}_crop'], 1e-3, 1e-3 * s)
        np.testing.assert_allclose(float(t.double().abs().sum()), float(g[f'{variant}/{nm}_abssum']), rtol=1e-4)


def _pixel_bar(nm, a, b, what=''):
    """north_star: <= 1e-3 max-abs delta vs the reference ops, ABSOLUTE (the random-weight outputs span 15-115, so a bar
    relative to the range was ~100x looser than stated).  Returns the measured delta."""
    delta = float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())
    assert delta <= 1e-3, f'{what}{nm}: max-abs delta {delta:.3e} > 1e-3 (output range {scale_of(b):.3e})'
    return delta


def test_synthesis_full_width_vs_oracle():
    """BASELINE config 2's network (channel_base 32768, 27.6 M parameters), N=1, against the CPU oracle."""
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(w_dim=512, img_resolution=512, img_channels=3, channel_base=32768, channel_max=512, conv_clamp=256)
    torch.manual_seed(0)
    ref_net = fill_module_(NR.SynthesisNetworkFull_v18(**kw), 'cfg2.').eval()
    net = _load(PN.SynthesisNetworkFull_v18(**kw), ref_net)
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref_net.parameters())
    inp = synthesis_inputs(1, labels=True)
    args = lambda f: (f(inp['ws']), f(inp['pose_feat']), {k: f(v) for k, v in inp['cat_feat'].items()}, f(inp['denorm_upper_input']),
                      f(inp['denorm_lower_input']), f(inp['denorm_upper_mask']), f(inp['denorm_lower_mask']), f(inp['gt_parsing']))
    with torch.no_grad():
        out = net(*args(lambda t: t.to(DEV)), noise_mode='const')
        ref = ref_net(*args(lambda t: t), noise_mode='const')
    for nm, a, b in zip(('img', 'finetune_img', 'pred_parsing'), out, ref):
        print(f'config 2 N=1 {nm}: max-abs delta {_pixel_bar(nm, a, b):.2e} (range {scale_of(b):.1f})')


# =============================================================== "next" row f1: encoders, mapping, full generator

def test_encoders_and_mapping_golden(golden):
    from training import networks as PN
    from oracle import network_ref as NR
    g = golden('g7_encoders.npz')
    tol = dict(rtol=3e-4, atol=5e-5)
    with torch.no_grad():
        ce = _load(PN.ConstEncoderNetwork(input_nc=5, output_nc=64, ngf=8, n_downsampling=6),
                   fill_module_(NR.ConstEncoderNetwork(input_nc=5, output_nc=64, ngf=8, n_downsampling=6), 'g7.const.'))
        close(ce(det_tensor('g7.const.x', [2, 5, 128, 128], 'uniform').to(DEV)), g['const/y'], **tol)
        se = _load(PN.StyleEncoderNetworkV18(input_nc=45, output_nc=64, ngf=8, n_downsampling=6),
                   fill_module_(NR.StyleEncoderNetworkV18(input_nc=45, output_nc=64, ngf=8, n_downsampling=6), 'g7.style.'))
        code, feats = se(det_tensor('g7.style.parts', [2, 45, 32, 32], 'uniform').to(DEV), det_tensor('g7.style.retain', [2, 6, 64, 64], 'uniform').to(DEV))
        close(code, g['style/code'], rtol=2e-3, atol=2e-4)
        for i, f in enumerate(feats):
            close(f, g[f'style/feat{i}'], **tol)
        mp = _load(PN.MappingNetwork(z_dim=0, c_dim=64, w_dim=32, num_ws=14, num_layers=1),
                   fill_module_(NR.MappingNetwork(z_dim=0, c_dim=64, w_dim=32, num_ws=14, num_layers=1), 'g7.map.'))
        close(mp(torch.zeros([2, 0], device=DEV), det_tensor('g7.map.c', [2, 64]).to(DEV)), g['map/ws'], **tol)
        ref2 = fill_module_(NR.MappingNetwork(z_dim=16, c_dim=8, w_dim=32, num_ws=5, num_layers=3), 'g7.map2.')
        ref2.w_avg.copy_(det_tensor('g7.map2.w_avg', [32]))
        mp2 = _load(PN.MappingNetwork(z_dim=16, c_dim=8, w_dim=32, num_ws=5, num_layers=3), ref2)
        close(mp2(det_tensor('g7.map2.z', [3, 16]).to(DEV), det_tensor('g7.map2.c', [3, 8]).to(DEV), truncation_psi=0.7, truncation_cutoff=3), g['map2/ws'], **tol)
        dn = _load(PN.Dense(6, 10), fill_module_(NR.Dense(6, 10), 'g7.dense.'))
        close(dn(det_tensor('g7.dense.x', [2, 6, 9, 11]).to(DEV)), g['dense/y'], **tol)


def test_full_generator_vs_oracle():
    """BASELINE config 3's network (GeneratorFull_v20: encoders + mapping + synthesis, full width) at N=1 vs the CPU oracle."""
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
              synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256))
    torch.manual_seed(0)
    ref = fill_module_(NR.GeneratorFull_v20(**kw), 'cfg3.').eval()
    net = _load(PN.GeneratorFull_v20(**kw), ref)
    n = 1
    inp = dict(z=torch.zeros([n, 0]), c=det_tensor('cfg3.parts', [n, 45, 128, 128], 'uniform'), retain=det_tensor('cfg3.retain', [n, 6, 512, 512], 'uniform'),
               pose=det_tensor('cfg3.pose', [n, 5, 512, 512], 'uniform'), du=det_tensor('cfg3.du', [n, 3, 512, 512], 'uniform'),
               dl=det_tensor('cfg3.dl', [n, 3, 512, 512], 'uniform'), mu=det_tensor('cfg3.mu', [n, 1, 512, 512], 'blockmask'),
               ml=det_tensor('cfg3.ml', [n, 1, 512, 512], 'blockmask'), gt=det_tensor('cfg3.gt', [n, 1, 512, 512], 'labels7'))
    call = lambda m, f: m(f(inp['z']), f(inp['c']), f(inp['retain']), f(inp['pose']), f(inp['du']), f(inp['dl']), f(inp['mu']), f(inp['ml']),
                          gt_parsing=f(inp['gt']), noise_mode='const')
    with torch.no_grad():
        out = call(net, lambda t: t.to(DEV))
        want = call(ref, lambda t: t)
    for nm, a, b in zip(('img', 'finetune_img', 'pred_parsing'), out, want):
        print(f'config 3 N=1 {nm}: max-abs delta {_pixel_bar(nm, a, b):.2e} (range {scale_of(b):.1f})')


def test_discriminator_with_r1_double_backward_golden(golden):
    """Row f2 on the GPU: training-mode Discriminator (graph route) incl. the R1 double backward through the HIP ops'
    own gradient kernels (bias_act grad 1 re-applied, upfirdn2d transposed) and aten's conv double-backward."""
    from training import networks as PN
    from oracle import network_ref as NR
    g = golden('g8_discriminator.npz')
    kw = dict(c_dim=16, img_resolution=32, img_channels=6, channel_base=512, channel_max=32, conv_clamp=256,
              mapping_kwargs=dict(num_layers=2), epilogue_kwargs=dict(mbstd_group_size=2))
    d = PN.Discriminator(**kw)
    d.load_state_dict(fill_module_(NR.Discriminator(**kw), 'g8.d.').state_dict(), strict=False)
    d = d.to(DEV).train()
    assert [n for n, _ in d.named_parameters()] == list(g['r1_grad_names'])
    img = det_tensor('g8.img', [4, 6, 32, 32], 'uniform').to(DEV).requires_grad_(True)
    c = det_tensor('g8.c', [4, 16]).to(DEV)
    logits = d(img, c)
    close(logits, g['logits'], 1e-3, 1e-4)
    with torch.no_grad():
        close(d(img.detach(), c), g['logits'], 1e-3, 1e-4)          # inference route gives the same logits
    gi, = torch.autograd.grad(logits.sum(), img, create_graph=True)
    pen = gi.square().sum([1, 2, 3])
    close(pen, g['r1_penalty'], 2e-3, 1e-6)
    grads = torch.autograd.grad(pen.sum(), list(d.parameters()), allow_unused=True)
    got = np.array([float(x.abs().sum()) if x is not None else 0.0 for x in grads])
    np.testing.assert_allclose(got, g['r1_grad_abssum'], rtol=5e-3, atol=1e-6)


# =============================================================== training step (config 4 rows)

def _d_kw(img_channels):
    return dict(c_dim=6, img_resolution=16, img_channels=img_channels, channel_base=256, channel_max=32, conv_clamp=256,
                mapping_kwargs=dict(num_layers=1), epilogue_kwargs=dict(mbstd_group_size=2))


@pytest.mark.parametrize('phase', ['Dboth', 'D_parsingboth', 'Gmain'])
def test_training_phase_gradients_vs_oracle(phase):
    """The product discriminators (HIP ops, graph route, R1 double backward) inside the product loss on the GPU against the
    oracle discriminators inside the same loss on the CPU; generator side = the plain-torch stub networks."""
    import stubs
    from training import networks as PN
    from training.loss import StyleGAN2Loss
    from oracle import network_ref as NR

    def run(device, D_cls):
        nets = stubs.build(device)
        for name, ch in (('D', 6), ('D_parsing', 10)):
            ref = fill_module_(NR.Discriminator(**_d_kw(ch)), f'tp.{name}.')
            d = D_cls(**_d_kw(ch))
            d.load_state_dict(ref.state_dict(), strict=False)
            nets[name] = d.to(device).train()
        loss = StyleGAN2Loss(device=torch.device(device), **nets, style_mixing_prob=0, r1_gamma=10, l1_weight=50, mask_weight=1.0)
        stubs.zero_grads(nets)
        stubs.set_phase_trainable(nets, phase)
        loss.accumulate_gradients(phase=phase, gain=1, **stubs.batch(4, device))
        return stubs.grad_signature(nets)

    got, want = run(DEV, PN.Discriminator), run('cpu', NR.Discriminator)
    assert got.keys() == want.keys()
    for k in want:
        assert abs(got[k] - want[k]) <= 3e-3 * abs(want[k]) + 1e-6, (k, got[k], want[k])
    assert any(v > 0 for v in got.values())


@pytest.mark.parametrize('phase', ['Dboth', 'Gmain'])
def test_config4_discriminators_at_real_shape_vs_oracle(phase):
    """BASELINE config 4's discriminators at their REAL shape and per-rank batch (train.py:174, 196-198: 512^2, channel_base 32768,
    conv_clamp 256, minibatch-std groups of 4, batch_gpu 4) inside the product loss on the GPU against the oracle discriminators in
    the same loss on the CPU: `Dboth` = both backward passes of the D phase incl. the R1 double backward (weight gradients of every
    layer, native wgrad kernels included); `Gmain` = the generator phase, i.e. the discriminators' INPUT gradients flowing into the
    (plain-torch stub) generator at 512^2.  fp32 on both sides; per-parameter sum|grad| within 3e-3."""
    import stubs
    from training import networks as PN
    from training.loss import StyleGAN2Loss
    from oracle import network_ref as NR
    res, n = 512, 4
    d_kw = lambda ch: dict(c_dim=stubs.CDIM, img_resolution=res, img_channels=ch, channel_base=32768, channel_max=512, conv_clamp=256,
                           mapping_kwargs=dict(num_layers=1), epilogue_kwargs=dict(mbstd_group_size=4))

    def run(device, D_cls):
        nets = stubs.build(device)
        for name, ch in (('D', 6), ('D_parsing', 10)):
            ref = fill_module_(NR.Discriminator(**d_kw(ch)), f'c4.{name}.')
            d = D_cls(**d_kw(ch))
            d.load_state_dict(ref.state_dict(), strict=False)
            nets[name] = d.to(device).train()
        loss = StyleGAN2Loss(device=torch.device(device), **nets, style_mixing_prob=0, r1_gamma=10, l1_weight=50, mask_weight=1.0)
        stubs.zero_grads(nets)
        stubs.set_phase_trainable(nets, phase)
        loss.accumulate_gradients(phase=phase, gain=1, **stubs.batch(n, device, res=res))
        full.append({f'{mn}.{pn}': (None if p_.grad is None else p_.grad.detach().cpu().clone()) for mn, m in nets.items() for pn, p_ in m.named_parameters()})
        return stubs.grad_signature(nets)

    full = []
    torch.set_num_threads(min(16, len(__import__('os').sched_getaffinity(0))))
    got, want = run(DEV, PN.Discriminator), run('cpu', NR.Discriminator)
    assert got.keys() == want.keys()
    ew, ew_name, ew_n = _elementwise_gradient_mismatch(full[0], full[1])
    print(f'config 4 {phase} at 512^2, N=4: element-wise gradient mismatch over {ew_n} tensors, worst {ew:.2e} of the tensor maximum ({ew_name})')
    assert ew <= 3e-3 and ew_n >= 4, (ew, ew_name, ew_n)
    worst = max((abs(got[k] - want[k]) / (abs(want[k]) + 1e-12), k) for k in want if want[k] > 0)
    print(f'config 4 {phase} at 512^2, N=4: {sum(1 for v in want.values() if v > 0)} parameters with gradients, worst signature mismatch {worst[0]:.2e} ({worst[1]})')
    for k in want:
        assert abs(got[k] - want[k]) <= 3e-3 * abs(want[k]) + 1e-6, (k, got[k], want[k])
    assert sum(1 for k, v in got.items() if v > 0 and k.startswith('D.' if phase == 'Dboth' else 'G_')) >= 4


def _elementwise_gradient_mismatch(got, want, skip=('noise_strength',), stats=None):
    """Element-wise comparison of two {name: gradient tensor or None} dicts (a per-parameter sum|grad| cannot see a transposed, permuted or
    sign-flipped gradient inside a tensor): for every tensor with more than one element, max|got - want| / max|want|.  Returns (worst ratio, its name, n compared)."""
    worst, n, table = (0.0, ''), 0, []
    # tensors whose true gradient is zero (a bias in front of an instance norm, say) carry float32 rounding noise on both sides, ~1e-10 beside gradients of
    # ~1e-2: anything below 1e-6 of the network's largest gradient element is checked for being that small on both sides, not element by element
    top = max([float(w.abs().max()) for w in want.values() if w is not None and w.numel() > 0] + [0.0])
    for k, w in want.items():
        if w is None or w.numel() <= 1 or any(k.endswith(sfx) for sfx in skip):
            continue
        g = got[k]
        assert g is not None and g.shape == w.shape, k
        scale = float(w.abs().max())
        if scale <= 1e-6 * top:
            assert float(g.abs().max()) <= 1e-5 * top, (k, float(g.abs().max()), top)
            if stats is not None:
                stats.setdefault('skipped', []).append(k)        # (callers that must not compare vacuously look at these)
            continue
        n += 1
        if stats is not None:
            stats.setdefault('compared', []).append(k)
        e = float((g.double() - w.double()).abs().max()) / scale
        cos = float((g.double() * w.double()).sum() / (g.double().norm() * w.double().norm() + 1e-300))
        table.append((e, k, scale, float(g.abs().max()), cos))
        worst = max(worst, (e, k))
    table.sort(reverse=True)
    print('  largest element-wise mismatches (ratio, name, max|want|, max|got|, cosine): ' + '; '.join(f'{e:.2e} {k} {sw:.2e} {sg:.2e} {c:+.4f}' for e, k, sw, sg, c in table[:6]))
    return worst[0], worst[1], n


def test_config4_generator_gradients_full_width_vs_oracle():
    """The TRAINING route of the full-width synthesis network (BASELINE config 4's generator: channel_base 32768, 512^2; modulated
    convolutions on the graph route, native input gradients incl. the F(4x4) kernel with flipped / transposed packs, native weight gradients,
    transposed-conv and FIR gradients, SPADE blocks) against the CPU oracle's autograd on the same weights and inputs, N = 1: a fixed random
    linear functional of the three outputs, per-parameter sum|grad| within 2e-3 (float32 sums over up to 2.6e5 pixels in different orders).
    The encoder's 7x7 layer and every other parameter with a gradient are covered; parameters without one must have none on both sides."""
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(w_dim=512, img_resolution=512, img_channels=3, channel_base=32768, channel_max=512, conv_clamp=256)
    ref_net = fill_module_(NR.SynthesisNetworkFull_v18(**kw), 'cfg2.').train()
    net = PN.SynthesisNetworkFull_v18(**kw)
    missing, unexpected = net.load_state_dict(ref_net.state_dict(), strict=False)
    assert not unexpected and not [m for m in missing if 'resample_filter' not in m]
    net = net.to(DEV).train()
    inp = synthesis_inputs(1, labels=True)
    proj = [det_tensor(f'c4g.proj{i}', shp) for i, shp in enumerate(([1, 3, 512, 512], [1, 3, 512, 512], [1, 7, 512, 512]))]
    args = lambda f: (f(inp['ws']), f(inp['pose_feat']), {k: f(v) for k, v in inp['cat_feat'].items()}, f(inp['denorm_upper_input']),
                      f(inp['denorm_lower_input']), f(inp['denorm_upper_mask']), f(inp['denorm_lower_mask']), f(inp['gt_parsing']))

    full = {}

    def signature(model, f, tag):
        for p_ in model.parameters():
            p_.grad = None
        out = model(*args(f), noise_mode='const')
        sum((o * f(r)).sum() for o, r in zip(out, proj)).backward()
        full[tag] = {n_: (None if p_.grad is None else p_.grad.detach().cpu().clone()) for n_, p_ in model.named_parameters()}
        return {n_: (None if p_.grad is None else float(p_.grad.double().abs().sum())) for n_, p_ in model.named_parameters()}

    torch.set_num_threads(min(16, len(__import__('os').sched_getaffinity(0))))
    got = signature(net, lambda t: t.to(DEV), 'got')
    want = signature(ref_net, lambda t: t, 'want')
    assert got.keys() == want.keys()
    # ELEMENT-WISE (round 5): every weight / bias gradient tensor of the network -- the F(4x4)-dgrad 3x3 layers of every resolution, the up = 2 layers,
    # the ToRGB heads, the SPADE gamma / beta convolutions, the affine layers.  Measured first against the float32 oracle: 153 of 155 tensors within
    # 2e-3 of their largest element, the worst (spade_b256_2.conv0.weight) at 1.5e-2 -- a weight gradient there is a sum over 65 536 pixels of terms that
    # cancel to ~1/250 of their absolute sum, so the float32 ORACLE is no better.  The referee is therefore the same oracle network in FLOAT64: every tensor of
    # the GPU route must be within 3e-3 of its largest element, or within 10x the float32 oracle's own distance from the float64 gradient (measured: 3-4.3x on the
    # tensors behind F(4x4,3x3) layers, whose transforms round ~4x coarser than a direct convolution -- tools/f43_error_probe.py) and never beyond 3e-2.
    # (The first bar was 2e-3 until the split-K form of the 8^2 / 16^2 up-convolutions arrived: its forward is 3-4x CLOSER to float64 than the single-share
    # kernel -- tools/probes/up2_splitk_error.py: 3.7e-7 against 1.6e-6 of the output's maximum -- yet the six b512 tensors moved from < 2e-3 to 2.1e-3 ... 2.6e-3:
    # at that level the draw of fp32 roundings in the F(4x4) forward decides, ten times the float32 oracle's 2.4e-4; PG_UP2_SPLITK=0 gives the old draw back.)
    # The multiple was 6 until the row-edge tiles changed which layers split K (a third draw of the same roundings): `texture_b512.spade_b512.spade1.conv_gamma.weight`
    # then sat at 5.1e-3 = 6.9x its float32-oracle distance of 7.4e-4 -- with the fp32 MFMA weight gradient and with both bf16x3 forms alike (to seven digits: the
    # weight-gradient kernel is not where it comes from), and inside the bar again with PG_UP2_SPLITK=0.  These tensors are sums over 262 144 pixels that cancel to
    # a thousandth of their absolute sum; a 1e-6 change of an 8^2 activation moves them by more than the float32 oracle's own error.  Hence 10x, and the 3e-2 cap.
    # A transposed, permuted or sign-flipped tensor misses by ~1.
    ew32, ew32_name, ew_n = _elementwise_gradient_mismatch(full['got'], full['want'])
    ref64 = ref_net.double()
    f64 = lambda t: t.double() if t.is_floating_point() else t
    signature(ref64, f64, 'want64')
    ref_net.float()
    worst_gpu, worst_cpu, bad = (0.0, ''), (0.0, ''), []
    for k, w64 in full['want64'].items():
        if w64 is None or w64.numel() <= 1 or k.endswith('noise_strength'):
            continue
        scale = float(w64.abs().max())
        if scale == 0.0:
            continue
        e_gpu = float((full['got'][k].double() - w64).abs().max()) / scale
        e_cpu = float((full['want'][k].double() - w64).abs().max()) / scale
        worst_gpu, worst_cpu = max(worst_gpu, (e_gpu, k)), max(worst_cpu, (e_cpu, k))
        if e_gpu > max(3e-3, 10.0 * e_cpu) or e_gpu > 3e-2:
            bad.append((k, e_gpu, e_cpu))
    print(f'config 4 generator training route, element-wise over {ew_n} gradient tensors (of the tensor maximum): GPU vs float32 oracle worst {ew32:.2e} ({ew32_name}); '
          f'against the float64 oracle: GPU worst {worst_gpu[0]:.2e} ({worst_gpu[1]}), float32 oracle worst {worst_cpu[0]:.2e} ({worst_cpu[1]})')
    assert not bad and ew_n > 100, bad[:6]
    numel = {n_: p_.numel() for n_, p_ in ref_net.named_parameters()}
    worst, n_grad, bad = (0.0, ''), 0, []
    for k in want:
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is None:
            continue
        n_grad += 1
        rel = abs(got[k] - want[k]) / (abs(want[k]) + 1e-9)
        # a one-element parameter (noise_strength) has ONE gradient value, a signed sum of dy * noise over every pixel and channel of its
        # layer (8.4e6 terms at 256^2): the cancellation amplifies float32 rounding ~3000x (measured 1.6 % / 6 % at 16^2 / 256^2), so it only
        # has to agree in sign and order of magnitude; dy itself is pinned by the layer's bias gradient (a per-channel sum of the same dy)
        if numel[k] == 1:
            if not (0.5 <= got[k] / (want[k] + 1e-30) <= 2.0):
                bad.append((k, got[k], want[k]))
            continue
        worst = max(worst, (rel, k))
        if abs(got[k] - want[k]) > 2e-3 * abs(want[k]) + 1e-5:
            bad.append((k, got[k], want[k]))
    print(f'config 4 generator training route, full width, N=1: {n_grad} parameters with gradients, worst signature mismatch {worst[0]:.2e} ({worst[1]})')
    assert not bad, bad
    assert n_grad > 100


def test_config4_layer_gradients_replayed_in_float64(monkeypatch):
    """The WELL-CONDITIONED gradient check.  test_config4_generator_gradients_full_width_vs_oracle compares whole-network gradients with an oracle
    whose forward pass rounds differently, so tensors that are sums over 262 144 pixels cancelling to a thousandth of their absolute sum needed a bar that follows
    the float32 oracle's own error (even ONE SPADE res-block replayed in float64 from the GPU's inputs is off by 5e-3 on `conv.weight`: the instance norms inside
    it).  Here the gradient KERNELS are taken one call at a time, inside the full-width training-route backward on the GPU (N = 1, the same functional): every
    call of the native weight gradient (conv2d_mfma.weight_gradient: fp32-MFMA kernel and the bf16x3 route, stride 1 / 2 / the transposed layers' swapped roles,
    3x3 / 1x1 / the 7x7 stem) and of the native input gradient (conv2d_gradfix._input_gradient: the forward kernels -- F(4x4), F(2x2), direct -- on flipped /
    transposed packs) is recorded with the ACTUAL x, dy and weight it was handed, at full size; each distinct geometry's first call is then recomputed in FLOAT64
    on the CPU from those same tensors -- no forward-rounding draw in between, nothing else of the network takes part -- and the GPU result must match element-wise:
    weight gradients <= 4e-6 of the tensor's largest element on the bf16x3 route and <= 1e-5 on the fp32 kernel (measured: <= 1.1e-6 over 32 geometries); input
    gradients <= 4e-5 (measured: <= 1.2e-5 over 18 geometries -- F(4x4) rounds ~4x coarser than a direct convolution).  The geometries include those of `spade_b256_2.conv0.weight` (128 -> 128 at 256^2), `texture_b512.spade_b512.spade1.
    conv_gamma.weight` (64 -> 64 at 512^2) -- the two tensors that set the network-level 10x bar --, the b512 layers, the up = 2 layers and the 7x7 stem.
    With this test in place the network-level bar is frozen."""
    from training import networks as PN
    from torch_utils.ops import conv2d_mfma, conv2d_gradfix
    from oracle import network_ref as NR
    kw = dict(w_dim=512, img_resolution=512, img_channels=3, channel_base=32768, channel_max=512, conv_clamp=256)
    ref_net = fill_module_(NR.SynthesisNetworkFull_v18(**kw), 'cfg2.')
    net = PN.SynthesisNetworkFull_v18(**kw)
    net.load_state_dict(ref_net.state_dict(), strict=False)
    del ref_net
    net = net.to(DEV).train()
    inp = synthesis_inputs(1, labels=True)
    proj = [det_tensor(f'c4g.proj{i}', shp) for i, shp in enumerate(([1, 3, 512, 512], [1, 3, 512, 512], [1, 7, 512, 512]))]
    wrec, xrec, wcalls, xcalls = {}, {}, [0], [0]
    real_w, real_x = conv2d_mfma.weight_gradient, conv2d_gradfix._input_gradient

    def rec_w(x, dy, weight_shape, pad, stride=1):
        dw = real_w(x, dy, weight_shape, pad, stride=stride)
        wcalls[0] += 1
        key = (tuple(int(v) for v in weight_shape), tuple(x.shape), tuple(dy.shape), int(stride), tuple(int(v) for v in pad))
        if dw is not None and key not in wrec:
            route = 'bf16x3' if conv2d_mfma._bf16x3_wanted(int(x.shape[0]), int(weight_shape[1]), int(weight_shape[0]), int(x.shape[2]), int(x.shape[3]), int(weight_shape[2]), int(weight_shape[3]), int(stride)) else 'fp32'
            wrec[key] = (x.detach().cpu().clone(), dy.detach().cpu().clone(), dw.detach().cpu().clone(), route)
        return dw

    def rec_x(dy, x_shape, weight, stride, padding, transposed, output_padding, fn=None, mod=None):
        dx = real_x(dy, x_shape, weight, stride, padding, transposed, output_padding, fn=fn, mod=mod)
        xcalls[0] += 1
        key = (tuple(weight.shape), tuple(dy.shape), tuple(x_shape), int(stride), tuple(padding), bool(transposed))
        if dx is not None and fn is None and key not in xrec:
            xrec[key] = (dy.detach().cpu().clone(), weight.detach().cpu().clone(), dx.detach().cpu().clone(), tuple(output_padding))
        return dx
    monkeypatch.setattr(conv2d_mfma, 'weight_gradient', rec_w)
    monkeypatch.setattr(conv2d_gradfix, '_input_gradient', rec_x)
    f = lambda t: t.to(DEV)
    out = net(f(inp['ws']), f(inp['pose_feat']), {k: f(v) for k, v in inp['cat_feat'].items()}, f(inp['denorm_upper_input']), f(inp['denorm_lower_input']),
              f(inp['denorm_upper_mask']), f(inp['denorm_lower_mask']), f(inp['gt_parsing']), noise_mode='const')
    sum((o * f(r)).sum() for o, r in zip(out, proj)).backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    del net, out
    torch.set_num_threads(min(32, len(__import__('os').sched_getaffinity(0))))
    report, bad = [], []
    for key, (x, dy, dw, route) in wrec.items():
        wshape, _, _, stride, pad = key
        want = torch.nn.grad.conv2d_weight(x.double(), wshape, dy.double(), stride=stride, padding=pad)
        sc = float(want.abs().max())
        e = float((dw.double() - want).abs().max()) / sc
        limit = 4e-6 if route == 'bf16x3' else 1e-5
        report.append((e / limit, f'dw {route} w{list(wshape)} x{list(x.shape)} s{stride}', e, limit))
        if e > limit:
            bad.append(report[-1])
    for key, (dy, weight, dx, opad) in xrec.items():
        wshape, _, xshape, stride, pad, transposed = key
        if transposed:          # forward was conv_transpose2d(x, w): dx = conv2d(dy, w, stride)
            want = torch.nn.functional.conv2d(dy.double(), weight.double(), stride=stride, padding=pad)
        else:
            want = torch.nn.grad.conv2d_input(xshape, weight.double(), dy.double(), stride=stride, padding=pad)
        sc = float(want.abs().max())
        e = float((dx.double() - want).abs().max()) / sc
        report.append((e / 4e-5, f'dx w{list(wshape)} dy{list(dy.shape)} s{stride}{" transposed" if transposed else ""}', e, 4e-5))
        if e > 4e-5:
            bad.append(report[-1])
    report.sort(reverse=True)
    print(f'gradient kernels replayed in float64 from the GPU\'s own operands: {len(wrec)} weight-gradient geometries of {wcalls[0]} calls, {len(xrec)} input-gradient geometries of {xcalls[0]} calls; '
          'closest to their bars: ' + '; '.join(f'{k} {e:.1e} (bar {lim:.0e})' for _, k, e, lim in report[:10]))
    assert not bad, bad
    shapes = {k[0] for k in wrec}
    assert (128, 128, 3, 3) in shapes and (64, 64, 3, 3) in shapes and any(s_[2:] == (7, 7) for s_ in shapes), shapes
    assert any(r == 'bf16x3' for *_, r in wrec.values()) and any(r == 'fp32' for *_, r in wrec.values())
    assert len(wrec) >= 12 and len(xrec) >= 6, (len(wrec), len(xrec))


@pytest.mark.parametrize('res,base,cmax', [(16, 256, 32), (64, 1024, 64)])
def test_discriminator_fp16_gradients_are_reproducible(res, base, cmax):
    """Two identical passes through a discriminator with a half-precision block must give bit-identical gradients, first order and through R1's double backward
    (loss_fullbody.py:247-256).  Until round 5 the weight gradient of the INPUT-GRADIENT node of the fp16 down-sampling convolution -- a transposed convolution --
    went to aten (MIOpen), whose stride-2 16-bit weight gradient is not run-to-run reproducible: `bNN.conv1.weight` differed between runs under R1
    (tools/probes/d_fp16_determinism.py); conv2d_gradfix now runs it on the native kernel with the roles of x and dy swapped."""
    from training import networks as PN
    torch.manual_seed(0)
    kw = dict(c_dim=6, img_resolution=res, img_channels=6, channel_base=base, channel_max=cmax, conv_clamp=256, mapping_kwargs=dict(num_layers=1),
              epilogue_kwargs=dict(mbstd_group_size=2))
    d = PN.Discriminator(**kw, num_fp16_res=1).to(DEV).train()
    x, c = torch.randn(4, 6, res, res, device=DEV), torch.randn(4, 6, device=DEV)

    def first_order():
        for p in d.parameters():
            p.grad = None
        d(x, c).sum().backward()
        return {n: p.grad.detach().clone() for n, p in d.named_parameters() if p.grad is not None}

    def r1():
        for p in d.parameters():
            p.grad = None
        xr = x.detach().requires_grad_(True)
        gx, = torch.autograd.grad(d(xr, c).sum(), xr, create_graph=True)
        (gx.square().sum([1, 2, 3]).mean() * 5).backward()
        return {n: p.grad.detach().clone() for n, p in d.named_parameters() if p.grad is not None}
    for fn in (first_order, r1):
        a, b = fn(), fn()
        assert a.keys() == b.keys() and len(a) > 10
        bad = [n for n in a if not torch.equal(a[n], b[n])]
        assert not bad, (fn.__name__, bad)


@pytest.mark.parametrize('flat_adam', ['1', '0'], ids=['flat_adam', 'torch_adam'])
@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graphed'])
def test_training_step_gain_fold_equals_multiplies(graphs, flat_adam, monkeypatch):
    """PG_GAIN_FOLD (round 5): the pre-scaled weight copies + gains applied in the bucket's gather must leave the same weights and Adam statistics as the
    per-call `weight * weight_gain` multiplies they replace -- product discriminators (equalised-LR convolutions, R1 double backward), stub generator, 5 iterations;
    one discriminator weight is edited IN PLACE after the step object exists (a checkpoint load would do that): its copy is stale when the first phase runs and must
    be refreshed on the spot, not bypassed (the gather multiplies that gradient by the gain either way).  float32 discriminators: two runs of the SAME setting differ
    by 2.4e-7 here and the two settings by 4.8e-7 (tools/probes/gain_fold_noise.py); with a half-precision block two runs of the same setting already differ by
    3.7e-4 after five Adam steps, which would hide anything this test looks for."""
    import stubs
    from training import networks as PN
    from training.loss import StyleGAN2Loss
    from training.training_step import TrainingStep
    from oracle import network_ref as NR

    # flat_adam = '0' (ADVICE r5): torch.optim.Adam on gather-mode buckets -- the second D_parsing entry of the phase table then has a bucket of its own, which must
    # carry the gains too (its phases run on the pre-scaled aliases like every other phase)
    monkeypatch.setenv('PG_FLAT_ADAM', flat_adam)

    def run(fold):
        monkeypatch.setenv('PG_GAIN_FOLD', '1' if fold else '0')
        torch.manual_seed(0)
        nets = stubs.build(DEV)
        for name, ch in (('D', 6), ('D_parsing', 10)):
            ref = fill_module_(NR.Discriminator(**_d_kw(ch)), f'gf.{name}.')
            d = PN.Discriminator(**_d_kw(ch))
            d.load_state_dict(ref.state_dict(), strict=False)
            nets[name] = d.to(DEV).train()
        loss = StyleGAN2Loss(device=torch.device(DEV), **nets, style_mixing_prob=0, r1_gamma=10, l1_weight=50, mask_weight=1.0)
        G_parts = {k: v for k, v in nets.items() if k.startswith('G_')}
        step = TrainingStep(G_parts, nets['D'], nets['D_parsing'], loss, batch_size=4, graphs=graphs)
        assert bool(step._gained) == fold
        if fold:
            for b in {id(ph.bucket): ph.bucket for ph in step.phases}.values():
                assert b.grad_gains is not None or not any(isinstance(m, PN._ConvBase) for ph in step.phases if ph.bucket is b for top in ph.modules for m in top.modules())
        with torch.no_grad():
            nets['D'].b8.conv0.weight.mul_(1.25)              # after the copies were made
        b = stubs.batch(4, DEV)
        for _ in range(5):
            step.run([b])
        torch.cuda.synchronize()
        return {f'{k}.{n}': p.detach().clone() for k, m in nets.items() for n, p in m.named_parameters()}

    plain, folded = run(False), run(True)
    assert plain.keys() == folded.keys()
    moved = 0
    for k in plain:
        assert torch.allclose(folded[k], plain[k], rtol=1e-5, atol=2e-6), (k, float((folded[k] - plain[k]).abs().max()))
        moved += int(not torch.equal(folded[k], plain[k]))
    assert PN._gained_provider[0] is None                     # armed only while a phase runs


def test_training_step_graph_replay_equals_eager():
    """TrainingStep(graphs=True): every phase captured into a hipGraph the second time it is due and replayed afterwards must leave the
    same weights, Adam statistics and EMA as the eager step (the replay runs the very kernels the eager phase launches; packed-weight
    caches are invalidated around captures and replays).  Product discriminators (HIP ops, R1 double backward) + stub generator, 6
    iterations: eager first run, capture, four replays of the every-iteration phases; the lazy-regularisation phases stay eager here."""
    import stubs
    from training import networks as PN
    from training.loss import StyleGAN2Loss
    from training.training_step import TrainingStep
    from oracle import network_ref as NR

    def run(graphs):
        torch.manual_seed(0)
        nets = stubs.build(DEV)
        for name, ch in (('D', 6), ('D_parsing', 10)):
            ref = fill_module_(NR.Discriminator(**_d_kw(ch)), f'tg.{name}.')
            d = PN.Discriminator(**_d_kw(ch))
            d.load_state_dict(ref.state_dict(), strict=False)
            nets[name] = d.to(DEV).train()
        loss = StyleGAN2Loss(device=torch.device(DEV), **nets, style_mixing_prob=0, r1_gamma=10, l1_weight=50, mask_weight=1.0)
        G_parts = {k: v for k, v in nets.items() if k.startswith('G_')}
        step = TrainingStep(G_parts, nets['D'], nets['D_parsing'], loss, batch_size=4, graphs=graphs)
        b = stubs.batch(4, DEV)
        for _ in range(6):
            step.run([b])
        torch.cuda.synchronize()
        return step, {f'{k}.{n}': p.detach().clone() for k, m in nets.items() for n, p in m.named_parameters()}

    eager_step, eager = run(False)
    graph_step, graphed = run(True)
    assert set(graph_step.graphed_phases()) >= {'Gmain', 'Dmain', 'D_parsingmain'}, graph_step.graphed_phases()
    assert eager.keys() == graphed.keys()
    for k in eager:
        assert torch.allclose(graphed[k], eager[k], rtol=1e-4, atol=1e-6), (k, float((graphed[k] - eager[k]).abs().max()))
    for a, b in zip(eager_step.G_ema_parts['G_synthesis'].parameters(), graph_step.G_ema_parts['G_synthesis'].parameters()):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('d_fp16_res', [0, 3])
def test_full_width_training_iteration_smoke(d_fp16_res):
    """One iteration of the 8-phase schedule (all phases due) with the full-width generator and both discriminators at
    N=2 on one GPU: finite gradients, every module updated, EMA tracking; exercises GradBucket's single-rank path.
    d_fp16_res = 3 is the reference's training configuration (train.py:196: the discriminators' 3 highest resolutions in fp16,
    i.e. forward, input gradients and the R1 double backward of those blocks on the 16-bit MFMA kernel)."""
    import time
    from training import networks as PN
    from training.loss import StyleGAN2Loss
    from training.training_step import TrainingStep
    torch.manual_seed(0)
    G = PN.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                             synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256)).to(DEV).train()
    dkw = dict(c_dim=512, img_resolution=512, channel_base=32768, channel_max=512, conv_clamp=256, epilogue_kwargs=dict(mbstd_group_size=2),
               num_fp16_res=d_fp16_res)
    D, DP = PN.Discriminator(img_channels=6, **dkw).to(DEV).train(), PN.Discriminator(img_channels=10, **dkw).to(DEV).train()
    with torch.no_grad():
        for m in (G, D, DP):
            for name, p in m.named_parameters():
                if name.endswith('noise_strength'):
                    p.fill_(0.1)
    parts = dict(G_mapping=G.mapping, G_synthesis=G.synthesis, G_const_encoding=G.const_encoding, G_style_encoding=G.style_encoding)
    loss = StyleGAN2Loss(device=torch.device(DEV), **parts, D=D, D_parsing=DP, style_mixing_prob=0.9, r1_gamma=10, l1_weight=50, mask_weight=1.0)
    step = TrainingStep(parts, D, DP, loss, batch_size=2)
    n = 2
    gen = torch.Generator(device='cpu').manual_seed(1)
    u = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).to(DEV)
    batch = dict(real_img=u(n, 3, 512, 512), gen_z=torch.zeros([n, 0], device=DEV), style_input=u(n, 45, 128, 128), retain=u(n, 6, 512, 512),
                 pose=u(n, 5, 512, 512), denorm_upper_input=u(n, 3, 512, 512), denorm_lower_input=u(n, 3, 512, 512),
                 denorm_upper_mask=(u(n, 1, 512, 512) > 0).float(), denorm_lower_mask=(u(n, 1, 512, 512) > 0).float(),
                 gt_parsing=torch.randint(0, 7, [n, 1, 512, 512], generator=gen).float().to(DEV))
    before = [p.detach().clone() for p in list(G.synthesis.parameters())[:8]] + [p.detach().clone() for p in list(D.parameters())[:4]]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step.run([batch])
    torch.cuda.synchronize()
    print(f'full-width training iteration (all 8 phases, N={n}): {time.perf_counter() - t0:.2f} s')
    after = list(G.synthesis.parameters())[:8] + list(D.parameters())[:4]
    assert all(torch.isfinite(p).all() for m in (G, D, DP) for p in m.parameters())
    assert sum(int(not torch.equal(a, b)) for a, b in zip(before, after)) >= 8
    assert step.batch_idx == 1


@pytest.mark.parametrize('d_fp16_res', [0, 3], ids=['d_fp32', 'd_fp16_top3'])
def test_config4_whole_iteration_batch4_vs_oracle(d_fp16_res):
    """BASELINE config 4's per-rank share as ONE piece: the full-width generator and both discriminators at 512^2,
    per-rank batch 4 (train.py:174), all eight phases of one `TrainingStep.run` on the GPU (training_loop_fullbody.py:468-481, 604-639) --
    and the per-parameter gradient signatures of its `Gmain` and `Dmain` phases, taken when the phase's gradients are final and before its
    optimizer steps, against the CPU oracle networks run through the same loss FROM THE WEIGHTS THE PRODUCT HAD AT THE START OF THAT PHASE
    (Dmain follows Gmain's Adam step: the oracle is handed the stepped generator, so that each comparison isolates one phase's forward +
    backward).  Two settings: fp32 discriminators on both sides, and -- round 5, the BENCHED setting -- both discriminators fp16 at their three top resolutions
    (train.py:196) at a 16-bit bar; besides the signatures every gradient TENSOR of the phase's network is compared element-wise (max|diff| of its largest element);
    noise_strength = 0 (the training route draws fresh noise per call, which two devices cannot share); no style mixing.  Bar: per-parameter
    sum|grad| within 3e-3 (the bar of the per-network tests this one joins); single-element parameters only in sign and magnitude."""
    import os
    import time
    from training import networks as PN
    from training.loss import StyleGAN2Loss
    from training.training_step import TrainingStep
    from oracle import network_ref as NR
    n = 4
    g_kw = dict(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256))
    d_kw = lambda ch: dict(c_dim=512, img_resolution=512, img_channels=ch, channel_base=32768, channel_max=512, conv_clamp=256, num_fp16_res=d_fp16_res,
                           epilogue_kwargs=dict(mbstd_group_size=4))
    ref = dict(G=fill_module_(NR.GeneratorFull_v20(**g_kw), 'c4w.G.', noise_strength=0.0).train(),
               D=fill_module_(NR.Discriminator(**d_kw(6)), 'c4w.D.').train(), D_parsing=fill_module_(NR.Discriminator(**d_kw(10)), 'c4w.DP.').train())
    if d_fp16_res:
        # With these synthetic weights the logits are ~6e-4 and the loss gradient reaching the 512^2 ... 128^2 blocks is ~1e-9 per element: below fp16's
        # smallest subnormal, so the real fp16 backward (this package's, and the reference's cuDNN one) yields exact zeros there, while the CPU oracle's
        # half-precision emulation does not underflow.  Output layers scaled by 2048 on both sides put the logits at O(1) and the gradients inside fp16's range.
        with torch.no_grad():
            for k in ('D', 'D_parsing'):
                ref[k].b4.out.weight.mul_(2048.0); ref[k].b4.out.bias.mul_(2048.0)
    net = dict(G=PN.GeneratorFull_v20(**g_kw), D=PN.Discriminator(**d_kw(6)), D_parsing=PN.Discriminator(**d_kw(10)))
    for k in net:
        missing, unexpected = net[k].load_state_dict(ref[k].state_dict(), strict=False)
        assert not unexpected and not [m for m in missing if 'resample_filter' not in m], (k, missing, unexpected)
        net[k] = net[k].to(DEV).train()
    parts = lambda g: dict(G_mapping=g.mapping, G_synthesis=g.synthesis, G_const_encoding=g.const_encoding, G_style_encoding=g.style_encoding)
    mk_loss = lambda nets, device: StyleGAN2Loss(device=torch.device(device), **parts(nets['G']), D=nets['D'], D_parsing=nets['D_parsing'],
                                                 style_mixing_prob=0, r1_gamma=10, l1_weight=50, mask_weight=1.0)
    u = lambda name, *shape: det_tensor('c4w.' + name, shape, 'uniform')
    batch = dict(real_img=u('real', n, 3, 512, 512), gen_z=torch.zeros([n, 0]), style_input=u('style', n, 45, 128, 128), retain=u('retain', n, 6, 512, 512),
                 pose=u('pose', n, 5, 512, 512), denorm_upper_input=u('du', n, 3, 512, 512), denorm_lower_input=u('dl', n, 3, 512, 512),
                 denorm_upper_mask=det_tensor('c4w.mu', [n, 1, 512, 512], 'blockmask'), denorm_lower_mask=det_tensor('c4w.ml', [n, 1, 512, 512], 'blockmask'),
                 gt_parsing=det_tensor('c4w.gt', [n, 1, 512, 512], 'labels7'))
    sig_of = lambda nets: {f'{k}.{pn}': (None if p_.grad is None else float(p_.grad.double().abs().sum())) for k, m in nets.items() for pn, p_ in m.named_parameters()}

    want_phases = ('Gmain', 'Dmain')
    # Gmain runs with noise_strength = 0 (initial value): nothing random, 3e-3 as in the per-network tests.  By Dmain the Adam step has moved every
    # noise_strength to +-4e-4 and the generator draws its noise afresh on each side (GPU generator here, CPU generator in the oracle): with nothing but the
    # torch seed changed the Dmain signatures move by up to 2.3e-3 (tools/probes/dmain_noise_sensitivity.py, three seeds), so that phase gets 3e-3 on top of it.
    bar = dict(Gmain=3e-3, Dmain=6e-3)
    # element-wise: of the tensor's largest element.  Dmain: the generator's fresh noise draws differ between the two devices (see `bar`); measured 5.2e-2 on the
    # smallest tensors (b4.conv.weight, max 2.8e-6) at cosine 0.9999-1.0000
    ew_bar = dict(Gmain=4e-3, Dmain=1e-1)
    if d_fp16_res:
        # the benched setting (train.py:196: the three top resolutions of both discriminators in fp16): the discriminator's own gradients and its input
        # gradient into the generator carry 16-bit rounding (2^-11 per layer, ~20 layers) on both sides, in different summation orders
        bar = dict(Gmain=2e-2, Dmain=2e-2)
        ew_bar = dict(Gmain=4e-2, Dmain=2e-1)
    torch.manual_seed(1234)          # the draws must not depend on which tests ran before this one
    start, got, got_full, order = {}, {}, {}, []

    def observer(event, ph):
        order.append((event, ph.name))
        if ph.name not in want_phases:
            return
        if event == 'begin':
            start[ph.name] = {k: {a: b.detach().cpu().clone() for a, b in m.state_dict().items()} for k, m in net.items()}
        else:
            got[ph.name] = sig_of(net)
            own = 'G' if ph.name.startswith('G') else 'D'
            got_full[ph.name] = {f'{own}.{pn}': (None if p_.grad is None else p_.grad.detach().cpu().clone()) for pn, p_ in net[own].named_parameters()}

    step = TrainingStep(parts(net['G']), net['D'], net['D_parsing'], mk_loss(net, DEV), batch_size=n)
    step.observer = observer
    before = {k: [p_.detach().clone() for p_ in m.parameters()] for k, m in net.items()}
    t0 = time.perf_counter()
    step.run([{k: v.to(DEV) for k, v in batch.items()}])
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    # the whole 8-phase schedule ran (Greg is statically empty: no backward, no step -- loss.phase_is_empty), every network moved, all finite
    assert [nm for ev, nm in order if ev == 'gradients'] == ['Gmain', 'Dmain', 'Dreg', 'D_parsingmain', 'D_parsingreg', 'D_parsingmain', 'D_parsingreg'], order
    for k, m in net.items():
        assert all(torch.isfinite(p_).all() for p_ in m.parameters()), k
        still = [pn for (pn, p_), a in zip(m.named_parameters(), before[k]) if torch.equal(a, p_)]
        if d_fp16_res and k != 'G':
            # with these synthetic weights the discriminators' loss gradients are ~1e-6 (fp32 run: max |dW| of b4.conv 2.8e-6) and underflow to ZERO inside the
            # fp16 blocks -- on the GPU and in the oracle alike (tools/probes/which_params_moved.py) -- so the three fp16 blocks cannot move; everything else must
            still = [pn for pn in still if not pn.startswith(('b512.', 'b256.', 'b128.'))]
        assert len(still) <= 0.1 * len(before[k]) + 2, (k, still)

    torch.set_num_threads(min(64, len(os.sched_getaffinity(0))))      # (the oracle generator's forward + backward at N = 4 is ~3 TFLOP of CPU work)
    ref_loss = mk_loss(ref, 'cpu')
    report = []
    for phase in want_phases:
        t0 = time.perf_counter()
        for k, m in ref.items():
            m.load_state_dict(start[phase][k], strict=False)
            for p_ in m.parameters():
                p_.grad = None
            m.requires_grad_(k == ('G' if phase.startswith('G') else 'D'))
        ref_loss.accumulate_gradients(phase=phase, gain=1, **batch)
        want = sig_of(ref)
        assert want.keys() == got[phase].keys()
        numel = {f'{k}.{pn}': p_.numel() for k, m in ref.items() for pn, p_ in m.named_parameters()}
        worst, n_grad, bad = (0.0, ''), 0, []
        owner = 'G.' if phase.startswith('G') else 'D.'
        for key, w in want.items():
            if not key.startswith(owner):
                continue                 # only the phase's own networks: the other buckets still hold the gradients of THEIR last phase (views into flat buckets)
            g = got[phase][key]
            if w is None or w == 0.0:
                assert g is None or g == 0.0 or (d_fp16_res and g <= 1e-12), (phase, key, g)     # e.g. synthesis.b8.const (networks.py:2118 vs :2157-2161) never receives a gradient
                continue
            assert g is not None, (phase, key)
            if key.endswith('noise_strength'):
                continue                 # d/d(noise_strength) = sum(dy * noise): the training route draws the noise afresh on each device
            n_grad += 1
            if numel[key] == 1:          # a signed sum over every pixel of a layer: sign and magnitude only (see test_config4_generator_gradients_full_width_vs_oracle)
                if not 0.5 <= g / (w + 1e-30) <= 2.0:
                    bad.append((key, g, w))
                continue
            worst = max(worst, (abs(g - w) / (abs(w) + 1e-12), key))
            if abs(g - w) > bar[phase] * abs(w) + 1e-6:
                bad.append((key, g, w))
        own = owner[:-1]
        want_full = {f'{own}.{pn}': (None if (p_.grad is None or float(p_.grad.abs().max()) == 0.0) else p_.grad.detach().clone()) for pn, p_ in ref[own].named_parameters()}
        ew_stats = {}
        ew, ew_name, ew_n = _elementwise_gradient_mismatch(got_full[phase], want_full, stats=ew_stats)
        report.append(f'{phase}: {n_grad} parameters with gradients, worst signature mismatch {worst[0]:.2e} ({worst[1]}), element-wise over {ew_n} tensors worst '
                      f'{ew:.2e} of the tensor maximum ({ew_name}), oracle {time.perf_counter() - t0:.0f} s')
        if phase == 'Dmain':
            # the half-precision blocks must not be compared vacuously -- their tensors have to be non-zero on BOTH sides and go through the element-wise check
            top3 = ('D.b512.', 'D.b256.', 'D.b128.')
            cmp3 = [k for k in ew_stats.get('compared', []) if k.startswith(top3)]
            skip3 = [k for k in ew_stats.get('skipped', []) if k.startswith(top3)]
            none3 = [k for k, w_ in want_full.items() if k.startswith(top3) and w_ is None]
            report.append(f'{phase} top-three blocks: {len(cmp3)} tensors compared element-wise, {len(skip3)} below 1e-6 of the largest gradient (skipped: {skip3}), {len(none3)} zero in the oracle')
            print(report[-1])
            if d_fp16_res:
                assert len(cmp3) >= 12, (cmp3, skip3, none3)
        assert not bad, (phase, bad[:8])
        assert ew <= ew_bar[phase], (phase, ew, ew_name)
        assert n_grad >= (150 if phase == 'Gmain' else 20), (phase, n_grad)
    print(f'config 4 whole iteration at batch {n}, discriminators fp16 at {d_fp16_res} resolutions (GPU {t_gpu:.2f} s incl. first-call work): ' + '; '.join(report))


@pytest.mark.timeout(900)
def test_bench_as_single_rank_under_torch_distributed_run():
    """The launch the driver uses for N > 1, at N = 1 on the hardware that is there: `torch.distributed.run --nproc-per-node 1`
    sets RANK / WORLD_SIZE, so bench.py is a rank -- `init_process_group('nccl')` (RCCL), the barrier on both sides of the timed region and
    `replicas.max_over_ranks` (an all-reduce MAX on the device) all execute.  One JSON line, n_gpus 1, a finite positive value."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.empty_cache()
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1', '--master-port', '29671',
                        os.path.join(root, 'bench.py'), '--gpus', '1', '--no-cpu-baseline', '--no-secondary', '--steps', '2', '--warmup', '1'],
                       capture_output=True, text=True, timeout=800, env=env)
    assert r.returncode == 0, (r.stderr or r.stdout)[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    j = lines[0]
    assert j['n_gpus'] == 1 and j['steps'] == 2 and j['value'] > 0 and j['config']['parallelism'] == 'replicas x1' and 'roofline' in j


# =============================================================== round-2 parity holes

def test_synthesis_full_width_batch8_vs_oracle():
    """BASELINE config 2 at its REAL batch (N=8, one launch sequence) against the CPU oracle run image by image on three of
    the eight images (first, an odd middle one, last): the tile -> image index maths of the persistent, XCD-remapped conv
    kernels is what an N-dependent bug would break."""
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(w_dim=512, img_resolution=512, img_channels=3, channel_base=32768, channel_max=512, conv_clamp=256)
    ref_net = fill_module_(NR.SynthesisNetworkFull_v18(**kw), 'cfg2.').eval()
    net = _load(PN.SynthesisNetworkFull_v18(**kw), ref_net)
    n = 8
    inp = synthesis_inputs(n, labels=True)
    args = lambda f: (f(inp['ws']), f(inp['pose_feat']), {k: f(v) for k, v in inp['cat_feat'].items()}, f(inp['denorm_upper_input']),
                      f(inp['denorm_lower_input']), f(inp['denorm_upper_mask']), f(inp['denorm_lower_mask']), f(inp['gt_parsing']))
    with torch.no_grad():
        out = [o.cpu() for o in net(*args(lambda t: t.to(DEV)), noise_mode='const')]
        for i in (0, 3, 7):
            ref = ref_net(*args(lambda t: t[i:i + 1]), noise_mode='const')
            for nm, a, b in zip(('img', 'finetune_img', 'pred_parsing'), out, ref):
                _pixel_bar(nm, a[i:i + 1], b, f'image {i} ')


def test_bench_workload_argmax_path_batch8_vs_oracle():
    """The EXACT workload bench.py times (its make_inputs / run_net: gt_parsing=None, i.e. the argmax parsing path of test.py) at
    N=8 against the CPU oracle on images 0, 3 and 7.  `img` and `pred_parsing` are upstream of the argmax and must meet the bar
    outright; `finetune_img` is downstream of it -- a near-tie in the parsing logits may legitimately flip a label -- so it is
    compared where both sides took the same labels: everywhere if the label maps agree (expected), otherwise the disagreeing
    fraction must be tiny and the comparison is skipped for that image with a message."""
    import bench
    from training import networks as PN
    from oracle import network_ref as NR
    bench.torch = torch
    ref_net = bench.init_weights(NR.SynthesisNetworkFull_v18(**bench.CFG2)).eval()
    net = _load(PN.SynthesisNetworkFull_v18(**bench.CFG2), ref_net)
    dev_inp, cpu_inp = bench.make_inputs(8, DEV, seed=0), bench.make_inputs(8, 'cpu', seed=0)
    take = lambda d, i: {k: ({kk: vv[i:i + 1] for kk, vv in v.items()} if isinstance(v, dict) else v[i:i + 1]) for k, v in d.items()}
    with torch.no_grad():
        out = [o.cpu() for o in bench.run_net(net, dev_inp)]
        for i in (0, 3, 7):
            ref = bench.run_net(ref_net, take(cpu_inp, i))
            d_img = _pixel_bar('img', out[0][i:i + 1], ref[0], f'image {i} ')
            d_pp = _pixel_bar('pred_parsing', out[2][i:i + 1], ref[2], f'image {i} ')
            flips = float((out[2][i:i + 1].argmax(dim=1) != ref[2].argmax(dim=1)).float().mean())
            if flips == 0:
                d_fi = _pixel_bar('finetune_img', out[1][i:i + 1], ref[1], f'image {i} ')
                print(f'bench workload image {i}: img {d_img:.2e}, pred_parsing {d_pp:.2e}, finetune_img {d_fi:.2e} (labels identical)')
            else:
                assert flips < 1e-4, f'image {i}: {flips:.2e} of the argmax labels differ'
                print(f'bench workload image {i}: img {d_img:.2e}, pred_parsing {d_pp:.2e}; {flips:.2e} of the labels flipped on near-ties, finetune_img not compared')


def test_bench_workload_repeats_bit_identical():
    """Every kernel on the config-2 path is deterministic (no atomics, fixed reduction orders), so the bench workload at N=8 must
    reproduce its first outputs bit for bit under load; a pass that differs is a race (the F(4x4) tail race of round 3 made 20 % of
    full-size launches wrong while every small test passed).  `tools/step_stress.py` is the long form of this test."""
    import bench
    from training import networks as PN
    bench.torch = torch
    net = bench.init_weights(PN.SynthesisNetworkFull_v18(**bench.CFG2)).to(DEV).eval()
    inp = bench.make_inputs(8, DEV, seed=5)
    other = torch.randn(32, 64, 256, 256, device=DEV)
    with torch.no_grad():
        ref = [t.clone() for t in bench.run_net(net, inp) if torch.is_tensor(t)]
        for it in range(12):
            if it % 3 == 1:
                other.mul_(1.0001)
            out = [t for t in bench.run_net(net, inp) if torch.is_tensor(t)]
            for k, (a, b) in enumerate(zip(ref, out)):
                assert torch.equal(a, b), f'pass {it}, output {k}: max |d| {float((a - b).abs().max()):.3e} against the first pass'


def test_config3_chain_patch_routing_into_generator_n16():
    """BASELINE config 3 end to end on the product: patch routing (HIP warps) -> uint8 tensors normalised as test.py does
    (test.py:126-147) -> GeneratorFull_v20 at N=16.  Checks: finite outputs, and every image of the batch equals the N=1 run
    of the same sample (four distinct samples, each four times in the batch)."""
    from training import networks as PN
    from training import patch_routing as P
    sys_path_ok = True
    from test_patch_routing import keypoints
    rng = np.random.default_rng(3)
    samples = []
    for k in range(4):
        ckp, pkp = keypoints(rng, 8.0), keypoints(rng, 8.0)
        up, lo = (rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) for _ in range(2))
        um = np.zeros((512, 512, 3), np.uint8); um[90:310, 150:370] = 255
        lm = np.zeros((512, 512, 3), np.uint8); lm[270:505, 190:330] = 255
        norm_img, norm_lower, den_up, _, den_lo = P.normalize(up, lo, um, lm, None, ckp, pkp, 2)
        f = lambda t: t.permute(2, 0, 1).float() / 127.5 - 1            # HWC uint8 -> CHW in [-1, 1]
        samples.append(dict(
            c=torch.cat([f(norm_img), f(norm_lower)], dim=0),
            du=f(den_up), dl=f(den_lo),
            mu=(den_up.sum(dim=2, keepdim=True) > 0).permute(2, 0, 1).float(), ml=(den_lo.sum(dim=2, keepdim=True) > 0).permute(2, 0, 1).float(),
            retain=torch.from_numpy(rng.uniform(-1, 1, (6, 512, 512)).astype(np.float32)).to(DEV),
            pose=torch.from_numpy(rng.uniform(-1, 1, (5, 512, 512)).astype(np.float32)).to(DEV)))
        assert samples[-1]['c'].shape == (45, 128, 128) and float(samples[-1]['mu'].sum()) > 0
    kw = dict(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
              synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256))
    net = fill_module_(PN.GeneratorFull_v20(**kw), 'cfg3.').to(DEV).eval()

    def run(idx):
        st = lambda key: torch.stack([samples[i][key] for i in idx]).to(DEV)
        with torch.no_grad():
            return net(torch.zeros([len(idx), 0], device=DEV), st('c'), st('retain'), st('pose'), st('du'), st('dl'), st('mu'), st('ml'), noise_mode='const')
    order = [i % 4 for i in range(16)]
    batch = run(order)
    assert all(o.shape[0] == 16 and torch.isfinite(o).all() for o in batch)
    for k in (0, 3):
        single = run([k])
        for nm, a, b in zip(('img', 'finetune_img', 'pred_parsing'), batch, single):
            s = scale_of(b)
            for pos in (k, k + 12):                                     # first and last occurrence of sample k in the batch
                delta = float((a[pos:pos + 1] - b).abs().max())
                assert delta <= 1e-4 * s, f'sample {k} at batch slot {pos}, {nm}: {delta:.3e} vs range {s:.3e}'


def test_discriminator_fp16_blocks_vs_oracle():
    """Row f2 in half precision: Discriminator(num_fp16_res=3) -- its three highest resolutions in fp16 on the 16-bit MFMA
    convolution (channels-last), conv_clamp 256 as train.py:196-197 sets -- against the float32 CPU oracle.  Tolerance: fp16
    activations carry 2^-11 relative rounding per layer; 3 blocks x 3 convs + the float32 tail -> 2e-2 of the logit scale."""
    from training import networks as PN
    from oracle import network_ref as NR
    kw = dict(c_dim=16, img_resolution=64, img_channels=6, channel_base=1024, channel_max=64, conv_clamp=256,
              mapping_kwargs=dict(num_layers=2), epilogue_kwargs=dict(mbstd_group_size=2))
    ref = fill_module_(NR.Discriminator(**kw), 'dfp16.')
    d = PN.Discriminator(num_fp16_res=3, **kw)
    d.load_state_dict(ref.state_dict(), strict=False)
    d = d.to(DEV).train()
    assert [b.use_fp16 for b in (d.b64, d.b32, d.b16, d.b8)] == [True, True, True, False]
    img = det_tensor('dfp16.img', [4, 6, 64, 64], 'uniform')
    c = det_tensor('dfp16.c', [4, 16])
    want = ref(img, c)
    x = img.to(DEV).requires_grad_(True)
    got = d(x, c.to(DEV))
    assert got.dtype == torch.float32
    tol = 2e-2 * scale_of(want)
    assert float((got.detach().cpu() - want.detach()).abs().max()) <= tol
    # the training-step use: R1 penalty through the fp16 blocks (double backward) stays finite and close to the fp32 one
    gi, = torch.autograd.grad(got.sum(), x, create_graph=True)
    pen = gi.square().sum([1, 2, 3])
    pen.sum().backward()
    xi = img.clone().requires_grad_(True)
    gr, = torch.autograd.grad(ref(xi, c).sum(), xi, create_graph=True)
    pen_ref = gr.square().sum([1, 2, 3])
    assert torch.isfinite(pen).all() and all(p.grad is None or torch.isfinite(p.grad).all() for p in d.parameters())
    assert float((pen.detach().cpu() - pen_ref.detach()).abs().max()) <= 6e-2 * float(pen_ref.abs().max())


def test_modulated_conv2d_fp16_prenorm_golden(golden):
    """The reference's fp16 pre-normalisation path (networks.py:57-59; golden made by the reference in fp16 on the CPU)."""
    from training import networks
    from torch_utils.ops import upfirdn2d
    g = golden('g4_modconv.npz')
    if 'fp16_prenorm/y' not in g:
        pytest.skip('fixture lacks the fp16 case')
    name = 'fp16_prenorm'
    x = det_tensor(name + '.x', [2, 5, 9, 9]).half().to(DEV)
    y = networks.modulated_conv2d(x, det_tensor(name + '.w', [6, 5, 3, 3]).to(DEV), (det_tensor(name + '.s', [2, 5]) + 1.0).to(DEV), padding=1,
                                  resample_filter=upfirdn2d.setup_filter(C.FIR_1331).to(DEV), fused_modconv=False)
    assert y.dtype == torch.float16
    close(y.float(), g[f'{name}/y'], rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize('shape', [(2, 16, 24, 20, 37, 3, 1), (1, 70, 130, 9, 33, 3, 1), (3, 64, 64, 17, 17, 1, 1), (2, 5, 7, 8, 40, 1, 1), (8, 64, 64, 64, 64, 3, 1),
                                   (2, 16, 24, 21, 37, 3, 2), (1, 70, 130, 10, 66, 3, 2), (4, 64, 64, 65, 65, 3, 2),
                                   (2, 3, 64, 40, 44, 7, 1), (1, 2, 70, 9, 33, 7, 1), (4, 3, 64, 128, 128, 7, 1)],
                         ids=['3x3_ragged', '3x3_multi_block', '1x1', '1x1_tiny', '3x3_many_chunks', '3x3s2_ragged', '3x3s2_multi_block', '3x3s2_odd_input',
                              '7x7_stem', '7x7_ragged', '7x7_many_chunks'])
def test_native_weight_gradient_exact(shape, monkeypatch):
    """csrc/conv2d_wgrad.hip (GEMM over pixels, K-split with a fixed-order second pass; stride 1 and 2; the few-channel 7x7 form of the encoders' stem)
    on small-integer data: every partial sum is exact in fp32, so the result must equal the fp64 weight gradient bit for bit.  (PG_WGRAD_BF16X3=0: the fp32 MFMA
    kernel on every shape; the operand-split route has test_weight_gradient_bf16x3.)"""
    from torch_utils.ops import conv2d_mfma
    monkeypatch.setenv('PG_WGRAD_BF16X3', '0')
    n, cin, cout, h, w, k, st = shape
    gen = torch.Generator().manual_seed(n * 1000 + cin + st)
    x = torch.randint(-3, 4, [n, cin, h, w], generator=gen).float()
    oh, ow = (h + 2 * (k // 2) - k) // st + 1, (w + 2 * (k // 2) - k) // st + 1
    dy = torch.randint(-2, 3, [n, cout, oh, ow], generator=gen).float()
    got = conv2d_mfma.weight_gradient(x.to(DEV), dy.to(DEV), [cout, cin, k, k], (k // 2, k // 2), stride=st)
    assert got is not None
    wref = torch.zeros([cout, cin, k, k], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x.double(), wref, padding=k // 2, stride=st).backward(dy.double())
    assert torch.equal(got.double().cpu(), wref.grad), float((got.double().cpu() - wref.grad).abs().max())


@pytest.mark.parametrize('shape', [(2, 16, 24, 20, 37, 3, 1), (1, 72, 136, 9, 33, 3, 1), (3, 64, 64, 17, 17, 1, 1), (8, 64, 64, 64, 64, 3, 1), (2, 16, 24, 21, 37, 3, 2), (4, 64, 64, 65, 65, 3, 2),
                                   (1, 128, 128, 70, 66, 3, 1)],
                         ids=['3x3_ragged', '3x3_multi_block', '1x1', '3x3_many_chunks', '3x3s2_ragged', '3x3s2_odd_input', '3x3_ragged_pixels'])
def test_weight_gradient_bf16x3(shape, monkeypatch):
    """PG_WGRAD_BF16X3=1 (round 5, exploratory: VERDICT r4 item 7): the float32 weight gradient on the bf16 matrix pipe by three-term operand splitting
    (csrc/conv2d_wgrad.hip: pg_split3_bf16_cl + pg_conv2d16_wgrad_x3).  (a) the split is exact: plane 0 + plane 1 + plane 2 == x bit for bit, every plane
    bf16-representable; (b) small-integer data: bit-exact against the float64 gradient, like the fp32 kernel; (c) random float32 data with a wide dynamic range:
    within 4e-6 of max|dw| of the float64 gradient -- the fp32 MFMA kernel's own class (it measures 1e-6 ... 2e-6 on the same data)."""
    from torch_utils.ops import conv2d_mfma
    from torch_utils.ops import _native as nat
    n, cin, cout, h, w, k, st = shape
    monkeypatch.setenv('PG_WGRAD_BF16X3', '1')
    assert conv2d_mfma._bf16x3_wanted(n, cin, cout, h, w, k, k, st)
    gen = torch.Generator().manual_seed(n * 1000 + cin + st)
    oh, ow = (h + 2 * (k // 2) - k) // st + 1, (w + 2 * (k // 2) - k) // st + 1
    # (a) the splitting pass
    xr = (torch.randn([n, cin, h, w], generator=gen) * torch.exp(4 * torch.randn([n, cin, 1, 1], generator=gen))).to(DEV)
    lib = conv2d_mfma._init().lib
    planes = torch.empty([3, n, h, w, cin], dtype=torch.bfloat16, device=DEV)
    nat.check(lib.pg_split3_bf16_cl(nat.ptr(xr), nat.ptr(planes), n, cin, h * w, nat.stream_of(xr)), 'pg_split3_bf16_cl')
    back = planes.float().permute(0, 1, 4, 2, 3)                      # [3, N, C, H, W]
    assert torch.equal((back[0] + back[1]) + back[2], xr)
    assert float(back[1].abs().max()) <= float(xr.abs().max()) * 2.0 ** -7 and float(back[2].abs().max()) <= float(xr.abs().max()) * 2.0 ** -15

    def f64(xx, dd):
        wref = torch.zeros([cout, cin, k, k], dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(xx.double().cpu(), wref, padding=k // 2, stride=st).backward(dd.double().cpu())
        return wref.grad
    # (b) integers
    x = torch.randint(-3, 4, [n, cin, h, w], generator=gen).float()
    dy = torch.randint(-2, 3, [n, cout, oh, ow], generator=gen).float()
    calls = []
    real = lib.pg_conv2d16_wgrad_x3
    monkeypatch.setattr(lib, 'pg_conv2d16_wgrad_x3', lambda *a: (calls.append(1), real(*a))[1])
    got = conv2d_mfma.weight_gradient(x.to(DEV), dy.to(DEV), [cout, cin, k, k], (k // 2, k // 2), stride=st)
    assert calls, 'the bf16x3 route did not run'
    ref = f64(x, dy)
    assert torch.equal(got.double().cpu(), ref), float((got.double().cpu() - ref).abs().max())
    # (c) random data
    dyr = (torch.randn([n, cout, oh, ow], generator=gen) * 0.01).to(DEV)
    got = conv2d_mfma.weight_gradient(xr, dyr, [cout, cin, k, k], (k // 2, k // 2), stride=st)
    ref = f64(xr, dyr)
    monkeypatch.setenv('PG_WGRAD_BF16X3', '0')
    plain = conv2d_mfma.weight_gradient(xr, dyr, [cout, cin, k, k], (k // 2, k // 2), stride=st)
    e3, e1 = float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max()), float((plain.double().cpu() - ref).abs().max()) / float(ref.abs().max())
    print(f'bf16x3 {e3:.2e} of max|dw|, fp32 kernel {e1:.2e}')
    assert e3 <= max(4e-6, 3 * e1), (e3, e1)


def test_conv2d_gradfix_native_backward_routes():
    """First-order backward of conv2d_gradfix.conv2d on the GPU: input gradient through the MFMA / Winograd kernels with the
    flipped, transposed pack taken straight from the parameter, weight gradient through the native GEMM-over-pixels kernel --
    against PyTorch's own double-precision convolution."""
    from torch_utils.ops import conv2d_gradfix, conv2d_mfma
    assert conv2d_gradfix.native_input_gradients
    calls = {'wgrad': 0}
    real_wgrad, was = conv2d_mfma.weight_gradient, conv2d_gradfix.native_weight_gradients
    conv2d_gradfix.native_weight_gradients = True       # the default; set explicitly so that an exported PG_NATIVE_WGRAD=0 cannot hollow out the check

    def counting_wgrad(*a, **k):
        out = real_wgrad(*a, **k)
        calls['wgrad'] += out is not None
        return out
    conv2d_mfma.weight_gradient = counting_wgrad
    gen = torch.Generator().manual_seed(31)
    try:
        _native_backward_cases(conv2d_gradfix, gen)
    finally:
        conv2d_mfma.weight_gradient = real_wgrad
        conv2d_gradfix.native_weight_gradients = was
    assert calls['wgrad'] == 3          # every case took the native weight-gradient kernel (the route, not only the numbers)


@pytest.mark.parametrize('case', [
    # name, dtype, N, cin, cout, k, stride, pad, (H, W)
    ('k3',          torch.float16,  2, 64, 64, 3, 1, 1, (40, 48)),
    ('k3_odd',      torch.float16,  1, 128, 72, 3, 1, 1, (17, 45)),
    ('k3_multi',    torch.float16,  3, 64, 128, 3, 1, 1, (128, 96)),
    ('k3_s2',       torch.float16,  2, 32, 64, 3, 2, 0, (35, 35)),
    ('k3_s2_pad',   torch.float16,  1, 64, 64, 3, 2, 1, (64, 50)),
    ('k1',          torch.float16,  2, 64, 128, 1, 1, 0, (33, 20)),
    ('fromrgb',     torch.float16,  2, 6, 64, 1, 1, 0, (32, 32)),
    ('k3_bf16',     torch.bfloat16, 2, 64, 64, 3, 1, 1, (24, 40)),
    ('k3_wide',     torch.float16,  1, 512, 512, 3, 1, 1, (16, 16)),
])
def test_native_weight_gradient_16bit(case):
    """conv2d16_wgrad (channels-last fp16 / bf16 operands, transposing LDS reads, fp32 accumulation) against float64 autograd of torch's convolution
    on the same 16-bit values: products of 16-bit numbers are exact in fp32, so only the summation order differs; twice -> bit-identical."""
    from torch_utils.ops import conv2d_mfma16
    name, dt, n, cin, cout, k, stride, pad, hw = case
    gen = torch.Generator().manual_seed(hash(name) % 1000)
    x = torch.randn([n, cin, *hw], generator=gen).to(dt)
    oh, ow = (hw[0] + 2 * pad - k) // stride + 1, (hw[1] + 2 * pad - k) // stride + 1
    dy = torch.randn([n, cout, oh, ow], generator=gen).to(dt)
    w64 = torch.zeros([cout, cin, k, k], dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(torch.nn.functional.conv2d(x.double(), w64, stride=stride, padding=pad), [w64], dy.double())
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    dyd = dy.to(DEV).contiguous(memory_format=torch.channels_last)
    got = conv2d_mfma16.weight_gradient(xd, dyd, (cout, cin, k, k), (pad, pad), stride=stride)
    assert got is not None and got.dtype == torch.float32 and tuple(got.shape) == (cout, cin, k, k)
    close(got, ref, 1e-4, 2e-5 * scale_of(ref))
    assert torch.equal(got, conv2d_mfma16.weight_gradient(xd, dyd, (cout, cin, k, k), (pad, pad), stride=stride))
    # NCHW-strided inputs are converted; through conv2d_gradfix the gradient arrives in the weight's dtype
    from torch_utils.ops import conv2d_gradfix
    wd = (torch.randn([cout, cin, k, k], generator=gen) / np.sqrt(cin * k * k)).to(dt).to(DEV).requires_grad_(True)
    y = conv2d_gradfix.conv2d(x.to(DEV), wd, stride=stride, padding=pad)
    gw, = torch.autograd.grad(y, [wd], dy.to(DEV))
    assert gw.dtype == dt
    close(gw, ref, 2e-2 if dt == torch.bfloat16 else 3e-3, (2e-2 if dt == torch.bfloat16 else 3e-3) * scale_of(ref))


def test_conv2d_gradfix_weight_gradient_is_differentiable():
    """create_graph with the weight gradient in the graph (the role of the reference's Conv2dGradWeight.backward, conv2d_gradfix.py:151-168):
    dw from the native kernel, then d(|dw|^2)/dx and /d(dy) through `_WeightGradient.backward` -- against float64 autograd of torch's own
    convolution, for a plain, a strided and a transposed case; the aten route must not have been taken."""
    from torch_utils.ops import conv2d_gradfix
    calls = {'n': 0}
    real = conv2d_gradfix._WeightGradient.forward

    def counting(ctx, *a):
        calls['n'] += 1
        return real(ctx, *a)
    conv2d_gradfix._WeightGradient.forward = staticmethod(counting)
    gen = torch.Generator().manual_seed(77)
    try:
        for kind, cin, cout, k, stride, pad, hw in (('conv', 32, 48, 3, 1, 1, (18, 22)), ('conv', 16, 32, 3, 2, 1, (21, 21)), ('conv', 24, 40, 1, 1, 0, (12, 14)),
                                                     ('transposed', 16, 24, 3, 2, 0, (10, 12))):
            x = torch.randn([2, cin, *hw], generator=gen)
            wshape = [cout, cin, k, k] if kind == 'conv' else [cin, cout, k, k]
            wt = torch.randn(wshape, generator=gen) / np.sqrt(cin * k * k)
            f_dev = (lambda a, b: conv2d_gradfix.conv2d(a, b, stride=stride, padding=pad)) if kind == 'conv' else (lambda a, b: conv2d_gradfix.conv_transpose2d(a, b, stride=stride, padding=pad))
            f_ref = (lambda a, b: torch.nn.functional.conv2d(a, b, stride=stride, padding=pad)) if kind == 'conv' else (lambda a, b: torch.nn.functional.conv_transpose2d(a, b, stride=stride, padding=pad))
            xd, wd = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True)
            y = f_dev(xd, wd)
            dy = torch.randn(y.shape, generator=gen)
            dyd = dy.to(DEV).requires_grad_(True)
            gw, = torch.autograd.grad(y, [wd], dyd, create_graph=True)
            hx, hdy = torch.autograd.grad(gw.square().sum(), [xd, dyd])
            x64, w64, dy64 = x.double().requires_grad_(True), wt.double().requires_grad_(True), dy.double().requires_grad_(True)
            rw, = torch.autograd.grad(f_ref(x64, w64), [w64], dy64, create_graph=True)
            rx, rdy = torch.autograd.grad(rw.square().sum(), [x64, dy64])
            close(gw, rw, 1e-4, 1e-5 * scale_of(rw))
            close(hx, rx, 2e-4, 2e-5 * scale_of(rx))
            close(hdy, rdy, 2e-4, 2e-5 * scale_of(rdy))
    finally:
        conv2d_gradfix._WeightGradient.forward = staticmethod(real)
    assert calls['n'] == 4


def _native_backward_cases(conv2d_gradfix, gen):
    for cin, cout, k, hw in ((32, 80, 3, (20, 24)), (16, 24, 3, (13, 19)), (64, 48, 1, (17, 21))):
        x = torch.randn([2, cin, *hw], generator=gen)
        wt = torch.randn([cout, cin, k, k], generator=gen) / np.sqrt(cin * k * k)
        b = torch.randn([cout], generator=gen)
        dy = torch.randn([2, cout, *hw], generator=gen)
        xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, wt, b))
        y = conv2d_gradfix.conv2d(xd, wd, bd, padding=k // 2)
        gx, gw, gb = torch.autograd.grad(y, [xd, wd, bd], dy.to(DEV))
        x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
        rx, rw, rb = torch.autograd.grad(torch.nn.functional.conv2d(x64, w64, b64, padding=k // 2), [x64, w64, b64], dy.double())
        close(gx, rx, 1e-4, 1e-5 * scale_of(rx))
        close(gw, rw, 1e-4, 1e-5 * scale_of(rw))
        close(gb, rb, 1e-4, 1e-5 * scale_of(rb))


@pytest.mark.gpu
@pytest.mark.parametrize('case', [('conv3', 64, 64, 64, 3), ('conv3_wide', 128, 96, 32, 3), ('torgb', 64, 3, 64, 1), ('up2', 64, 32, 64, 3), ('up2_big', 128, 64, 128, 3)])
def test_modulated_conv_training_route_native_vs_graph(case):
    """_ModConvTrain (one forward launch; backward = bias_act' + db pass, input gradient with the scales riding in the launch, per-sample
    weight gradients folded into dw / dstyles / ddcoefs) against the differentiable composition of the same layer (the route the oracle
    comparison of the whole generator has pinned): output and the gradients of x, w, every parameter.  A double-backward request is refused."""
    from training import networks as PN
    name, cin, cout, res, k = case
    torch.manual_seed(3)
    if k == 3:
        layer = PN.SynthesisLayer(cin, cout, w_dim=64, resolution=res, conv_clamp=256, up=2 if name.startswith('up2') else 1).to(DEV).train()
        with torch.no_grad():
            layer.noise_strength.fill_(0.3)
            layer.bias.copy_(det_tensor(f'mt.{name}.b', [cout]).to(DEV))
        call = lambda x, w: layer(x, w, noise_mode='const', fused_modconv=False, gain=0.8)
    else:
        layer = PN.ToRGBLayerFull_v1_v5(cin, cout, w_dim=64, conv_clamp=256, is_last=True, is_style=True).to(DEV).train()
        with torch.no_grad():
            layer.bias.copy_(det_tensor(f'mt.{name}.b', [cout]).to(DEV))
        def call(x, w):
            rgb, parsing = layer(x, w, fused_modconv=False)
            return torch.cat([rgb, parsing], dim=1)
    res_in = res // 2 if name.startswith('up2') else res
    x0 = det_tensor(f'mt.{name}.x', [3, cin, res_in, res_in]).to(DEV)
    w0 = det_tensor(f'mt.{name}.w', [3, 64]).to(DEV)
    params = [p for p in layer.parameters()]

    def run(fused):
        was = PN.fused_training_modconv
        PN.fused_training_modconv = fused
        try:
            x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
            y = call(x, w)
            dy = det_tensor(f'mt.{name}.dy', list(y.shape)).to(DEV)
            return y, torch.autograd.grad(y, [x, w] + params, dy, allow_unused=True), (x, y)
        finally:
            PN.fused_training_modconv = was
    ya, ga, (xa, yya) = run(True)
    assert yya.grad_fn is not None and type(yya.grad_fn).__name__ in ('_ModConvTrainBackward', '_ModConvUp2TrainBackward', 'CatBackward0'), type(yya.grad_fn).__name__
    yb, gb, (_, yyb) = run(False)
    assert 'ModConv' not in type(yyb.grad_fn).__name__
    close(ya, yb, 2e-5, 2e-5 * scale_of(yb))
    assert len(ga) == len(gb)
    for a, b in zip(ga, gb):
        assert (a is None) == (b is None)
        if a is not None:
            close(a, b, 2e-4, 3e-5 * scale_of(b))
    was = PN.fused_training_modconv
    PN.fused_training_modconv = True
    try:
        x = x0.clone().requires_grad_(True)
        g, = torch.autograd.grad(call(x, w0).sum(), [x], create_graph=True)
        with pytest.raises(RuntimeError):
            g.square().sum().backward()
    finally:
        PN.fused_training_modconv = was


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [[2, 32, 40, 36], [1, 5, 7, 9], [4, 128, 64, 64]])
def test_spade_combine_training_route_vs_float64_autograd(shape):
    """_SpadeCombine (instance norm -> x_hat (1 + gamma) + beta, networks.py:1715-1723) forward and gradient -- dx through the norm, dgamma, dbeta --
    against float64 autograd of the composed expression; a second run is bit-identical; a create_graph request differentiates the composition."""
    from training import networks as PN
    n, c, h, w = shape
    x = det_tensor(f'sc.{shape}.x', shape, scale=2.0) + 0.5
    gb = det_tensor(f'sc.{shape}.gb', [n, 2 * c, h, w])
    dy = det_tensor(f'sc.{shape}.dy', shape)
    x64, gb64 = x.double().requires_grad_(True), gb.double().requires_grad_(True)
    y64 = torch.nn.functional.instance_norm(x64, eps=1e-5) * (1 + gb64[:, :c]) + gb64[:, c:]
    rx, rgb = torch.autograd.grad(y64, [x64, gb64], dy.double())
    xd, gbd = x.to(DEV).requires_grad_(True), gb.to(DEV).requires_grad_(True)
    y = PN._SpadeCombine.apply(xd, gbd, 1e-5)
    gx, ggb = torch.autograd.grad(y, [xd, gbd], dy.to(DEV))
    close(y, y64, 2e-5, 2e-5 * scale_of(y64))
    close(gx, rx, 1e-4, 2e-5 * scale_of(rx))
    close(ggb, rgb, 2e-5, 2e-5 * scale_of(rgb))
    y2 = PN._SpadeCombine.apply(xd, gbd, 1e-5)
    gx2, ggb2 = torch.autograd.grad(y2, [xd, gbd], dy.to(DEV))
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and torch.equal(ggb, ggb2)
    # only one of the two gradients requested
    only_x, = torch.autograd.grad(PN._SpadeCombine.apply(xd, gbd.detach(), 1e-5), [xd], dy.to(DEV))
    assert torch.equal(only_x, gx)
    only_gb, = torch.autograd.grad(PN._SpadeCombine.apply(xd.detach(), gbd, 1e-5), [gbd], dy.to(DEV))
    assert torch.equal(only_gb, ggb)
    if n * c * h * w < 1e5:     # second order through the fall-back composition
        g1, = torch.autograd.grad(PN._SpadeCombine.apply(xd, gbd, 1e-5), [xd], dy.to(DEV), create_graph=True)
        g2, = torch.autograd.grad(g1.square().sum(), [gbd])
        r1, = torch.autograd.grad(torch.nn.functional.instance_norm(x64, eps=1e-5) * (1 + gb64[:, :c]) + gb64[:, c:], [x64], dy.double(), create_graph=True)
        r2, = torch.autograd.grad(r1.square().sum(), [gb64])
        close(g2, r2, 1e-3, 1e-4 * scale_of(r2))


@pytest.mark.gpu
@pytest.mark.parametrize('case', [
    # name, dtype, cin, cout, k, down, hw, act, clamp
    ('f32_k3_lrelu', torch.float32, 64, 64, 3, 1, (40, 48), 'lrelu', 1.2),
    ('f32_k3_wino4', torch.float32, 64, 64, 3, 1, (72, 72), 'lrelu', None),
    ('f32_k3_down2', torch.float32, 32, 64, 3, 2, (32, 32), 'lrelu', 256),
    ('f32_k1_down2', torch.float32, 32, 48, 1, 2, (24, 24), 'linear', None),
    ('f32_k4_relu',  torch.float32, 16, 32, 4, 1, (20, 20), 'relu', None),
    ('f16_k3_lrelu', torch.float16, 64, 64, 3, 1, (32, 32), 'lrelu', 256),
    ('f16_k3_down2', torch.float16, 32, 64, 3, 2, (32, 32), 'lrelu', 256),
])
def test_conv_layer_training_route_epilogue_in_the_launch(case):
    """Conv2dLayer on the training route (networks.py:170-179: conv2d_resample -> bias_act): with the bias_act in the convolution's epilogue
    (conv2d_gradfix `_epilogue`, derivative from the saved output, db from the same pass) against the two-op composition of the same
    kernels -- output, first-order gradients of x / weight / bias, and the R1-style second order d/dw of |dy/dx|^2."""
    from training import networks as PN
    from torch_utils.ops import conv2d_gradfix
    name, dt, cin, cout, k, down, hw, act, clamp = case
    layer = fill_module_(PN.Conv2dLayer(cin, cout, kernel_size=k, activation=act, down=down, conv_clamp=clamp), f'ep.{name}.').to(DEV).train()
    with torch.no_grad():
        layer.bias.copy_(det_tensor(f'ep.{name}.b', [cout]).to(DEV))
    fmt = torch.channels_last if dt == torch.float16 else torch.contiguous_format
    x0 = det_tensor(f'ep.{name}.x', [2, cin, *hw]).to(DEV).to(dt).contiguous(memory_format=fmt)

    def run(fused):
        was = conv2d_gradfix.fused_epilogue
        conv2d_gradfix.fused_epilogue = fused
        try:
            x = x0.clone().requires_grad_(True)
            y = layer(x, gain=0.7)
            dy = det_tensor(f'ep.{name}.dy', list(y.shape)).to(DEV).to(dt)
            gx, = torch.autograd.grad(y, [x], dy, create_graph=True)
            pen = gx.float().square().sum()
            g2 = torch.autograd.grad(pen, [layer.weight, layer.bias], allow_unused=True, retain_graph=True)
            g1 = torch.autograd.grad(y, [layer.weight, layer.bias], dy)
            return y, gx, g1, g2
        finally:
            conv2d_gradfix.fused_epilogue = was
    ya, gxa, g1a, g2a = run(True)
    yb, gxb, g1b, g2b = run(False)
    tol = 2e-5 if dt == torch.float32 else 4e-3
    close(ya, yb, tol, tol * scale_of(yb))
    close(gxa, gxb, tol, tol * scale_of(gxb))
    for a, b in zip(g1a + g2a, g1b + g2b):
        if a is None or b is None:       # "no dependence": None on one route may be an all-zero tensor on the other
            assert all(t is None or float(t.abs().max()) == 0.0 for t in (a, b))
        else:
            close(a, b, 10 * tol, 10 * tol * scale_of(b))


@pytest.mark.gpu
@pytest.mark.parametrize('cout,cin,hw,use_styles,use_skip,clamp', [(3, 64, (32, 36), True, True, 256.0), (7, 20, (16, 8), True, False, 0.5),
                                                                  (1, 8, (4, 4), False, False, None), (8, 130, (10, 12), True, True, None),
                                                                  (3, 512, (8, 8), True, True, 256.0), (3, 96, (128, 128), True, True, 256.0), (7, 64, (96, 128), True, False, 2.0),
                                                                  (3, 64, (512, 256), True, True, 256.0)])
def test_streaming_head_fp32(cout, cin, hw, use_styles, use_skip, clamp):
    """pg_conv1x1_small (the fp32 ToRGB / parsing heads as one streaming pass) against the same arithmetic in float64.  Images too small to give every CU a
    workgroup (cases 1, 4-7: 4 / 4 / 4 / 16 / 16 pixel quads per workgroup) run the channel-split form of round 5, the last case and the narrow ones the first form."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(100 * cout + cin)
    x = torch.randn([3, cin, *hw], generator=gen)
    w = torch.randn([cout, cin, 1, 1], generator=gen)
    styles = torch.randn([3, cin], generator=gen) if use_styles else None
    bias = torch.randn([cout], generator=gen)
    skip = torch.randn([3, cout, *hw], generator=gen) if use_skip else None
    assert conv2d_mfma.conv1x1_small_ok(x.to(DEV), w.to(DEV), skip.to(DEV) if use_skip else None)
    y = conv2d_mfma.conv1x1_small(x.to(DEV), w.to(DEV), styles.to(DEV) if use_styles else None, bias.to(DEV),
                                  skip=skip.to(DEV) if use_skip else None, scale=0.37, clamp=clamp)
    xs = x.double() * (styles.double()[:, :, None, None] if use_styles else 1.0)
    ref = torch.nn.functional.conv2d(xs, w.double() * 0.37) + bias.double()[None, :, None, None]
    if clamp is not None:
        ref = ref.clamp(-clamp, clamp)
    if use_skip:
        ref = ref + skip.double()
    close(y, ref, 1e-5, 1e-5 * scale_of(ref))


@pytest.mark.gpu
@pytest.mark.parametrize('n,h,w,cout,act', [(2, 9, 12, 5, 'relu'), (1, 1, 4, 3, 'linear'), (3, 33, 64, 64, 'relu')])
def test_one_channel_stencil_conv(n, h, w, cout, act):
    """pg_conv3x3_cin1 (the SPADE blocks' first layer on the one-channel map) against F.conv2d in float64."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(7 * h + w)
    x = torch.randn([n, 1, h, w], generator=gen)
    wt = torch.randn([cout, 1, 3, 3], generator=gen)
    assert conv2d_mfma.conv3x3_cin1_ok(x.to(DEV), wt.to(DEV))
    y = conv2d_mfma.conv3x3_cin1(x.to(DEV), wt.to(DEV), scale=0.61, act=act)
    ref = torch.nn.functional.conv2d(x.double(), wt.double() * 0.61, padding=1)
    if act == 'relu':
        ref = ref.relu()
    close(y, ref, 1e-5, 1e-6 * scale_of(ref))


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cout,h,w,mod', [(2, 16, 32, 8, 32, True), (1, 5, 7, 9, 13, True), (3, 24, 40, 17, 33, False), (1, 64, 64, 32, 64, True),
                                               (1, 3, 2, 1, 1, True), (2, 8, 33, 2, 40, False), (1, 17, 5, 40, 2, True), (1, 9, 64, 8, 31, True),
                                               (2, 16, 40, 16, 16, True), (2, 32, 32, 8, 8, True), (1, 8, 8, 33, 7, False),      # 16- and 8-wide position tiles
                                               (2, 256, 64, 16, 16, True), (3, 128, 33, 9, 13, True), (4, 512, 96, 8, 8, True), (1, 192, 32, 40, 36, False)])      # split-K: 4, 2, 8, 2 shares
def test_fused_up2_transposed_conv(n, cin, cout, h, w, mod):
    """pg_conv2d_up2_forward (all four parities of the stride-2 transposed 3x3 convolution in one launch, modulation prologue,
    demodulation epilogue, pitched output) against conv_transpose2d in float64.  The last four cases have few tiles and >= 16 K chunks: they run the split-K form
    of round 5 (pg_conv2d_up2_forward_splitk: shares of the input channels in workspace slices + one summing pass), main and edge tiles alike."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(1000 * n + cin + w)
    x = torch.randn([n, cin, h, w], generator=gen)
    wt = torch.randn([cout, cin, 3, 3], generator=gen) / np.sqrt(cin * 9)          # OIHW as the kernel indexes it: y[2iy+ky] += x[iy] w[co,ci,ky,kx]
    s_in = torch.randn([n, cin], generator=gen) if mod else None
    s_out = torch.rand([n, cout], generator=gen) + 0.5 if mod else None
    flip = bool((n + cin) % 2)                     # pack_up2 flips iff asked: hand it the pre-flipped kernel then
    wdev = (wt.flip([2, 3]) if flip else wt).contiguous().to(DEV)
    packs = conv2d_mfma.pack_up2(wdev, flip=flip)
    y = conv2d_mfma.conv_up2_forward(x.to(DEV), packs, cout, in_scale=s_in.to(DEV) if mod else None, out_scale=s_out.to(DEV) if mod else None)
    assert y.shape == (n, cout, 2 * h + 1, 2 * w + 1) and y.stride(2) % 4 == 0
    if cin >= 128:
        assert conv2d_mfma._init().lib.pg_conv2d_up2_splitk_plan(n, cin, h, w, cout) > 1
    xs = x.double() * (s_in.double()[:, :, None, None] if mod else 1.0)
    ref = torch.nn.functional.conv_transpose2d(xs, wt.double().transpose(0, 1), stride=2)
    if mod:
        ref = ref * s_out.double()[:, :, None, None]
    close(y, ref, 1e-5, 2e-6 * scale_of(ref))
    # the FIR pass reads the pitched tensor in place
    from torch_utils.ops import upfirdn2d
    f = upfirdn2d.setup_filter([1, 3, 3, 1]).to(DEV)
    ref1 = upfirdn2d.upfirdn2d(y.contiguous(), f, padding=[1, 1, 1, 1], gain=4)          # dense rows: the generic tiled kernel; pitched rows: the 16-byte blur kernel
    close(upfirdn2d.upfirdn2d(y, f, padding=[1, 1, 1, 1], gain=4), ref1, 1e-6, 1e-6 * scale_of(ref1))
    for pad in ([2, 2, 2, 2], [0, 3, 1, 2], [3, 0, 2, 1]):                                     # every footprint misalignment D of the blur kernel
        refp = upfirdn2d.upfirdn2d(y.contiguous(), f, padding=pad)
        if refp.shape[3] % 4 == 0:
            close(upfirdn2d.upfirdn2d(y, f, padding=pad), refp, 1e-6, 1e-6 * scale_of(refp))
    fused = upfirdn2d.upfirdn2d_bias_act(y, f, padding=[1, 1, 1, 1], gain=4, b=torch.zeros(cout, device=DEV), act='lrelu', act_gain=1.0)
    ref2 = torch.nn.functional.leaky_relu(upfirdn2d.upfirdn2d(y.contiguous(), f, padding=[1, 1, 1, 1], gain=4), 0.2)
    close(fused, ref2, 1e-6, 1e-6 * scale_of(ref2))


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cout,h,w', [(1, 32, 32, 8, 32), (2, 48, 40, 21, 36), (1, 64, 96, 33, 64), (3, 32, 70, 17, 100), (2, 128, 64, 40, 96), (8, 128, 64, 256, 256), (2, 512, 256, 64, 64)])
def test_up2_transposed_conv_on_the_bf16_pipe_is_float32_class(n, cin, cout, h, w, monkeypatch):
    """csrc/conv2d_up2x3.h (round 6): the fp32 `up = 2` layer's stride-2 transposed 3x3 convolution (conv2d_resample.py:125-142 -> conv2d_gradfix.conv_transpose2d)
    with every float32 operand as the exact sum of three bf16 values and each float32 product as six bf16 products on v_mfma_f32_32x32x16_bf16 (fp32 accumulation);
    main tiles by the new kernel (producer waves: 16-byte halo words -> LDS -> split planes; multiplying waves: 108 MFMAs per 16-channel chunk), the last output
    column / row by the fp32 kernel's edge pass.  Admissible as float32 only if it IS float32-class: referee float64, error <= 2x the fp32-MFMA kernel's on the same
    launch (measured 0.6-1.0x) and <= 2e-6 of the output scale; plain and modulated (input scale applied before the split, demodulation after); ragged heights (H % 8
    != 0), widths that are no multiple of 32, Cout % 32 != 0, Cin = 32 (two chunks: the producers' one-round-ahead requests at their shortest); bit-identical
    repeats; the pitched output the FIR pass reads in place."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(7 * cin + cout + h)
    x = torch.randn([n, cin, h, w], generator=gen).to(DEV)
    wt = (torch.randn([cout, cin, 3, 3], generator=gen) / (3 * math.sqrt(cin))).to(DEV)
    s_in, s_out = (torch.rand([n, cin], generator=gen) + 0.5).to(DEV), (torch.rand([n, cout], generator=gen) + 0.5).to(DEV)
    packs = conv2d_mfma.pack_up2(wt)
    assert 'x3' in packs and packs['x3'].numel() == conv2d_mfma._init().lib.pg_conv2d_up2x3_packed_size(cout, cin)
    if conv2d_mfma._init().lib.pg_conv2d_up2_splitk_plan(n, cin, h, w, cout) > 1:
        pytest.skip('split-K plan: this launch stays on the fp32 kernel')
    for kw in (dict(), dict(in_scale=s_in, out_scale=s_out)):
        xs = x.double() * (s_in.double()[:, :, None, None] if kw else 1.0)
        ref = torch.nn.functional.conv_transpose2d(xs, wt.double().transpose(0, 1), stride=2)
        if kw:
            ref = ref * s_out.double()[:, :, None, None]
        sc = float(ref.abs().max())
        monkeypatch.setattr(conv2d_mfma, 'UP2_X3', False)
        y32 = conv2d_mfma.conv_up2_forward(x, packs, cout, **kw)
        monkeypatch.setattr(conv2d_mfma, 'UP2_X3', True)
        tl = conv2d_mfma.start_timeline()
        y = conv2d_mfma.conv_up2_forward(x, packs, cout, **kw)
        conv2d_mfma.stop_timeline()
        assert ' x3' in tl[-1][0][4], tl[-1][0]                        # the launch did take the bf16x3 kernel
        assert y.shape == (n, cout, 2 * h + 1, 2 * w + 1) and y.stride(2) % 4 == 0
        e32, e = float((y32.double() - ref).abs().max()), float((y.double() - ref).abs().max())
        assert e <= 2 * e32 and e <= 2e-6 * sc, (e / sc, e32 / sc)
        for _ in range(3):
            assert torch.equal(conv2d_mfma.conv_up2_forward(x, packs, cout, **kw), y)


@pytest.mark.gpu
@pytest.mark.parametrize('n,cout,h,w,act,clamp', [(2, 64, 64, 64, 'relu', None), (1, 64, 37, 100, 'lrelu', 0.4), (1, 48, 33, 300, 'linear', None), (2, 128, 70, 260, 'relu', None),
                                                  (1, 64, 5, 7, 'relu', None)])
def test_stem7_conv_on_the_bf16_pipe_is_float32_class(n, cout, h, w, act, clamp):
    """csrc/conv2d_stem7x3.h (round 6): the garment encoder's 7x7 three-channel stem (networks.py:2233-2238 -> conv2d_resample.py:145-147, bias_act in the epilogue)
    with every float32 operand as the exact sum of three bf16 values, six plane products per float32 product on v_mfma_f32_32x32x16_bf16, float32 accumulation;
    column records sliding down a 256-column strip, weights resident in registers.  Admissible as float32 only if it IS float32-class: referee float64, error <= 2x
    the fp32-MFMA kernel's on the same launch and <= 2e-6 of the output scale; ragged strips (W % 256 != 0, two strips), ragged row segments (H % 32 != 0), images
    smaller than the kernel, Cout % 64 != 0 and two m-pairs, bias / activation / gain / clamp in the epilogue; bit-identical repeats."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(11 * cout + h + w)
    x = (torch.rand([n, 3, h, w], generator=gen) * 2 - 1).to(DEV)
    wt = torch.randn([cout, 3, 7, 7], generator=gen).to(DEV)
    bias = torch.randn([cout], generator=gen).to(DEV)
    scale, gain = 1 / math.sqrt(3 * 49), math.sqrt(2)
    alpha = 0.2 if act == 'lrelu' else 0.0
    pre = torch.nn.functional.conv2d(x.double(), wt.double() * scale, padding=3) + bias.double()[None, :, None, None]
    ref = {'linear': pre, 'relu': pre.clamp(min=0), 'lrelu': torch.where(pre > 0, pre, pre * alpha)}[act] * gain
    if clamp is not None:
        ref = ref.clamp(-clamp, clamp)
    packed = conv2d_mfma.pack_stem7(wt, scale=scale)
    assert packed.numel() == conv2d_mfma._init().lib.pg_conv2d_stem7x3_packed_size(cout)
    y = conv2d_mfma.conv_stem7_forward(x, packed, cout, bias=bias, act=act, alpha=alpha, gain=gain, clamp=clamp)
    y32 = conv2d_mfma.conv2d_forward(x, conv2d_mfma.pack_weight(wt, scale=scale), cout, 7, 7, pad=(3, 3), bias=bias, act=act, alpha=alpha, gain=gain, clamp=clamp)
    assert y.shape == ref.shape
    sc = float(pre.abs().max())
    e32, e = float((y32.double() - ref).abs().max()), float((y.double() - ref).abs().max())
    assert e <= 2 * e32 and e <= 2e-6 * sc, (e / sc, e32 / sc)
    for _ in range(2):
        assert torch.equal(conv2d_mfma.conv_stem7_forward(x, packed, cout, bias=bias, act=act, alpha=alpha, gain=gain, clamp=clamp), y)


@pytest.mark.gpu
@pytest.mark.parametrize('n,c,h,w', [(2, 5, 64, 64), (1, 3, 37, 50), (3, 4, 37, 51), (1, 64, 512, 512), (2, 2, 4, 6)])
def test_fir_pass_shared_by_the_two_down2_layers_of_a_res_block(n, c, h, w, monkeypatch):
    """pg_upfirdn2d_with_odd_samples (round 6): the FIR pass in front of a strided 3x3 convolution (padding p + 1, conv2d_resample.py:119-122) also writes its odd
    rows / columns densely -- bit for bit what the FIR pass in front of the 1x1 skip convolution computes (down = 2, padding p: conv2d_resample.py:107-110).  Then a
    whole ResBlock(down = 2) with and without the shared pass: identical outputs."""
    from torch_utils.ops import upfirdn2d
    from training import networks as PN
    from training.synthetic import fill_module_ as fill
    gen = torch.Generator().manual_seed(71)
    x = torch.randn([n, c, h, w], generator=gen).to(DEV)
    f = upfirdn2d.setup_filter([1, 3, 3, 1]).to(DEV)
    y, y_odd = upfirdn2d.filter_with_odd_samples(x, f, padding=[2, 2, 2, 2])
    assert torch.equal(y, upfirdn2d.upfirdn2d(x, f, padding=[2, 2, 2, 2]))
    assert torch.equal(y_odd, upfirdn2d.upfirdn2d(x, f, down=2, padding=[1, 1, 1, 1]))
    for _ in range(3):                                 # (odd input extents: the full pass then has one odd row / column more than the decimated pass keeps -- it must
        y2, y2_odd = upfirdn2d.filter_with_odd_samples(x, f, padding=[2, 2, 2, 2])      #  not be written past the end of a plane: round 6's first build raced there)
        assert torch.equal(y2, y) and torch.equal(y2_odd, y_odd)
    if c >= 3 and h >= 8:
        blk = fill(PN.ResBlock(c, 2 * c, kernel_size=4, activation='relu', down=2), 'fs.res.').to(DEV).eval()
        calls = []
        real = upfirdn2d.filter_with_odd_samples
        monkeypatch.setattr(upfirdn2d, 'filter_with_odd_samples', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        with torch.no_grad():
            a = blk(x)
            assert calls == [1]
            monkeypatch.setenv('PG_FIR_SHARED', '0')
            b = blk(x)
            assert calls == [1]
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_spade_res_block_gathers_its_statistics_in_the_convolution_tails(monkeypatch):
    """A SPADE res-block at the widths of the generator (128 channels, 64^2: the F(4x4) kernel's wide form, whichever `conv2d_mfma.F4_WIDE` names) makes NO
    separate instance-norm statistics pass: the three norm blocks' statistics come out of the tails of the convolutions that produce their inputs (round 4).
    Round 6 had lost that silently when the bf16x3 form became the default (`wg == 2` in Spade_Conv2dLayer.forward: six extra passes, 0.42 ms of the config-2 step)."""
    from training import networks as PN
    from training.synthetic import fill_module_
    from torch_utils.ops import conv2d_mfma
    blk = fill_module_(PN.Spade_ResBlockV4_512(128, 128, spade_channels=128), 'st.spade.').to(DEV).eval()
    gen = torch.Generator().manual_seed(67)
    x = torch.randn([2, 128, 64, 64], generator=gen).to(DEV)
    feat = torch.randn([2, 128, 64, 64], generator=gen).to(DEV)
    calls = []
    real = conv2d_mfma.instance_norm_stats
    monkeypatch.setattr(conv2d_mfma, 'instance_norm_stats', lambda t, eps: (calls.append(tuple(t.shape)), real(t, eps=eps))[1])
    with torch.no_grad():
        y = blk(x, feat)
    assert not calls, f'separate statistics passes over {calls}'
    monkeypatch.setenv('PG_FUSED_STATS', '0')
    with torch.no_grad():
        y0 = blk(x, feat)
    assert len(calls) == 2                             # (the A/B switch: x and dx each take a pass)
    assert float((y - y0).abs().max()) <= 2e-5 * float(y0.abs().max())


@pytest.mark.gpu
def test_stem7_bf16x3_repeated_full_size_launches_are_identical():
    """conv2d_stem7x3 at the size the headline runs it (N = 8, 3 -> 64 at 512^2: 256 workgroups, one per CU, double-buffered column records behind one barrier per
    row, samples by LDS-DMA with a hand-placed wait), 30 launches with other kernels in between: every result equals the first bit for bit and matches the fp32
    kernel to rounding (the kind of test that caught the F(4x4) kernel's missing barrier in round 3)."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(61)
    x = (torch.rand([8, 3, 512, 512], generator=gen) * 2 - 1).to(DEV)
    other = (torch.rand([8, 3, 512, 512], generator=gen) * 2 - 1).to(DEV)
    wt = torch.randn([64, 3, 7, 7], generator=gen).to(DEV)
    bias = torch.randn([64], generator=gen).to(DEV)
    scale = 1 / math.sqrt(147)
    packed, packed32 = conv2d_mfma.pack_stem7(wt, scale=scale), conv2d_mfma.pack_weight(wt, scale=scale)
    kw = dict(bias=bias, act='relu', gain=math.sqrt(2))
    ref = conv2d_mfma.conv2d_forward(x, packed32, 64, 7, 7, pad=(3, 3), **kw)
    first = conv2d_mfma.conv_stem7_forward(x, packed, 64, **kw)
    assert float((first - ref).abs().max()) <= 4e-6 * float(ref.abs().max())
    for it in range(30):
        if it % 3 == 1:
            conv2d_mfma.conv2d_forward(other, packed32, 64, 7, 7, pad=(3, 3), **kw)
        if it % 4 == 2:
            conv2d_mfma.conv_stem7_forward(other, packed, 64, **kw)
        y = conv2d_mfma.conv_stem7_forward(x, packed, 64, **kw)
        assert torch.equal(y, first), f'launch {it} differs from the first one: max |d| {float((y - first).abs().max()):.3e}'


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cout,h,w', [(2, 64, 48, 40, 64), (1, 32, 32, 24, 48), (2, 96, 64, 33, 36), (1, 64, 40, 64, 20)])
def test_up2_bf16x3_edge_kernel(n, cin, cout, h, w):
    """The last output column / row of the bf16-pipe form (csrc/conv2d_up2_edges.h: 32 positions x 32 couts per workgroup, K split over its four waves, fp32
    MFMA) against float64 at the fp32 kernel's bar, on ragged shapes (H + 1 and W not multiples of 32, H not a multiple of 8: the main tiles then cover row 2H;
    Cin = 32: two of the four waves have no chunk), with the dense input column the main kernel leaves behind and without it: the two must agree bit for bit."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(59)
    x = torch.randn([n, cin, h, w], generator=gen).to(DEV)
    wt = (torch.randn([cout, cin, 3, 3], generator=gen) / (3 * math.sqrt(cin))).to(DEV)
    s_in, s_out = (torch.rand([n, cin], generator=gen) + 0.5).to(DEV), (torch.rand([n, cout], generator=gen) + 0.5).to(DEV)
    packs = conv2d_mfma.pack_up2(wt)
    assert 'x3' in packs and conv2d_mfma._init().lib.pg_conv2d_up2_splitk_plan(n, cin, h, w, cout) == 1
    for mod in (True, False):
        kw = dict(in_scale=s_in, out_scale=s_out) if mod else {}
        y = conv2d_mfma.conv_up2_forward(x, packs, cout, **kw)
        y_gather = conv2d_mfma.conv_up2_forward(x, packs, cout, edge_column=False, **kw)
        y32 = conv2d_mfma.conv_up2_forward(x, packs, cout, x3=False, **kw)
        xd = (x * s_in[:, :, None, None]).double() if mod else x.double()
        ref = torch.nn.functional.conv_transpose2d(xd, wt.double().transpose(0, 1), stride=2)
        if mod:
            ref = ref * s_out[:, :, None, None].double()
        assert y.shape == ref.shape == (n, cout, 2 * h + 1, 2 * w + 1)
        assert torch.equal(y, y_gather)
        edge = lambda t: torch.cat([t[:, :, :, -1].reshape(-1), t[:, :, -1, :].reshape(-1)])
        sc = scale_of(ref)
        e_new, e_32 = float((edge(y).double() - edge(ref)).abs().max()), float((edge(y32).double() - edge(ref)).abs().max())
        assert e_new <= max(2.0 * e_32, 2e-6 * sc), f'edge error {e_new:.3e} against {e_32:.3e} of the fp32 kernel (scale {sc:.3g})'
        assert float((y.double() - ref).abs().max()) <= 4e-6 * sc


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cout,h', [(8, 128, 64, 256), (8, 512, 256, 64), (4, 512, 512, 32)])
def test_up2_bf16x3_repeated_launches_are_identical(n, cin, cout, h):
    """Full-size launches of conv2d_up2x3 (producer / consumer waves behind one barrier per chunk, counted vector-memory waits, planes and weight slabs double
    buffered), 40 in a row with other work in between: every result must equal the first one bit for bit and match the fp32-MFMA kernel to rounding -- the kind
    of test that caught the F(4x4) kernel's missing barrier in round 3 (20 % of the launches wrong under load, every small test green)."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(53)
    x = torch.randn([n, cin, h, h], generator=gen).to(DEV)
    other = torch.randn([n, cin, h, h], generator=gen).to(DEV)
    wt = (torch.randn([cout, cin, 3, 3], generator=gen) / (3 * math.sqrt(cin))).to(DEV)
    s_in, s_out = (torch.rand([n, cin], generator=gen) + 0.5).to(DEV), (torch.rand([n, cout], generator=gen) + 0.5).to(DEV)
    packs = conv2d_mfma.pack_up2(wt)
    assert 'x3' in packs
    ref = conv2d_mfma.conv_up2_forward(x, packs, cout, in_scale=s_in, out_scale=s_out, x3=False)
    first = conv2d_mfma.conv_up2_forward(x, packs, cout, in_scale=s_in, out_scale=s_out).clone()
    assert float((first - ref).abs().max()) <= 4e-6 * scale_of(ref)       # two fp32-class kernels against each other (K up to 4608); each vs float64 is tested above
    for it in range(40):
        if it % 3 == 1:
            conv2d_mfma.conv_up2_forward(other, packs, cout, in_scale=s_in, out_scale=s_out, x3=False)
        if it % 5 == 2:
            conv2d_mfma.conv_up2_forward(other, packs, cout)
        y = conv2d_mfma.conv_up2_forward(x, packs, cout, in_scale=s_in, out_scale=s_out)
        assert torch.equal(y, first), f'launch {it} differs from the first one: max |d| {float((y - first).abs().max()):.3e}'


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cin2,cout,h,w,fused', [(2, 64, 0, 64, 64, 64, True), (1, 32, 24, 40, 64, 66, True), (2, 70, 0, 96, 64, 64, False),
                                                     (1, 64, 64, 128, 80, 52, True), (1, 20, 0, 33, 64, 64, True)])
def test_streaming_1x1_conv(n, cin, cin2, cout, h, w, fused):
    """The streaming 1x1 kernel (csrc/conv2d_s1x1.h: B operand straight from global memory, weights in LDS, 16-/8-byte stores) --
    taken by pg_conv2d_forward for 32 <= Cout <= 128 and H*W >= 4096 -- against float64, with two-source input, modulation,
    demodulation, bias, lrelu, gain, clamp and residual; must agree with the tiled kernel (PG_S1X1=0 is an A/B switch of the
    library, so the comparison here is against the reference arithmetic)."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(17 * cin + cout)
    x = torch.randn([n, cin, h, w], generator=gen)
    x2 = torch.randn([n, cin2, h, w], generator=gen) if cin2 else None
    ct = cin + cin2
    wt = torch.randn([cout, ct, 1, 1], generator=gen) / np.sqrt(ct)
    kw = {}
    ref_in = torch.cat([x, x2], 1).double() if cin2 else x.double()
    if fused:
        s_in, s_out = torch.randn([n, ct], generator=gen), torch.rand([n, cout], generator=gen) + 0.5
        bias, res = torch.randn([cout], generator=gen), torch.randn([n, cout, h, w], generator=gen)
        kw = dict(in_scale=s_in.to(DEV), out_scale=s_out.to(DEV), bias=bias.to(DEV), act='lrelu', alpha=0.2, gain=1.3, clamp=1.5, residual=res.to(DEV))
        ref_in = ref_in * s_in.double()[:, :, None, None]
    y = conv2d_mfma.conv2d_forward(x.to(DEV), conv2d_mfma.pack_weight(wt.to(DEV)), cout, 1, 1, x2=x2.to(DEV) if cin2 else None, **kw)
    ref = torch.nn.functional.conv2d(ref_in, wt.double())
    if fused:
        ref = ref * s_out.double()[:, :, None, None] + bias.double()[None, :, None, None]
        ref = (torch.nn.functional.leaky_relu(ref, 0.2) * 1.3).clamp(-1.5, 1.5) + res.double()
    close(y, ref, 1e-5, 3e-6 * scale_of(ref))


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cin2,cout,h,w,fused', [(3, 64, 0, 64, 512, 256, False), (3, 64, 64, 64, 256, 256, True), (1, 32, 0, 64, 32, 32, True),
                                                      (5, 96, 32, 64, 64, 112, True), (2, 160, 0, 64, 128, 64, False), (9, 64, 0, 64, 128, 128, True),
                                                      (3, 128, 0, 128, 256, 256, True), (2, 128, 64, 128, 128, 128, False), (2, 320, 0, 256, 64, 64, True),
                                                      (1, 576, 0, 512, 32, 32, False), (5, 64, 0, 192, 64, 48, True), (2, 32, 0, 64, 64, 64, True), (1, 32, 32, 128, 128, 64, False)])
def test_streaming_1x1_conv_ring(n, cin, cin2, cout, h, w, fused):
    """The ring form of the streaming 1x1 kernel (conv1x1_stream_ring: Cout % 64 == 0 -- one pass over the pixels per 64-cout block --,
    Cin % 32 == 0, H*W % 1024 == 0, no residual; input words requested three groups ahead across tile boundaries with hand-counted
    vmcnt) against float64: several tiles, cout blocks and images per workgroup, two-source input, modulation, demodulation, bias,
    lrelu, gain, clamp; repeated, bit-identical."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(31 * cin + n)
    x = torch.randn([n, cin, h, w], generator=gen)
    x2 = torch.randn([n, cin2, h, w], generator=gen) if cin2 else None
    ct = cin + cin2
    wt = torch.randn([cout, ct, 1, 1], generator=gen) / np.sqrt(ct)
    kw = {}
    ref_in = torch.cat([x, x2], 1).double() if cin2 else x.double()
    if fused:
        s_in, s_out = torch.randn([n, ct], generator=gen), torch.rand([n, cout], generator=gen) + 0.5
        bias = torch.randn([cout], generator=gen)
        kw = dict(in_scale=s_in.to(DEV), out_scale=s_out.to(DEV), bias=bias.to(DEV), act='lrelu', alpha=0.2, gain=1.3, clamp=1.5)
        ref_in = ref_in * s_in.double()[:, :, None, None]
    pk = conv2d_mfma.pack_weight(wt.to(DEV))
    xd, x2d = x.to(DEV), (x2.to(DEV) if cin2 else None)
    y = conv2d_mfma.conv2d_forward(xd, pk, cout, 1, 1, x2=x2d, **kw)
    ref = torch.nn.functional.conv2d(ref_in, wt.double())
    if fused:
        ref = ref * s_out.double()[:, :, None, None] + bias.double()[None, :, None, None]
        ref = (torch.nn.functional.leaky_relu(ref, 0.2) * 1.3).clamp(-1.5, 1.5)
    close(y, ref, 1e-5, 3e-6 * scale_of(ref))
    for _ in range(3):
        assert torch.equal(conv2d_mfma.conv2d_forward(xd, pk, cout, 1, 1, x2=x2d, **kw), y)


@pytest.mark.gpu
def test_transposed_conv_weight_gradient_native():
    """conv_transpose2d(stride 2): its weight gradient is the weight gradient of the strided convolution dy -> x with the roles swapped,
    so conv2d_gradfix sends it to the same native kernel (exact on small integers; the route is asserted)."""
    from torch_utils.ops import conv2d_gradfix, conv2d_mfma
    gen = torch.Generator().manual_seed(77)
    x = torch.randint(-2, 3, [2, 24, 9, 11], generator=gen).float()
    w = torch.randint(-2, 3, [24, 40, 3, 3], generator=gen).float()
    calls, real, was = [0], conv2d_mfma.weight_gradient, conv2d_gradfix.native_weight_gradients
    conv2d_gradfix.native_weight_gradients = True

    def counting(*a, **k):
        out = real(*a, **k)
        calls[0] += out is not None
        return out
    conv2d_mfma.weight_gradient = counting
    try:
        xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        y = conv2d_gradfix.conv_transpose2d(xd, wd, stride=2, padding=0)
        dy = torch.randint(-2, 3, list(y.shape), generator=gen).float()
        gx, gw = torch.autograd.grad(y, [xd, wd], dy.to(DEV))
    finally:
        conv2d_mfma.weight_gradient = real
        conv2d_gradfix.native_weight_gradients = was
    assert calls[0] == 1
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    rx, rw = torch.autograd.grad(torch.nn.functional.conv_transpose2d(x64, w64, stride=2), [x64, w64], dy.double())
    assert torch.equal(gw.double().cpu(), rw)
    close(gx, rx, 1e-5, 1e-5 * scale_of(rx))


def test_flat_adam_matches_torch_adam_and_skips_untouched_parameters():
    """training/flat_adam.py (csrc/optim.hip: nan_to_num + Adam of a phase in one launch over flat buffers, round 5) against torch.nan_to_num +
    torch.optim.Adam (training_loop_fullbody.py:632-639) on the same parameters and gradients: odd sizes (the flat layout pads every parameter to 16
    bytes), NaN / +-inf gradients, three steps, and one parameter that never receives a gradient -- it must keep its value, its moments and its step
    count (`grad is None` in the reference), decided on the device from GradBucket.alive without a host read-back."""
    from training import ddp
    from training.flat_adam import FlatAdam
    gen = torch.Generator().manual_seed(5)
    shapes = [(7,), (64, 3, 3, 3), (1,), (513,), (33, 17), (5000,), (2, 2)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    lr, betas, eps = 0.002 * 4 / 5, (0.0, 0.99 ** (4 / 5)), 1e-8
    bucket = ddp.GradBucket(ps)
    opt = FlatAdam(bucket, lr, betas, eps)
    opt2 = FlatAdam(bucket, lr * 0.5, (0.9, 0.999), eps, share_params_with=opt)      # a second optimizer over the same parameters (the reference's duplicated D_parsing phase)
    ref_opt = torch.optim.Adam(ref, lr=lr, betas=betas, eps=eps)
    ref_opt2 = torch.optim.Adam(ref, lr=lr * 0.5, betas=(0.9, 0.999), eps=eps)
    assert all(p.data_ptr() == opt.flat_p[bucket.offset[i]:].data_ptr() and p.data_ptr() % 16 == 0 for i, p in enumerate(ps))
    dead = 3
    for it in range(4):
        use2 = it == 2
        if it == 3:                                   # a schedule editing param_groups (`step` reads lr / betas / eps from there, like torch.optim)
            opt.param_groups[0]['lr'] = ref_opt.param_groups[0]['lr'] = lr * 0.25
        bucket.begin()
        for i, (p, r) in enumerate(zip(ps, ref)):
            r.grad = None
            if i == dead:
                continue
            g = torch.randn(p.shape, generator=gen)
            if i == 1 and it == 1:
                g.view(-1)[5], g.view(-1)[6], g.view(-1)[7] = float('nan'), float('inf'), float('-inf')
            if bucket.gather:
                p.grad = g.to(DEV)                    # (autograd's AccumulateGrad keeps the produced tensor; finish() gathers it into the bucket)
            else:
                p.grad.copy_(g.to(DEV))
            bucket._touched_host[i] = True            # (what the post-accumulate hook records during a backward pass)
            r.grad = torch.nan_to_num(g.to(DEV), nan=0, posinf=1e5, neginf=-1e5)
        assert bucket.finish()
        before = ps[dead].detach().clone()
        (opt2 if use2 else opt).step()
        (ref_opt2 if use2 else ref_opt).step()
        assert torch.equal(ps[dead], before)
        for i, (p, r) in enumerate(zip(ps, ref)):
            assert torch.allclose(p, r, rtol=2e-6, atol=1e-7), (it, i, float((p - r).abs().max()))
            assert p._version > 0
    for i, r in enumerate(ref):
        st = opt.state_for(ps[i])
        if i == dead:
            assert float(st['step']) == 0 and float(st['exp_avg_sq'].abs().max()) == 0 and r not in ref_opt.state
            continue
        assert float(st['step']) == float(ref_opt.state[r]['step']) == 3
        assert torch.allclose(st["exp_avg_sq"], ref_opt.state[r]["exp_avg_sq"], rtol=1e-5, atol=1e-12)          # (v * b2 + (1 - b2) * g * g: contracted differently)
        assert torch.allclose(st["exp_avg"], ref_opt.state[r]["exp_avg"], rtol=1e-5, atol=1e-12)
        assert float(opt2.state_for(ps[i])['step']) == 1
    assert torch.isfinite(bucket.flat).all()           # the gradients were cleaned in place
