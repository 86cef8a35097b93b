"""GPU tests of csrc/conv2d_s2x3.h: the fp32 stride-2 3x3 convolution with padding 0 (after the FIR pass of a `down = 2` layer) on the bf16 matrix pipe --
three-term operand splits, six plane products per float32 product, float32 accumulation.  Referee: float64 conv2d(stride=2) on the CPU.  Bars: the project's
own for its bf16x3 kernels (test_up2_transposed_conv_on_the_bf16_pipe_is_float32_class): error <= 2x the fp32-MFMA kernel's on the same launch and <= 2e-6 of the
output scale, repeats bit-identical."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import conv2d_mfma
    assert conv2d_mfma._init() is not None      # native code loaded, or fail loudly


def _operands(n, cin, cout, h, w):
    gen = torch.Generator().manual_seed(13 * cin + cout + 3 * h + w)
    x = torch.randn([n, cin, h, w], generator=gen)
    wt = torch.randn([cout, cin, 3, 3], generator=gen) / (3 * math.sqrt(cin))
    bias = torch.randn([cout], generator=gen)
    return x, wt, bias


def _run(x, packed, cout, **ep):
    """One stride-2 launch through conv2d_forward with its timeline entry."""
    from torch_utils.ops import conv2d_mfma
    tl = conv2d_mfma.start_timeline()
    try:
        y = conv2d_mfma.conv2d_forward(x, packed, cout, 3, 3, stride=2, **ep)
    finally:
        conv2d_mfma.stop_timeline()
    assert tl[-1][0][:4] == (3, 3, 2, 'direct'), tl[-1][0]
    return y, tl[-1][0][4]


SHAPES = [(1, 32, 32, 9, 33),            # exactly one tile, two chunks: the producers' one-ahead requests at their shortest
          (2, 48, 40, 21, 37),           # Cout % 32 != 0; ragged tile rows and columns (OH = 10, OW = 18)
          (1, 64, 128, 35, 67),          # a full cout group; OW = 33 is one column past two tiles
          (3, 64, 160, 19, 131),         # two cout groups, the second ragged
          (1, 64, 128, 129, 129),        # 64 tiles: the tile stream and its XCD order run
          (2, 128, 256, 65, 65)]         # config 3's geometry, small


@pytest.mark.parametrize('n,cin,cout,h,w', SHAPES)
def test_stride2_conv_on_the_bf16_pipe_is_float32_class(n, cin, cout, h, w, monkeypatch):
    from torch_utils.ops import conv2d_mfma
    x, wt, bias = _operands(n, cin, cout, h, w)
    pre = torch.nn.functional.conv2d(x.double(), wt.double(), stride=2)
    xd, bd = x.to(DEV), bias.to(DEV)
    packed = conv2d_mfma.pack_weight(wt.to(DEV))
    gain = math.sqrt(2)
    cases = [(dict(), pre),
             (dict(bias=bd, act='relu', gain=gain, clamp=256.0), ((pre + bias.double()[None, :, None, None]).clamp(min=0) * gain).clamp(-256, 256))]
    with torch.no_grad():
        for ep, ref in cases:
            sc = float(ref.abs().max())
            monkeypatch.setenv('PG_S2_X3', '0')
            y32, label32 = _run(xd, packed, cout, **ep)
            assert ' s2x3' not in label32, label32
            monkeypatch.setenv('PG_S2_X3', '1')
            y, label = _run(xd, packed, cout, **ep)
            assert label.endswith(' s2x3'), label                      # the launch did take the new kernel
            assert y.shape == ref.shape
            e32, e = float((y32.double().cpu() - ref).abs().max()), float((y.double().cpu() - ref).abs().max())
            print(f'N{n} {cin}->{cout} {h}x{w} {"epilogue" if ep else "plain"}: error / scale {e / sc:.3e}, fp32 kernel {e32 / sc:.3e}')
            assert e <= 2 * e32 and e <= 2e-6 * sc, (e / sc, e32 / sc)
            for _ in range(3):
                assert torch.equal(_run(xd, packed, cout, **ep)[0], y)


@pytest.mark.parametrize('case', ['cin24', 'pad1', 'residual', 'grad', 'env'])
def test_launches_the_kernel_does_not_serve_take_the_fp32_kernel(case, monkeypatch):
    """Cin = 24, padding 1, a residual, grad mode on, PG_S2_X3=0: the fp32 kernel, bit for bit."""
    from torch_utils.ops import conv2d_mfma
    n, cin, cout, h, w = 2, (24 if case == 'cin24' else 32), 40, 21, 37
    x, wt, bias = _operands(n, cin, cout, h, w)
    xd, bd = x.to(DEV), bias.to(DEV)
    packed = conv2d_mfma.pack_weight(wt.to(DEV))
    ep = dict(bias=bd, act='lrelu', alpha=0.2, gain=math.sqrt(2))
    if case == 'pad1':
        ep['pad'] = (1, 1)
    if case == 'residual':
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        ep['residual'] = torch.randn([n, cout, oh, ow], generator=torch.Generator().manual_seed(5)).to(DEV)
    monkeypatch.setenv('PG_S2_X3', '0')
    with torch.no_grad():
        want, label = _run(xd, packed, cout, **ep)
    assert ' s2x3' not in label
    if case != 'env':
        monkeypatch.setenv('PG_S2_X3', '1')
    with (torch.enable_grad() if case == 'grad' else torch.no_grad()):
        got, label = _run(xd, packed, cout, **ep)
    assert ' s2x3' not in label, label
    assert torch.equal(got, want)
    if case in ('grad', 'env'):          # the same launch does take the new kernel once the switch / the grad mode allow it
        monkeypatch.setenv('PG_S2_X3', '1')
        with torch.no_grad():
            assert _run(xd, packed, cout, **ep)[1].endswith(' s2x3')


def test_the_training_route_keeps_the_fp32_kernel(monkeypatch):
    """conv2d_gradfix.conv2d(stride=2) launches from inside an autograd Function, where grad mode is off: the launch must still be the fp32 kernel's (the training
    route's gradient-parity bars were frozen with it), bit for bit what PG_S2_X3=0 gives."""
    from torch_utils.ops import conv2d_gradfix, conv2d_mfma
    x, wt, bias = _operands(2, 32, 40, 21, 37)
    xd, wd, bd = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True), bias.to(DEV)
    outs = []
    for s2 in ('0', '1'):
        monkeypatch.setenv('PG_S2_X3', s2)
        tl = conv2d_mfma.start_timeline()
        try:
            outs.append(conv2d_gradfix.conv2d(xd, wd, bd, stride=2))
        finally:
            conv2d_mfma.stop_timeline()
        assert [t[0][:4] for t in tl] == [(3, 3, 2, 'direct')] and ' s2x3' not in tl[0][0][4], [t[0] for t in tl]
    assert outs[1].requires_grad and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('cout,cin', [(40, 48), (160, 64)])
def test_packed_planes_add_up_to_the_scaled_weight(cout, cin):
    """The stream is [cout group of 128][chunk][m-block 4][tap 9][plane 3][k-half 2][32 couts][8 channels] bf16; its three planes, re-added in float32 on the
    host, are w * scale bit for bit, and zero beyond Cout."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(cout + cin)
    wt = torch.randn([cout, cin, 3, 3], generator=gen)
    scale = 0.37
    packed = conv2d_mfma.pack_weight(wt.to(DEV), scale=scale)
    x3 = conv2d_mfma.pack_x3('s2', packed, cout, cin)
    assert conv2d_mfma.pack_x3('s2', packed, cout, cin) is x3                                    # once per pack
    groups, nchunks = (cout + 127) // 128, cin // 16
    assert x3.numel() == conv2d_mfma._init().lib.pg_conv2d_s2x3_packed_size(cout, cin) == groups * nchunks * 4 * 27 * 1024
    bits = x3.cpu().view(torch.int16).to(torch.int32).reshape(groups, nchunks, 4, 9, 3, 2, 32, 8)
    planes = (bits << 16).view(torch.float32)
    total = (planes[:, :, :, :, 0] + planes[:, :, :, :, 1]) + planes[:, :, :, :, 2]          # [group, chunk, m-block, tap, k-half, cout 32, channel 8]
    got = total.permute(0, 2, 5, 1, 4, 6, 3).reshape(groups * 128, cin, 3, 3)                # [cout, (chunk, k-half, channel), tap]
    want = wt * torch.tensor(scale, dtype=torch.float32)
    assert torch.equal(got[:cout], want)
    assert not got[cout:].any()


def _readd(x3, *shape):
    """A bf16 plane stream as float32 values of `shape` (the plane axis among them)."""
    return (x3.cpu().view(torch.int16).to(torch.int32).reshape(*shape) << 16).view(torch.float32)


@pytest.mark.parametrize('cout,cin', [(40, 48), (96, 32)])
def test_up2_packed_planes_add_up_to_the_scaled_weight(cout, cin):
    """pack_x3('up2'): [m-block of 32][chunk][tap 9][plane 3][k-half 2][32 couts][8 channels] bf16 (csrc/conv2d_up2x3.h); the three planes, re-added in float32
    on the host, are w * scale bit for bit, and zero beyond Cout."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(2 * cout + cin)
    wt = torch.randn([cout, cin, 3, 3], generator=gen)
    scale = 0.37
    packed = conv2d_mfma.pack_weight(wt.to(DEV), scale=scale)
    x3 = conv2d_mfma.pack_x3('up2', packed, cout, cin)
    mblocks, nchunks = (cout + 31) // 32, cin // 16
    assert x3.numel() == conv2d_mfma._init().lib.pg_conv2d_up2x3_packed_size(cout, cin) == mblocks * nchunks * 27 * 1024
    planes = _readd(x3, mblocks, nchunks, 9, 3, 2, 32, 8)
    total = (planes[:, :, :, 0] + planes[:, :, :, 1]) + planes[:, :, :, 2]                    # [m-block, chunk, tap, k-half, cout 32, channel 8]
    got = total.permute(0, 4, 1, 3, 5, 2).reshape(mblocks * 32, cin, 3, 3)                   # [cout, (chunk, k-half, channel), tap]
    want = wt * torch.tensor(scale, dtype=torch.float32)
    assert torch.equal(got[:cout], want)
    assert not got[cout:].any()


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('cout', [40, 96])
def test_stem7_packed_planes_add_up_to_the_scaled_weight(cout, flip):
    """pack_stem7: [m-tile of 32 couts][K step 11][plane 3][lane 64][8] bf16 with lane = (K step half, cout & 31), K group g = 2 step + half = 3 kx + ci, the 8
    values of a lane = ky 0..6 and one zero (csrc/conv2d_stem7x3.h).  The planes re-add to w * scale (flipped when asked) bit for bit; every slot the window does
    not use -- group >= 21, row 7, cout >= Cout -- is zero."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator().manual_seed(cout + int(flip))
    wt = torch.randn([cout, 3, 7, 7], generator=gen)
    scale = 0.37
    x3 = conv2d_mfma.pack_stem7(wt.to(DEV), scale=scale, flip=flip)
    mtiles = (cout + 63) // 64 * 2
    assert x3.numel() == conv2d_mfma._init().lib.pg_conv2d_stem7x3_packed_size(cout) == mtiles * 11 * 3 * 1024
    planes = _readd(x3, mtiles, 11, 3, 2, 32, 8)                                             # [m-tile, step, plane, half, cout 32, row 8]
    total = (planes[:, :, 0] + planes[:, :, 1]) + planes[:, :, 2]
    slots = total.permute(0, 3, 1, 2, 4).reshape(mtiles * 32, 22, 8)                         # [cout, group, row]
    got = slots[:, :21, :7].reshape(mtiles * 32, 7, 3, 7).permute(0, 2, 3, 1)                # [cout, (kx, ci), ky] -> [cout, ci, ky, kx]
    want = (wt.flip([2, 3]) if flip else wt) * torch.tensor(scale, dtype=torch.float32)
    assert torch.equal(got[:cout], want)
    assert not slots[cout:].any() and not slots[:, 21].any() and not slots[:, :, 7].any()


def test_split3_planes_add_up_and_keep_an_infinite_value():
    """pg_split3_bf16_cl (the guarded split of csrc/bf16x3.h) on a ragged pixel tile and a ragged channel tile: the three channels-last planes re-add to x bit for
    bit where x is finite; an infinite element keeps +-inf in the leading plane with both remainders zero."""
    from torch_utils.ops import conv2d_mfma
    from torch_utils.ops import _native as nat
    n, c, hw = 2, 24, 37
    x = torch.randn([n, c, hw], generator=torch.Generator().manual_seed(37)) * 100
    x[0, 3, 5], x[1, 17, 36] = float('inf'), float('-inf')
    xd = x.to(DEV)
    out = torch.empty([3, n, hw, c], dtype=torch.bfloat16, device=DEV)
    nat.check(conv2d_mfma._init().lib.pg_split3_bf16_cl(nat.ptr(xd), nat.ptr(out), n, c, hw, nat.stream_of(xd)), 'pg_split3_bf16_cl')
    planes = out.cpu().float().permute(0, 1, 3, 2)                                           # [3, N, C, HW]
    fin = torch.isfinite(x)
    assert int((~fin).sum()) == 2
    total = (planes[0] + planes[1]) + planes[2]
    assert torch.equal(total[fin], x[fin])
    assert torch.equal(planes[0][~fin], x[~fin])
    assert not planes[1][~fin].any() and not planes[2][~fin].any()


def test_pack_x3_is_cached_per_pack_and_kind():
    """One plane stream per (float32 pack, kind) for as long as the pack lives; the table's entries go with the pack."""
    import gc
    from torch_utils.ops import conv2d_mfma
    p = conv2d_mfma.pack_weight(torch.randn([40, 32, 3, 3], generator=torch.Generator().manual_seed(1)).to(DEV))
    up2, s2 = conv2d_mfma.pack_x3('up2', p, 40, 32), conv2d_mfma.pack_x3('s2', p, 40, 32)
    assert conv2d_mfma.pack_x3('up2', p, 40, 32) is up2 and conv2d_mfma.pack_x3('s2', p, 40, 32) is s2 and up2 is not s2
    ident = id(p)
    assert {(ident, 'up2'), (ident, 's2')} <= set(conv2d_mfma._x3_planes)
    del p
    gc.collect()
    assert not [k for k in conv2d_mfma._x3_planes if k[0] == ident]


@pytest.mark.parametrize('h,w', [(64, 64), (37, 51)])
def test_res_block_down2_on_the_new_route(h, w, monkeypatch):
    """ResBlock(64, 128, down=2), N = 2, against the float64 oracle block: the new route's error <= 2x the PG_S2_X3=0 route's, and PG_FIR_SHARED=0|1
    identical to each other under the new route."""
    from oracle import network_ref as NR
    from training import networks as PN
    from training.synthetic import fill_module_
    ref = fill_module_(NR.ResBlock(64, 128, kernel_size=3, activation='lrelu', down=2, conv_clamp=256), 's2x3.res.').eval()
    blk = PN.ResBlock(64, 128, kernel_size=3, activation='lrelu', down=2, conv_clamp=256)
    blk.load_state_dict(ref.state_dict(), strict=False)
    blk = blk.to(DEV).eval()
    x = torch.randn([2, 64, h, w], generator=torch.Generator().manual_seed(h + w))
    with torch.no_grad():
        want = ref.double()(x.double())
        xd = x.to(DEV)
        outs = {}
        for s2 in ('0', '1'):
            for shared in ('1', '0'):
                monkeypatch.setenv('PG_S2_X3', s2)
                monkeypatch.setenv('PG_FIR_SHARED', shared)
                outs[s2, shared] = blk(xd)
    assert torch.equal(outs['1', '1'], outs['1', '0'])
    assert not torch.equal(outs['1', '1'], outs['0', '1'])             # (the two kernels round differently: the switch did change the route)
    e_new, e_old = (float((outs[s2, '1'].double().cpu() - want).abs().max()) for s2 in ('1', '0'))
    print(f'ResBlock {h}x{w}: error new {e_new:.3e}, fp32 route {e_old:.3e}, scale {float(want.abs().max()):.3e}')
    assert e_new <= 2 * e_old, (e_new, e_old)


def test_repeats_at_the_benchmark_geometry():
    """N = 2, 64 -> 128 from 513^2 (the geometry the benchmark runs, 2048 tiles: eight per workgroup): five launches identical."""
    from torch_utils.ops import conv2d_mfma
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn([2, 64, 513, 513], generator=gen, device=DEV)
    wt = torch.randn([128, 64, 3, 3], generator=gen, device=DEV) / 24
    bias = torch.randn([128], generator=gen, device=DEV)
    packed = conv2d_mfma.pack_weight(wt)
    ep = dict(bias=bias, act='lrelu', alpha=0.2, gain=math.sqrt(2), clamp=256.0)
    with torch.no_grad():
        y, label = _run(x, packed, 128, **ep)
        assert label.endswith(' s2x3'), label
        assert y.shape == (2, 128, 256, 256) and bool(torch.isfinite(y).all())
        for _ in range(4):
            assert torch.equal(_run(x, packed, 128, **ep)[0], y)
