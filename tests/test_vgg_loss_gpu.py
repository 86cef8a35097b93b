"""GPU tests of the VGG19 perceptual loss on its native route (csrc/vgg_loss.hip through torch_utils/ops/vgg_ops.py, the trunk's convolutions on
the package's own kernels): the pool and the L1 mean against aten, bit for bit where the arithmetic is exact; trunk, loss and input gradient
against the fixture made by the reference (g12_vgg.npz) and a float64 CPU evaluation of the same composition; determinism, no host
synchronisation, and one Gmain phase of the full-width networks with the term on.  Run with ``-m gpu`` on an MI355X."""

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import vgg_cases as VC
from detgen import det_tensor

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FIX = 'g12_vgg.npz'


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import vgg_ops
    assert vgg_ops._init()          # native code loaded, or fail loudly


def same(a, b):
    """Bit-for-bit up to the sign of zero and the payload of a NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def misaligned(t):
    """A contiguous GPU copy of `t` whose base address is 4 bytes past a 16-byte boundary (the kernels' plain path)."""
    buf = torch.empty([t.numel() + 4], dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out.copy_(t)


# ---------------------------------------------------------------------------- pool

# the first three are the odd / floor shapes (one window per plane; both extents odd; W no multiple of the 8-wide vector path); the others take the
# 16-byte path: even H, odd H (a dropped row), and enough lanes for several blocks
POOL_SHAPES = ([3, 3, 2, 2], [2, 5, 7, 9], [1, 64, 34, 38], [2, 3, 8, 16], [1, 4, 9, 24], [2, 16, 66, 72])


def pool_input(shape):
    """A ReLU'd det_tensor (many all-zero windows: ties at 0), one window of four equal positive values, one holding inf, one holding a NaN."""
    x = det_tensor('vgg.pool.x.' + 'x'.join(map(str, shape)), shape).relu()
    x[0, 0, 0:2, 0:2] = 0.75
    x[0, 1, 0:2, 0:2] = torch.tensor([[0.5, 2.0], [float('inf'), 1.0]])
    x[0, 2, 0:2, 0:2] = torch.tensor([[3.0, float('nan')], [4.0, 0.0]])
    return x


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'misaligned'])
def test_pool_matches_aten_bit_for_bit(shape, aligned):
    from torch_utils.ops import vgg_ops
    x = pool_input(shape)
    xc = x.clone().requires_grad_(True)
    yc = F.max_pool2d(xc, 2, 2)
    dy = det_tensor('vgg.pool.dy.' + 'x'.join(map(str, shape)), yc.shape)
    dxc, = torch.autograd.grad(yc, xc, dy)

    xg = (x.to(DEV) if aligned else misaligned(x)).requires_grad_(True)
    yg = vgg_ops.maxpool2x2(xg)
    dxg, = torch.autograd.grad(yg, xg, dy.to(DEV) if aligned else misaligned(dy))
    assert same(yg, yc)
    assert same(dxg, dxc)
    n, c, h, w = shape
    if h % 2:
        assert bool((dxg[:, :, h - 1, :] == 0).all())
    if w % 2:
        assert bool((dxg[:, :, :, w - 1] == 0).all())

    # every element of dx is written: the C entry on a buffer pre-filled with NaN
    dx = torch.full(shape, float('nan'), device=DEV)
    dyg = dy.to(DEV)
    st = vgg_ops._plugin.lib.pg_maxpool2x2_backward(ctypes.c_void_p(xg.data_ptr()), ctypes.c_void_p(dyg.data_ptr()), ctypes.c_void_p(dx.data_ptr()), n * c, h, w,
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    assert same(dx, dxc)
    assert not bool(dx.isnan().any())                         # (dy is finite: no NaN belongs in dx)


def test_pool_refuses_bad_input_and_double_backward():
    from torch_utils.ops import vgg_ops
    from torch_utils.ops._native import NativeOpError
    with pytest.raises(NativeOpError):
        vgg_ops.maxpool2x2(torch.zeros([1, 1, 4, 4], dtype=torch.float16, device=DEV))
    with pytest.raises(NativeOpError):
        vgg_ops.maxpool2x2(torch.zeros([1, 4, 4], device=DEV))
    with pytest.raises(NativeOpError):
        vgg_ops.maxpool2x2(torch.zeros([1, 1, 1, 4], device=DEV))
    with pytest.raises(NativeOpError):
        vgg_ops.l1_mean(torch.zeros([3, 1, 4, 4], device=DEV), torch.zeros([2, 1, 4, 4], device=DEV), groups=2)
    x = torch.rand([1, 2, 4, 4], device=DEV, requires_grad=True)
    g, = torch.autograd.grad(vgg_ops.maxpool2x2(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---------------------------------------------------------------------------- L1 mean

@pytest.mark.parametrize('shape', [[2, 64, 64, 96], [1, 5, 7, 9]], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'misaligned'])
def test_l1_mean(shape, groups, aligned):
    from torch_utils.ops import vgg_ops
    tag = 'x'.join(map(str, shape))
    xshape = [groups * shape[0]] + shape[1:]
    x, y = det_tensor(f'vgg.l1.x.{groups}.{tag}', xshape), det_tensor(f'vgg.l1.y.{tag}', shape)
    x.view(-1)[5::7] = y.repeat([groups, 1, 1, 1]).view(-1)[5::7]                      # exact zeros of x - y: sign(0) = 0
    gw = torch.tensor([0.7, 1.3][:groups])                                             # upstream gradient of the G means
    numel = y.numel()
    want = (x.double().view(groups, -1) - y.double().view(1, -1)).abs().sum(dim=1) / numel       # <= 8e5 terms per group
    want_dx = torch.cat([torch.sign(x[g * shape[0]:(g + 1) * shape[0]] - y) * (gw[g] / numel) for g in range(groups)])

    place = (lambda t: t.to(DEV)) if aligned else misaligned
    outs = []
    for _ in range(2):
        xg, yg = place(x).requires_grad_(True), place(y).requires_grad_(True)
        m = vgg_ops.l1_mean(xg, yg, groups=groups)
        (m * gw.to(DEV)).sum().backward()
        assert yg.grad is None
        outs.append((m.detach().cpu(), xg.grad.cpu()))
    m, dx = outs[0]
    assert m.shape == (groups,) and m.dtype == torch.float32
    rel = ((m.double() - want).abs() / want).max()
    print(f'l1_mean {tag} G={groups}: relative deviation from the float64 sum {float(rel):.2e}')
    assert float(rel) <= 2e-6                                  # fp32 blocked summation of <= 1e6 terms
    assert torch.equal(dx, want_dx)
    assert int((dx == 0).sum()) >= x.numel() // 7
    assert torch.equal(outs[1][0], m) and torch.equal(outs[1][1], dx)


# ---------------------------------------------------------------------------- trunk, loss, input gradient on the fixture's cases

def maxabs(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@functools.lru_cache(maxsize=None)
def _modules():
    from training.synthetic import vgg19_state_dict
    from training.vgg_loss import VGG19Features, VGGLoss
    sd = vgg19_state_dict()
    return VGGLoss(VGG19Features(sd)), VGGLoss(VGG19Features(sd)).double(), VGGLoss(VGG19Features(sd)).to(DEV)


@functools.lru_cache(maxsize=None)
def _evaluations(case):
    """{route: (taps, loss, dx)} for the float32 CPU route, the float64 CPU route and the native route, each computed once and left unchanged."""
    out = {}
    for route, V in zip(('f32', 'f64', 'native'), _modules()):
        x, y = VC.inputs(case)
        p = next(V.features.buffers())
        x, y = x.to(p.device, p.dtype).requires_grad_(True), y.to(p.device, p.dtype)
        taps = V.features(x)
        loss = V([x], y)[0]
        dx, = torch.autograd.grad(loss, x)
        out[route] = ([t.detach().cpu() for t in taps], loss.detach().cpu(), dx.cpu())
    return out


@pytest.mark.parametrize('case', list(VC.CASES))
def test_trunk_and_loss(golden, case):
    g = golden(FIX)
    ev = _evaluations(case)
    taps, loss, _ = ev['native']
    # the fixture: float32 arithmetic of another convolution algorithm.  A dot product of K <= 4608 terms carries ~ sqrt(K) * 2^-24 ~ 4e-6 of its
    # scale per layer, thirteen layers deep ~ 5e-5: the bar is 1e-4 of the tensor's maximum, the package's float32-class bar (test_augment_gpu)
    for name, t in zip(VC.TAP_NAMES, taps):
        pix, sums, scale = VC.check(g, f'{case}/{name}', t, 1e-4)
        print(f'{case}/{name}: fixture max-abs {pix:.2e}, sums {sums:.2e} (scale {scale:.2f})')
    assert abs(float(loss) - float(g[f'{case}/loss'])) <= 1e-4 * float(g[f'{case}/loss'])
    # float32-class against float64: native deviation <= 2 x the float32 CPU route's own + 1e-6 of the maximum
    for name, tn, t32, t64 in zip(VC.TAP_NAMES + ('loss',), taps + [loss], ev['f32'][0] + [ev['f32'][1]], ev['f64'][0] + [ev['f64'][1]]):
        devnat, dev32, top = maxabs(tn, t64), maxabs(t32, t64), float(t64.abs().max())
        print(f'{case}/{name}: deviation from float64: native {devnat:.3e}, float32 CPU {dev32:.3e} (max {top:.3e})')
        assert devnat <= 2 * dev32 + 1e-6 * top, (name, devnat, dev32, top)


@pytest.mark.parametrize('case', list(VC.CASES))
def test_input_gradient(golden, case):
    """dx against float64 by the network-level gradient bar (test_hip_parity): a ReLU mask, pool arg-max or sign decided the other way by a rounding
    moves dx far more than float32 noise.  The float32 CPU route is itself inside 3e-3 for these inputs (measured on the CPU: A 5.1e-7, B 5.3e-7)."""
    ev = _evaluations(case)
    top = float(ev['f64'][2].abs().max())
    relnat, rel32 = maxabs(ev['native'][2], ev['f64'][2]) / top, maxabs(ev['f32'][2], ev['f64'][2]) / top
    print(f'{case}/dx: relative deviation from float64: native {relnat:.3e}, float32 CPU {rel32:.3e}')
    assert rel32 <= 3e-3
    assert relnat <= min(max(3e-3, 10 * rel32), 3e-2)
    pix, sums, scale = VC.deviation(golden(FIX), f'{case}/dx', ev['native'][2])
    print(f'{case}/dx: fixture max-abs {pix:.2e}, sums {sums:.2e} (scale {scale:.2e})')
    assert pix <= 3e-2 * scale and sums <= 3e-2 * scale      # the same outer bar against the reference's own float32 gradient


def test_stacked_groups_equal_single_calls_and_repeat_bit_identically():
    V = _modules()[2]
    x1, y = [t.to(DEV) for t in VC.inputs('A')]
    x2 = det_tensor('vgg.x2.A', VC.CASES['A'], 'uniform').to(DEV)
    runs = []
    for _ in range(2):
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        both = V([a, b], y)
        da, db = torch.autograd.grad(both.sum(), [a, b])
        runs.append((both.detach(), da, db))
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    both, da, db = runs[0]
    for k, (x, d) in enumerate(((x1, da), (x2, db))):
        xs = x.clone().requires_grad_(True)
        one = V([xs], y)
        ds, = torch.autograd.grad(one.sum(), xs)
        # a stacked batch may tile the convolutions differently: two float32 evaluations, each held to ~2e-6 of float64 by test_trunk_and_loss
        assert abs(float(one[0].detach()) - float(both[k])) <= 4e-6 * float(one[0].detach())
        assert float((ds - d).abs().max()) <= 3e-3 * float(ds.abs().max())


@pytest.mark.parametrize('shape', [VC.CASES['B'], [1, 3, 512, 512]], ids=['B', '512'])
def test_no_vendor_convolution(shape):
    """Every convolution of the term, forward and input gradient, runs on the package's kernels: no aten convolution is dispatched (odd sizes; training size)."""
    V = _modules()[2]
    x = det_tensor('vgg.novendor.x', [2 * shape[0]] + shape[1:], 'uniform').to(DEV).requires_grad_(True)
    y = det_tensor('vgg.novendor.y', shape, 'uniform').to(DEV)
    with torch.autograd.profiler.profile() as prof:
        V([x[:shape[0]], x[shape[0]:]], y).sum().backward()
    torch.cuda.synchronize()
    names = {e.name for e in prof.function_events}
    assert not {n for n in names if 'conv' in n.lower() and n.startswith('aten::')}, names
    assert not {n for n in names if 'max_pool' in n}, names
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


def test_forward_and_backward_do_not_synchronise():
    V = _modules()[2]
    x, y = [t.to(DEV) for t in VC.inputs('A')]

    def once():
        xs = x.clone().requires_grad_(True)
        V([xs, xs * 0.5], y).sum().backward()
    once()                                                   # warm-up: plugin load, weight packs
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        once()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_forward_and_backward_capture_into_a_graph():
    """The term is capture-safe (no host read, no allocation outside torch's allocator): captured as the training step captures a phase, its replay on new
    inputs gives the eager result bit for bit."""
    from torch_utils.ops import _native as nat
    V = _modules()[2]
    x, y = [t.to(DEV) for t in VC.inputs('A')]
    x2 = det_tensor('vgg.x2.A', VC.CASES['A'], 'uniform').to(DEV)

    def once(a, b, target):
        a = a.detach().requires_grad_(True)
        loss = V([a, b], target)
        g, = torch.autograd.grad(loss.sum(), a)
        return loss.detach(), g
    want = once(x2, x, y)                                    # eager, and the first-call work
    sx, sb, sy = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(y)
    nat.invalidate_packed_weights()                          # no pack made outside the capture is reused inside it
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = once(sx, sb, sy)
    sx.copy_(x2)
    sb.copy_(x)
    sy.copy_(y)
    graph.replay()
    torch.cuda.synchronize()
    nat.invalidate_packed_weights()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---------------------------------------------------------------------------- one Gmain phase on the full-width networks

def test_gmain_phase_with_vgg_term():
    from training import training_loop as T
    from training.loss import StyleGAN2Loss
    dev = torch.device(DEV)
    n = 2
    torch.manual_seed(0)
    G, D, DP = T.build_networks(n, dev)
    keys = [set(m.state_dict()) for m in (G, D, DP)]
    D.requires_grad_(False)
    DP.requires_grad_(False)
    g = torch.Generator(device='cpu').manual_seed(100)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)
    batch = dict(real_img=u(n, 3, 512, 512), gen_z=torch.zeros([n, 0], device=dev), style_input=u(n, 45, 128, 128), retain=u(n, 6, 512, 512),
                 pose=u(n, 5, 512, 512), denorm_upper_input=u(n, 3, 512, 512), denorm_lower_input=u(n, 3, 512, 512),
                 denorm_upper_mask=(u(n, 1, 512, 512) > 0).float(), denorm_lower_mask=(u(n, 1, 512, 512) > 0).float(),
                 gt_parsing=torch.randint(0, 7, [n, 1, 512, 512], generator=g).float().to(dev))
    V = _modules()[2]

    def gmain(vgg_weight):
        reports = {}
        loss = StyleGAN2Loss(device=dev, **T.g_parts(G), D=D, D_parsing=DP, style_mixing_prob=0.9, r1_gamma=10, l1_weight=10, mask_weight=30,
                             vgg_weight=vgg_weight, vgg=V if vgg_weight else None, report=lambda name, value: reports.__setitem__(name, value))
        G.zero_grad(set_to_none=True)
        torch.manual_seed(1)                                 # the same style-mixing draw and noise in both runs
        loss.accumulate_gradients(phase='Gmain', sync=True, gain=1, **batch)
        return reports, {k: p.grad.detach().clone() for k, p in G.named_parameters() if p.grad is not None}

    rep0, grads0 = gmain(0)
    rep1, grads1 = gmain(20)
    assert 'Loss/G/vgg' not in rep0 and 'Loss/G/vgg_finetune' not in rep0
    assert set(rep1) == set(rep0) | {'Loss/G/vgg', 'Loss/G/vgg_finetune'}
    for name, value in rep1.items():
        assert bool(torch.isfinite(torch.as_tensor(value)).all()), name
    assert float(rep1['Loss/G/vgg'].detach()) > 0 and float(rep1['Loss/G/vgg_finetune'].detach()) > 0
    assert set(grads0) == set(grads1)
    assert all(bool(torch.isfinite(v).all()) for v in grads1.values())
    assert sum(not torch.equal(grads0[k], grads1[k]) for k in grads0) >= len(grads0) // 2
    assert [set(m.state_dict()) for m in (G, D, DP)] == keys
