"""GPU tests of the contextual loss on its native route (csrc/contextual.hip through torch_utils/ops/contextual_ops.py; the trunk's convolutions on
the package's own kernels): the op against the float64 restatement under the bars the fixture stores (g14_contextual.npz: twice the float32
composition's own deviation from float64, at least 1e-6), its two prepare kernels on their own, the closed forms, the saturated case, memory, determinism,
no host synchronisation, NaN-filled fresh allocations, NaN locality, the trunk and the combined term, and one Gmain phase.  Run with ``-m gpu`` on an MI355X."""

import functools
import math

import pytest
import torch

import contextual_cases as CC
import contextual_ref as CR
import vgg_cases as VC
from detgen import det_tensor
from poisoned_alloc import poisoned_empty

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FIX = 'g14_contextual.npz'


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import contextual_ops
    assert contextual_ops._init()          # native code loaded, or fail loudly


def same(a, b):
    """Bit-for-bit up to the sign of zero and the payload of a NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def misaligned(t):
    """A contiguous GPU copy of `t` whose base address is 4 bytes past a 16-byte boundary."""
    buf = torch.empty([t.numel() + 4], dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out.copy_(t)


def run(x, y, groups=1, weights=None, h=0.1):
    """(loss [S], d(sum_s w_s loss_s)/dx) of the native route; x, y already on the GPU."""
    from torch_utils.ops.contextual_ops import contextual_loss
    x = x.detach().requires_grad_(True)
    loss = contextual_loss(x, y, h=h, groups=groups)
    w = torch.ones_like(loss) if weights is None else weights.to(loss)
    dx, = torch.autograd.grad((loss * w).sum(), x)
    return loss.detach(), dx


# ---------------------------------------------------------------------------- op parity on the fixture's cases

@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'misaligned'])
@pytest.mark.parametrize('case', list(CC.OP_CASES))
def test_op_matches_float64_within_the_float32_compositions_own_error(golden, case, aligned):
    g = golden(FIX)
    x, y, groups = CC.op_inputs(case)
    place = (lambda t: t.to(DEV)) if aligned else misaligned
    loss, dx = run(place(x), place(y), groups, CC.op_weights(case))
    assert loss.shape == (x.shape[0],) and dx.shape == x.shape
    want = torch.as_tensor(g[f'{case}/loss'])
    dev = float((loss.cpu().double() - want).abs().max())
    bar = max(1e-6, 2 * float(g[f'{case}/loss_dev']))
    rel = max(1e-6, 2 * float(g[f'{case}/dx_dev']))
    pix, sums, scale = VC.deviation(g, f'{case}/dx', dx)
    print(f'{case}: loss deviation {dev:.3e} (bar {bar:.1e}); dx max-abs {pix / scale:.3e}, sums {sums / scale:.3e} of max|dx| (bar {rel:.1e})')
    assert dev <= bar
    assert pix <= rel * scale and sums <= rel * scale


# ---------------------------------------------------------------------------- the prepare kernels on their own

def test_prepare_and_its_backward_match_the_restatement():
    from torch_utils.ops import contextual_ops as ops
    s, n, c, h, w = 4, 2, 21, 5, 7
    y = 30 * torch.relu(det_tensor('cx.prep.y', [n, c, h, w]))
    x = 30 * torch.relu(det_tensor('cx.prep.x', [s, c, h, w]))
    y[0, :, 2, 3] = 2.0                      # mu is exactly 2 there ...
    x[2, :, 2, 3] = 2.0                      # ... and sample 2 (which meets y[0]) has x' == 0 at that position
    zero = (2, 2 * w + 3)
    xn, yn, rx = ops.prepare(misaligned(x), misaligned(y))
    cp = xn.shape[2]
    assert xn.shape == (s, h * w, cp) and yn.shape == (n, h * w, cp) and cp == 32 and rx.shape == (s, h * w)
    x64 = x.double().requires_grad_(True)
    xn64, yn64, rx64 = CR.prepare(x64, y.double().repeat([2, 1, 1, 1]))
    # unit vectors from a float32 sum of C squares: sqrt(C) * 2^-24 ~ 3e-7 of 1, a few operations deep
    assert float((xn[:, :, :c].cpu().double() - xn64.detach()).abs().max()) <= 2e-6
    assert float((yn[:, :, :c].cpu().double() - yn64[:n].detach()).abs().max()) <= 2e-6
    assert bool((xn[:, :, c:] == 0).all()) and bool((yn[:, :, c:] == 0).all())
    assert float((rx.cpu().double() - rx64.detach()).abs().max()) <= 2e-6 * float(rx64.detach().max())
    assert float(rx[zero]) == 0 and bool((xn[zero] == 0).all())

    dxn = det_tensor('cx.prep.dxn', [s, h * w, cp])
    dx = ops.prepare_backward(dxn.to(DEV), xn, rx, x.shape).cpu()
    keep = torch.ones([s, h * w], dtype=torch.bool)
    keep[zero] = False
    (xn64 * dxn[:, :, :c].double() * keep.unsqueeze(-1)).sum().backward()
    flat = dx.reshape(s, c, -1)
    assert bool((flat[zero[0], :, zero[1]] == 0).all())                  # a zero row where the norm is zero
    mask = keep.unsqueeze(1).expand(s, c, h * w).reshape(x.shape)
    nowhere = torch.zeros([], dtype=torch.float64)
    want = torch.where(mask, x64.grad, nowhere)                          # (autograd's own value at the zero norm is NaN)
    # dx ~ dxn / r through a float32 dot product of C terms: 1e-5 of the maximum
    assert float(torch.where(mask, dx.double() - want, nowhere).abs().max()) <= 1e-5 * float(want.abs().max())


# ---------------------------------------------------------------------------- closed forms and the saturated case

@pytest.mark.parametrize('shape', [(2, 1, 5, 7), (1, 1, 40, 33)], ids=['P35', 'P1320'])
def test_one_channel_gives_log_p(shape):
    """C = 1: y' = 0, every d is 1, every A is 1 / P: loss = log P.  S is a float32 sum of P equal terms in a fixed tree: within 1e-5."""
    x = 30 * torch.relu(det_tensor('cx.c1.x', list(shape))) + 1
    y = 30 * torch.relu(det_tensor('cx.c1.y', list(shape)))
    loss, dx = run(x.to(DEV), y.to(DEV))
    p = shape[2] * shape[3]
    assert float((loss.cpu() - math.log(p)).abs().max()) <= 1e-5
    assert bool(torch.isfinite(dx).all())


def test_one_position_gives_zero():
    x = 30 * torch.relu(det_tensor('cx.p1.x', [3, 21, 1, 1])) + 1
    y = 30 * torch.relu(det_tensor('cx.p1.y', [3, 21, 1, 1]))
    loss, dx = run(x.to(DEV), y.to(DEV))
    assert bool((loss == 0).all()) and bool(torch.isfinite(dx).all())


def test_saturated_case_stays_finite():
    """x == y: every row's minimum is ~ 0, the weights span exp(10) ... exp(-9990) -> 0; the loss is finite and >= 0, dx finite everywhere."""
    y = 30 * torch.relu(det_tensor('cx.sat.y', [2, 64, 9, 13])).to(DEV)
    loss, dx = run(y.clone(), y)
    assert bool(torch.isfinite(loss).all()) and bool((loss >= 0).all())
    assert bool(torch.isfinite(dx).all())


# ---------------------------------------------------------------------------- memory, determinism, synchronisation, fresh allocations

def test_no_p_by_p_allocation():
    x = (30 * torch.relu(det_tensor('cx.mem.x', [1, 16, 64, 64]))).to(DEV)
    y = (30 * torch.relu(det_tensor('cx.mem.y', [1, 16, 64, 64]))).to(DEV)
    run(x, y)                                                      # plugin load
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss, dx = run(x, y)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f'P = 4096: peak rise {rise / 2 ** 20:.2f} MiB (one P x P float matrix: 64 MiB)')
    assert rise < 16 * 2 ** 20
    assert bool(torch.isfinite(loss).all())


def test_two_runs_are_bit_identical():
    x, y, groups = CC.op_inputs('blocks')
    x, y = x.to(DEV), y.to(DEV)
    a, b = run(x, y, groups), run(x, y, groups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_forward_and_backward_do_not_synchronise():
    x, y, groups = CC.op_inputs('groups')
    x, y = x.to(DEV), y.to(DEV)
    run(x, y, groups)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        run(x, y, groups)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', ['small', 'edges'])
def test_nan_filled_fresh_allocations_change_nothing(case):
    x, y, groups = CC.op_inputs(case)
    x, y = x.to(DEV), y.to(DEV)
    plain = run(x, y, groups)
    with poisoned_empty():
        poisoned = run(x, y, groups)
    assert torch.equal(plain[0], poisoned[0]) and torch.equal(plain[1], poisoned[1])
    assert bool(torch.isfinite(plain[1]).all())


def test_nan_reaches_only_the_samples_that_depend_on_it():
    x, y, groups = CC.op_inputs('groups')                          # S = 4, N = 2
    x, y = x.to(DEV), y.to(DEV)
    w = CC.op_weights('groups')
    clean = run(x, y, groups, w)
    xb = x.clone()
    xb[0, 5, 3, 4] = float('nan')
    loss, dx = run(xb, y, groups, w)
    assert bool(loss[0].isnan()) and torch.equal(loss[1:], clean[0][1:]) and torch.equal(dx[1:], clean[1][1:])
    yb = y.clone()
    yb[0, 7, 2, 9] = float('nan')
    loss, dx = run(x, yb, groups, w)
    assert bool(loss[0].isnan()) and bool(loss[2].isnan())
    for s in (1, 3):
        assert torch.equal(loss[s], clean[0][s]) and torch.equal(dx[s], clean[1][s])


def test_refusals():
    from torch_utils.ops import _native as nat
    from torch_utils.ops.contextual_ops import contextual_loss
    x, y = torch.zeros([4, 8, 3, 3], device=DEV), torch.zeros([2, 8, 3, 3], device=DEV)
    for bad in (lambda: contextual_loss(x, y, groups=1), lambda: contextual_loss(x.double(), y.double(), groups=2), lambda: contextual_loss(x[0], y[0]),
                lambda: contextual_loss(x, y, h=0.0, groups=2), lambda: contextual_loss(torch.zeros([18, 8, 3, 3], device=DEV), y, groups=9),
                lambda: contextual_loss(x, y.cpu(), groups=2)):
        with pytest.raises(nat.NativeOpError):
            bad()
    loss = contextual_loss(x.requires_grad_(True) + 1, y + 2, groups=2)
    g, = torch.autograd.grad(loss.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()                                         # once_differentiable: a double backward raises


# ---------------------------------------------------------------------------- trunk and combined term against the fixture

@functools.lru_cache(maxsize=None)
def _module():
    from training.contextual_loss import ContextualLoss, VGG19ConvFeatures
    from training.synthetic import vgg19_conv_state_dict
    return ContextualLoss(VGG19ConvFeatures(vgg19_conv_state_dict())).to(DEV)


@pytest.mark.parametrize('case', list(CC.TRUNK_CASES))
def test_trunk_taps_combined_loss_and_gradient(golden, case):
    """Taps, combined loss and dx of the native route against the float64 values of the fixture, each within twice the deviation the reference's own
    float32 run has from them (at least 1e-6).  The case is one whose float64 trunk keeps every ReLU and pool decision 2e-6 of the layer's maximum
    away from flipping (contextual_cases.TRUNK_MARGIN, asserted by the generator): without that margin a gradient bar is a lottery -- on
    [2, 3, 64, 96] (margins ~ 1e-7) one unit decided the other way moved the native dx by 2.2e-3 of its maximum, against 1.2e-5 measured here."""
    g = golden(FIX)
    M = _module()
    x, y = [t.to(DEV) for t in CC.trunk_inputs(case)]
    x.requires_grad_(True)
    for name, t in zip(CC.TAP_NAMES, M.features(x)):
        bar = max(1e-6, 2 * float(g[f'{case}/{name}_dev']))
        pix, sums, scale = VC.deviation(g, f'{case}/{name}', t)
        print(f'{case}/{name}: max-abs {pix / scale:.2e}, sums {sums / scale:.2e} of the maximum (bar {bar:.1e})')
        assert pix <= bar * scale and sums <= bar * scale
    loss = M([x], y)
    assert loss.shape == (1,)
    dx, = torch.autograd.grad(loss[0], x)
    dev, bar = abs(float(loss[0].detach()) - float(g[f'{case}/loss'])), max(1e-6, 2 * float(g[f'{case}/loss_dev']))
    rel = max(1e-6, 2 * float(g[f'{case}/dx_dev']))
    pix, sums, scale = VC.deviation(g, f'{case}/dx', dx)
    print(f'{case}: loss deviation {dev:.3e} (bar {bar:.1e}); dx max-abs {pix / scale:.3e}, sums {sums / scale:.3e} of max|dx| (bar {rel:.1e})')
    assert dev <= bar
    assert pix <= rel * scale and sums <= rel * scale


# ---------------------------------------------------------------------------- one Gmain phase on narrow networks

class _Spy(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, None

    def forward(self, xs, y):
        self.seen = ([x.detach().clone() for x in xs], y.detach().clone())
        return self.inner(xs, y)


def test_gmain_phase_with_contextual_term():
    from training import training_loop as T
    from training.loss import StyleGAN2Loss
    dev = torch.device(DEV)
    n = 1
    torch.manual_seed(0)
    G, D, DP = T.build_networks(n, dev, dict(channel_base=4096, channel_max=512))
    keys = [set(m.state_dict()) for m in (G, D, DP)]
    D.requires_grad_(False)
    DP.requires_grad_(False)
    g = torch.Generator(device='cpu').manual_seed(100)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)                                  # noqa: E731
    batch = dict(real_img=u(n, 3, 512, 512), gen_z=torch.zeros([n, 0], device=dev), style_input=u(n, 45, 128, 128), retain=u(n, 6, 512, 512),
                 pose=u(n, 5, 512, 512), denorm_upper_input=u(n, 3, 512, 512), denorm_lower_input=u(n, 3, 512, 512),
                 denorm_upper_mask=(u(n, 1, 512, 512) > 0).float(), denorm_lower_mask=(u(n, 1, 512, 512) > 0).float(),
                 gt_parsing=torch.randint(0, 7, [n, 1, 512, 512], generator=g).float().to(dev))
    spy = _Spy(_module())
    weight = 0.5

    def gmain(contextual_weight):
        reports = {}
        loss = StyleGAN2Loss(device=dev, **T.g_parts(G), D=D, D_parsing=DP, style_mixing_prob=0.9, r1_gamma=10, l1_weight=10, mask_weight=30,
                             contextual_weight=contextual_weight, contextual=spy if contextual_weight else None,
                             report=lambda name, value: reports.__setitem__(name, value))
        G.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        loss.accumulate_gradients(phase='Gmain', sync=True, gain=1, **batch)
        return reports, {k: p.grad.detach().clone() for k, p in G.named_parameters() if p.grad is not None}

    rep0, grads0 = gmain(0)
    rep1, grads1 = gmain(weight)
    new = {'Loss/G/contextual', 'Loss/G/contextual_finetune'}
    assert not new & set(rep0) and set(rep1) == set(rep0) | new
    for name, value in rep1.items():
        assert bool(torch.isfinite(torch.as_tensor(value)).all()), name
    with torch.no_grad():
        direct = spy.inner(*spy.seen) * weight                     # the same images, the same stacking: the same bits
    assert torch.equal(direct[0], rep1['Loss/G/contextual'].detach()) and torch.equal(direct[1], rep1['Loss/G/contextual_finetune'].detach())
    assert float(direct[0]) > 0 and float(direct[1]) > 0
    assert set(grads0) == set(grads1)
    assert all(bool(torch.isfinite(v).all()) for v in grads1.values())
    assert sum(not torch.equal(grads0[k], grads1[k]) for k in grads0) >= len(grads0) // 2
    assert [set(m.state_dict()) for m in (G, D, DP)] == keys
