"""GPU tests of AugmentPipe's late stages on their native route (``pg_augment_late`` of csrc/augment.hip through ``augment_ops.late``):
parity with the fixtures made by the reference (g13_augment_late.npz) and with a float64 CPU evaluation on the same parameters, bit
exactness of the noise and the cutout against torch's composition, gradients, adjointness, R1's double backward, no host
synchronisation, the ``set_native_late`` switch and the C ABI's argument errors.  Late parameters are drawn by ``sample_late`` on the
CPU, where they are the reference's draws, and moved to the device.  Run with ``-m gpu`` on an MI355X."""

import ctypes

import pytest
import torch

import augment_cases as AC
import augment_late_cases as LC
from detgen import det_tensor

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FIX = 'g13_augment_late.npz'


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import augment_ops
    assert augment_ops._init()          # native code loaded, or fail loudly


def pipe_of(spec, p=1.0, device='cpu'):
    from training.augment import AugmentPipe
    pipe = AugmentPipe(**LC.SPECS[spec]).requires_grad_(False)
    pipe.p.copy_(torch.as_tensor(float(p)))
    return pipe.to(device).set_native_late(True)


def to(ts, device=None, dtype=None):
    """A parameter tuple on another device / in another float dtype (the int32 margins keep theirs)."""
    return tuple(None if t is None else t.to(device=device, dtype=dtype if t.is_floating_point() else None) for t in ts)


def draw(key):
    """The draws of the call that made `key` in the fixture, on the CPU: (x, early params, late params)."""
    kind, spec, val, shape = key.split('/')
    pct, p = (float(val), 1.0) if kind == 'det' else (None, float(val))
    return draw_spec(spec, LC.SHAPES[shape], LC.seed_of(key), p, pct)


def draw_spec(spec, shape, seed, p=1.0, pct=None, device='cpu'):
    pipe = pipe_of(spec, p, device)
    x = LC.image(shape)
    n, c, h, w = shape
    torch.manual_seed(seed)
    params = pipe.sample_params(n, h, w, torch.device(device), debug_percentile=pct, num_channels=c)
    late = pipe.sample_late(n, c, h, w, torch.device(device), debug_percentile=pct)
    return x, params, late


def apply_all(pipe, x, params, late):
    """AugmentPipe.apply on drawn parameters: the geometric and colour blocks, then the late stages."""
    from torch_utils.ops import augment_ops
    G, m, C = params
    if G is not None:
        x = augment_ops.geometric(x, G, m, pipe.Hz_geom)
    if C is not None:
        x = augment_ops.color(x, C)
    return pipe.apply_late(x, late)


def three_routes(spec, x, params, late):
    """(native on the device, float32 CPU, float64 CPU) on the same parameters."""
    nat = apply_all(pipe_of(spec, device=DEV), x.to(DEV), to(params, DEV), to(late, DEV))
    cpu = pipe_of(spec)
    f32 = apply_all(cpu, x, params, late)
    exact = apply_all(cpu, x.double(), to(params, dtype=torch.float64), to(late, dtype=torch.float64))
    return nat, f32, exact


def maxabs(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def assert_float32_class(nat, f32, exact, what=''):
    """|native - exact| <= 2 |float32 CPU - exact| + 1e-6 max(1, max|exact|)"""
    dn, d32 = maxabs(nat, exact), maxabs(f32, exact)
    bar = 2 * d32 + 1e-6 * max(1.0, float(exact.abs().max()))
    print(f'{what}: native {dn:.3e}, float32 CPU {d32:.3e}, bar {bar:.3e}, max|y| {float(exact.abs().max()):.3g}')
    assert dn <= bar, (what, dn, d32, bar)


@pytest.mark.parametrize('key', LC.det_keys() + LC.seed_keys())
def test_native_against_fixture_and_float64(golden, key):
    g = golden(FIX)
    spec, shape = key.split('/')[1], key.split('/')[3]
    x, params, late = draw(key)
    nat, f32, exact = three_routes(spec, x, params, late)
    pix, worst = AC.check(nat, g[key + '/px'], g[key + '/sum'], LC.STRIDE[shape], 1e-4)
    print(f'{key}: fixture pixels {pix:.3e}, worst sum / bar {worst:.3f}')
    assert_float32_class(nat, f32, exact, key)


@pytest.mark.parametrize('shape', list(LC.SHAPES))
@pytest.mark.parametrize('spec', ['noise', 'cutout'])
def test_noise_and_cutout_equal_torch_bit_for_bit(spec, shape):
    from torch_utils.ops import augment_ops
    cases = [(pct, 1.0) for pct in LC.DET_PCTS[spec]] + [(None, 0.6), (None, 1.0)]
    for k, (pct, p) in enumerate(cases):
        x, _, late = draw_spec(spec, LC.SHAPES[shape], 900 + k, p, pct)
        xd, lated = x.to(DEV), to(late, DEV)
        nat = pipe_of(spec, p, DEV).apply_late(xd, lated)
        assert torch.equal(nat, augment_ops.late_reference(xd, *lated)), (spec, shape, pct, p)
        assert torch.equal(nat.cpu(), augment_ops.late_reference(x, *late)), (spec, shape, pct, p)     # and the reference's CPU arithmetic
        if spec == 'cutout':                                                                          # the mask itself, at every pixel
            ones = torch.ones_like(xd)
            mask = augment_ops.late(ones, cut=lated[3])
            assert torch.equal(mask, augment_ops.late_reference(ones, None, None, None, lated[3]))
            assert set(mask.unique().tolist()) <= {0.0, 1.0}
            if pct is not None or p == 1.0:
                assert 0 < int((mask == 0).sum()) < mask.numel()


@pytest.mark.parametrize('name', list(LC.GRAD_CASES))
def test_native_input_gradient(golden, name):
    g = golden(FIX)
    spec, shape, kw, p = LC.GRAD_CASES[name]
    x, params, late = draw_spec(spec, LC.SHAPES[shape], LC.seed_of(LC.grad_key(name)), p, kw.get('debug_percentile'))
    xd = x.to(DEV).requires_grad_(True)
    y = apply_all(pipe_of(spec, p, DEV), xd, to(params, DEV), to(late, DEV))
    AC.check(y, g[LC.grad_key(name) + '/px'], g[LC.grad_key(name) + '/sum'], LC.STRIDE[shape], 1e-4)
    dx, = torch.autograd.grad(y, xd, LC.grad_dy(name, y.shape).to(DEV))
    pix, worst = AC.check(dx, g[f'grad/{name}/dx/px'], g[f'grad/{name}/dx/sum'], LC.STRIDE[shape], 1e-4)
    print(f'grad/{name}: dx pixels {pix:.3e}, worst sum / bar {worst:.3f}')


@pytest.mark.parametrize('shape', list(LC.SHAPES))
def test_linear_and_adjoint_modes_are_adjoint(shape):
    from torch_utils.ops import augment_ops as ops
    x, _, late = draw_spec('filtercut', LC.SHAPES[shape], 31, 1.0)
    taps, _, _, cut = to(late, DEV)
    assert taps is not None and cut is not None
    xd = x.to(DEV)
    v = det_tensor('aug.late.adj.v.' + shape, LC.SHAPES[shape]).to(DEV)
    fx = ops._Late.apply(xd, taps, None, None, cut, ops._LATE_LINEAR)
    ftv = ops._Late.apply(v, taps, None, None, cut, ops._LATE_ADJOINT)
    lhs, rhs = float((fx.double() * v.double()).sum()), float((xd.double() * ftv.double()).sum())
    print(f'adjointness {shape}: lhs {lhs:.9e}, rhs {rhs:.9e}')
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))
    # the affine mode's backward is the adjoint mode, whose backward is the linear mode
    xr = xd.clone().requires_grad_(True)
    noise = torch.ones_like(xd)
    y = ops.late(xr, taps, noise, torch.ones([xd.shape[0]], device=DEV), cut)
    gx, = torch.autograd.grad(y, xr, v, create_graph=True)
    assert torch.equal(gx, ftv)
    vr = v.clone().requires_grad_(True)
    ggv, = torch.autograd.grad(ops._Late.apply(vr, taps, None, None, cut, ops._LATE_ADJOINT), vr, xd)
    assert torch.equal(ggv, fx)


@pytest.mark.parametrize('shape', list(LC.SHAPES))
def test_forward_and_backward_are_bit_identical(shape):
    x, _, late = draw_spec('bgcfnc', LC.SHAPES[shape], 17, 1.0)
    pipe, lated = pipe_of('bgcfnc', device=DEV), to(late, DEV)
    xd = x.to(DEV).requires_grad_(True)
    dy = det_tensor('aug.late.bit.dy.' + shape, LC.SHAPES[shape]).to(DEV)
    outs = []
    for _ in range(2):
        y = pipe.apply_late(xd, lated)
        dx, = torch.autograd.grad(y, xd, dy)
        outs.append((y.detach().clone(), dx.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][1].abs().max()) > 0


class SmallD(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.c1 = torch.nn.Conv2d(3, 8, 3, padding=1, stride=2)
        self.c2 = torch.nn.Conv2d(8, 8, 3, padding=1, stride=2)
        self.fc = torch.nn.Linear(8, 1)

    def forward(self, x):
        sp = torch.nn.functional.softplus
        return self.fc(sp(self.c2(sp(self.c1(x)))).mean(dim=(2, 3)))


def _r1_backward(pipe, x, params, late, D):
    D.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)
    logits = D(apply_all(pipe, x, params, late))
    g, = torch.autograd.grad(logits.sum(), x, create_graph=True)
    g.square().sum().backward()


def test_r1_double_backward_matches_float64_cpu():
    x, params, late = draw_spec('bgcfnc', [2, 3, 64, 64], 13, 0.6)
    grads = []
    for pipe, xx, pp, ll, D in ((pipe_of('bgcfnc', device=DEV), x.to(DEV), to(params, DEV), to(late, DEV), SmallD().to(DEV)),
                                (pipe_of('bgcfnc'), x.double(), to(params, dtype=torch.float64), to(late, dtype=torch.float64), SmallD().double())):
        _r1_backward(pipe, xx, pp, ll, D)
        grads.append([None if q.grad is None else q.grad.detach().cpu().double() for q in D.parameters()])      # (fc.bias: no R1 gradient)
    got, want = grads
    assert [a is None for a in got] == [b is None for b in want] and sum(a is not None for a in got) >= 4
    for a, b in zip(got, want):
        if b is not None:
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            print(f'R1 weight gradient {tuple(b.shape)}: {err:.3e} of {scale:.3e}')
            assert err <= 1e-4 * scale


def test_sample_apply_backward_double_backward_do_not_synchronise():
    pipe = pipe_of('bgcfnc', 0.6, DEV)
    D = SmallD().to(DEV)
    x = LC.image([2, 3, 64, 64]).to(DEV)

    def once():
        params = pipe.sample_params(2, 64, 64, torch.device(DEV))
        late = pipe.sample_late(2, 3, 64, 64, torch.device(DEV))
        _r1_backward(pipe, x, params, late, D)
    once()                                                   # warm-up: plugin load, cached constants
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        once()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_whole_pipe_drawn_on_the_gpu():
    x, params, late = draw_spec('bgcfnc', [2, 3, 64, 96], 23, 1.0, device=DEV)
    assert all(t is not None and t.device.type == 'cuda' for t in params + late)
    nat, f32, exact = three_routes('bgcfnc', x, to(params, 'cpu'), to(late, 'cpu'))
    assert maxabs(exact, x) > 0.1
    assert_float32_class(nat, f32, exact, 'bgcfnc drawn on the GPU')
    torch.manual_seed(23)                                     # and forward() is those two draws and that application
    y = pipe_of('bgcfnc', device=DEV)(x.to(DEV))
    assert torch.equal(y, nat)


def test_switch_off_is_the_torch_composition_and_on_runs_bgcf():
    from torch_utils.ops import augment_ops
    from training.augment import AugmentPipe, AUGPIPE_SPECS
    x = LC.image(LC.SHAPES['small']).to(DEV)
    n, c, h, w = x.shape
    for spec in ('noise', 'cutout'):
        pipe = AugmentPipe(**AUGPIPE_SPECS[spec]).requires_grad_(False).to(DEV)
        assert pipe.native_late is False
        torch.manual_seed(41)
        y = pipe(x)
        torch.manual_seed(41)
        late = pipe.sample_late(n, c, h, w, x.device)
        assert torch.equal(y, augment_ops.late_reference(x, *late)) and not torch.equal(y, x)
    pipe = AugmentPipe(**AUGPIPE_SPECS['bgcf']).requires_grad_(False).to(DEV)
    with pytest.raises(NotImplementedError, match='imgfilter'):
        pipe(x)
    torch.manual_seed(43)
    y = pipe.set_native_late(True)(x)
    assert y.shape == x.shape and torch.isfinite(y).all() and not torch.equal(y, x)


def test_c_abi_argument_errors_return_before_any_launch():
    from torch_utils.ops import augment_ops
    lib = augment_ops._plugin.lib
    INVALID, UNSUPPORTED = -1, -2
    h, w = 22, 23
    x = torch.full([1, 1, h, w], 3.0, device=DEV)
    y = torch.full_like(x, 7.0)
    taps = torch.ones([1, 44], device=DEV)
    sigma = torch.ones([1], device=DEV)
    cut = torch.ones([1, 4], device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(xp, yp, tp, ntaps, noise, sg, ct, n, c, hh, ww, mode):
        return lib.pg_augment_late(xp, yp, tp, ntaps, noise, sg, ct, n, c, hh, ww, mode, None)
    assert call(None, P(y), P(taps), 43, None, None, None, 1, 1, h, w, 0) == INVALID
    assert call(P(x), None, P(taps), 43, None, None, None, 1, 1, h, w, 0) == INVALID
    for n, c, hh, ww in ((0, 1, h, w), (1, 0, h, w), (1, 1, 0, w), (1, 1, h, -1)):
        assert call(P(x), P(y), P(taps), 43, None, None, None, n, c, hh, ww, 0) == INVALID
    assert call(P(x), P(y), None, 0, P(x), None, None, 1, 1, h, w, 0) == INVALID          # noise without sigma
    assert call(P(x), P(y), None, 0, None, P(sigma), None, 1, 1, h, w, 0) == INVALID      # sigma without noise
    assert call(P(x), P(y), P(taps), 43, None, None, P(cut), 1, 1, h, w, 3) == INVALID    # unknown mode
    assert call(P(x), P(y), P(taps), 43, None, None, None, 1, 1, h, w, -1) == INVALID
    assert call(P(x), P(y), P(taps), 44, None, None, None, 1, 1, h, w, 0) == UNSUPPORTED  # even
    assert call(P(x), P(y), P(taps), 45, None, None, None, 1, 1, 64, 64, 0) == UNSUPPORTED  # more than the kernel is built for
    assert call(P(x), P(y), P(taps), 43, None, None, None, 1, 1, 21, w, 0) == UNSUPPORTED   # h = p: reflect padding needs p + 1
    assert call(P(x), P(y), P(taps), 43, None, None, None, 1, 1, h, 21, 2) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((x == 3.0).all())                                # nothing was launched
    with pytest.raises(augment_ops.nat.NativeOpError):
        augment_ops.late(x, taps=torch.ones([1, 43], device=DEV, dtype=torch.float64))
    with pytest.raises(augment_ops.nat.NativeOpError):
        augment_ops.late(x, taps=torch.ones([1, 43]))                                       # wrong device
    with pytest.raises(augment_ops.nat.NativeOpError):
        augment_ops.late(x, cut=torch.ones([2, 4], device=DEV))
    with pytest.raises(augment_ops.nat.NativeOpError):
        augment_ops.late(x, noise=torch.ones_like(x))
    with pytest.raises(augment_ops.nat.NativeOpError):
        augment_ops.late(x[:, :, :21], taps=torch.ones([1, 43], device=DEV))
