"""GPU tests of ADA's AugmentPipe on its native route (csrc/augment.hip through torch_utils/ops/augment_ops.py): parity with the fixtures
made by the reference (g11_augment.npz) and with a float64 CPU evaluation of the same composition, determinism, adjointness, R1's double
backward, no host synchronisation, and one augmented training iteration with the ADA heuristic.  Run with ``-m gpu`` on an MI355X."""

import numpy as np
import pytest
import torch

import augment_cases as AC
from detgen import det_tensor

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FIX = 'g11_augment.npz'
SHAPES = {'small': [2, 3, 64, 96], 'large': [1, 3, 256, 256]}
PCTS = (0.1, 0.5, 0.83)


@pytest.fixture(scope='module', autouse=True)
def _require_gpu_and_native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import augment_ops
    assert augment_ops._init()          # native code loaded, or fail loudly


def image(shape):
    return det_tensor('aug.x.' + 'x'.join(str(s) for s in shape), shape, 'uniform')


def pipe_of(spec, device=DEV):
    from training.augment import AugmentPipe, AUGPIPE_SPECS
    return AugmentPipe(**AUGPIPE_SPECS[spec]).requires_grad_(False).to(device)


def maxabs(a, b):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(np.asarray(b)).detach().cpu().double()).abs().max())


def matches(g, key, y, kind, tol=1e-4):
    """`y` against the fixture's digest of the reference's image `key` (augment_cases.py); raises on a miss."""
    return AC.check(y, g[key + '/px'], g[key + '/sum'], AC.STRIDE[kind], tol)


def cpu_params(params, dtype):
    G, m, C = params
    return (None if G is None else G.cpu().to(dtype), None if m is None else m.cpu(), None if C is None else C.cpu().to(dtype))


@pytest.mark.parametrize('spec', ['blit', 'geom', 'color', 'bgc'])
@pytest.mark.parametrize('pct', PCTS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_native_deterministic_cases(golden, spec, pct, shape):
    x = image(SHAPES[shape])
    pipe, pipe_cpu = pipe_of(spec), pipe_of(spec, 'cpu')
    y = pipe(x.to(DEV), debug_percentile=pct)
    matches(golden(FIX), f'det/{spec}/{pct}/{shape}', y, shape)
    # float32-class: the native route's deviation from a float64 evaluation of the same composition (same parameters) is at most
    # twice the float32 CPU route's own
    n, c, h, w = x.shape
    params = pipe_cpu.sample_params(n, h, w, torch.device('cpu'), debug_percentile=pct, num_channels=c)
    exact = pipe_cpu.apply(x.double(), cpu_params(params, torch.float64))
    f32 = pipe_cpu.apply(x, params)
    nat = pipe.apply(x.to(DEV), tuple(None if t is None else t.to(DEV) for t in params))
    dev32, devnat = maxabs(f32, exact), maxabs(nat, exact)
    assert devnat <= 2 * dev32 + 1e-6, (devnat, dev32)


@pytest.mark.parametrize('pct', PCTS)
def test_native_color_one_channel(golden, pct):
    y = pipe_of('color')(image([2, 1, 64, 96]).to(DEV), debug_percentile=pct)
    matches(golden(FIX), f'det/color/{pct}/1ch', y, '1ch')


def test_native_input_gradient(golden):
    g = golden(FIX)
    x = image(SHAPES['small']).to(DEV).requires_grad_(True)
    y = pipe_of('bgc')(x, debug_percentile=0.5)
    dx, = torch.autograd.grad(y, x, det_tensor('aug.grad.dy', y.shape).to(DEV))
    matches(g, 'grad/bgc/dx', dx, 'small')


def _bar(nat, f32, exact):
    return maxabs(nat, exact) <= 2 * maxabs(f32, exact) + 1e-6


def test_params_route_full_size():
    """Draw on the GPU (bgc, p = 0.6, 4 x 3 x 512^2), apply natively; the CPU route on the same parameters in float64 is the yardstick."""
    pipe, pipe_cpu = pipe_of('bgc'), pipe_of('bgc', 'cpu')
    pipe.p.fill_(0.6)
    x = image([4, 3, 512, 512])
    torch.manual_seed(7)
    params = pipe.sample_params(4, 512, 512, torch.device(DEV))
    y = pipe.apply(x.to(DEV), params)
    exact = pipe_cpu.apply(x.double(), cpu_params(params, torch.float64))
    f32 = pipe_cpu.apply(x, cpu_params(params, torch.float32))
    assert maxabs(y, exact) <= 1e-4 * max(1.0, float(exact.abs().max()))
    assert _bar(y, f32, exact)


def test_p0_changes_the_image_like_the_reference_composition():
    pipe, pipe_cpu = pipe_of('bgc'), pipe_of('bgc', 'cpu')
    pipe.p.zero_()
    x = image([2, 3, 128, 128])
    params = pipe.sample_params(2, 128, 128, torch.device(DEV))
    y = pipe.apply(x.to(DEV), params)
    exact = pipe_cpu.apply(x.double(), cpu_params(params, torch.float64))
    f32 = pipe_cpu.apply(x, cpu_params(params, torch.float32))
    assert maxabs(exact, x) > 1e-7                 # ~1.6e-7: the float32-rounded sym6 taps are nearly, not exactly, orthogonal
    assert not torch.equal(y.cpu(), x)
    assert _bar(y, f32, exact)


def test_forward_and_backward_are_bit_identical():
    pipe = pipe_of('bgc')
    pipe.p.fill_(1.0)
    torch.manual_seed(3)
    params = pipe.sample_params(4, 256, 256, torch.device(DEV))
    x = image([4, 3, 256, 256]).to(DEV).requires_grad_(True)
    dy = det_tensor('aug.bit.dy', [4, 3, 256, 256]).to(DEV)
    outs = []
    for _ in range(2):
        y = pipe.apply(x, params)
        dx, = torch.autograd.grad(y, x, dy)
        outs.append((y.detach().clone(), dx.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_adjointness_at_512():
    from torch_utils.ops import augment_ops
    pipe = pipe_of('bgc')
    pipe.p.fill_(1.0)
    torch.manual_seed(11)
    G, m, _ = pipe.sample_params(4, 512, 512, torch.device(DEV))
    x = image([4, 3, 512, 512]).to(DEV).requires_grad_(True)
    v = det_tensor('aug.adj.v', [4, 3, 512, 512]).to(DEV)
    y = augment_ops.geometric(x, G, m, pipe.Hz_geom)
    aty, = torch.autograd.grad(y, x, v)
    lhs, rhs = float((y.detach().double() * v.double()).sum()), float((x.detach().double() * aty.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


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


def _r1_backward(pipe, x, params, D):
    D.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)
    logits = D(pipe.apply(x, params))
    g, = torch.autograd.grad(logits.sum(), x, create_graph=True)
    g.square().sum().backward()


def _r1_weight_grads(pipe, x, params, D):
    _r1_backward(pipe, x, params, D)
    return [None if p.grad is None else p.grad.detach().cpu().double() for p in D.parameters()]   # (fc.bias: no R1 gradient)


def test_r1_double_backward_matches_float64_cpu():
    pipe, pipe_cpu = pipe_of('bgc'), pipe_of('bgc', 'cpu')
    pipe.p.fill_(0.6)
    torch.manual_seed(13)
    params = pipe.sample_params(2, 128, 128, torch.device(DEV))
    x = image([2, 3, 128, 128])
    got = _r1_weight_grads(pipe, x.to(DEV), params, SmallD().to(DEV))
    want = _r1_weight_grads(pipe_cpu, x.double(), cpu_params(params, torch.float64), SmallD().double())
    assert [a is None for a in got] == [b is None for b in want] and sum(a is not None for a in got) >= 4
    for a, b in zip(got, want):
        if b is not None:
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


def test_forward_backward_double_backward_do_not_synchronise():
    pipe = pipe_of('bgc')
    pipe.p.fill_(0.6)
    D = SmallD().to(DEV)
    x = image([2, 3, 128, 128]).to(DEV)

    def once():
        params = pipe.sample_params(2, 128, 128, torch.device(DEV))
        _r1_backward(pipe, x, params, D)
    once()                                                   # warm-up: plugin load, cached constants
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        once()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_imgfilter_is_refused_on_the_gpu():
    with pytest.raises(NotImplementedError, match='imgfilter'):
        pipe_of('bgcf')(image([1, 3, 32, 32]).to(DEV))


def test_training_iteration_with_ada():
    """One config-4 step at batch 4 with augment_pipe (bgc, p = 0.6) and ADA (interval 4): finite losses; p moves by the heuristic."""
    from training import networks
    from training.loss import StyleGAN2Loss
    from training.training_step import TrainingStep
    dev = torch.device(DEV)
    torch.manual_seed(0)
    G = networks.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                   synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256)).to(dev).train()
    dkw = dict(c_dim=512, img_resolution=512, channel_base=32768, channel_max=512, conv_clamp=256, epilogue_kwargs=dict(mbstd_group_size=4), num_fp16_res=3)
    D = networks.Discriminator(img_channels=6, **dkw).to(dev).train()
    DP = networks.Discriminator(img_channels=10, **dkw).to(dev).train()
    parts = dict(G_mapping=G.mapping, G_synthesis=G.synthesis, G_const_encoding=G.const_encoding, G_style_encoding=G.style_encoding)
    reports = []
    loss = StyleGAN2Loss(device=dev, **parts, D=D, D_parsing=DP, style_mixing_prob=0.9, r1_gamma=10, l1_weight=50, mask_weight=1.0,
                         report=lambda name, value: reports.append((name, value.detach().clone() if isinstance(value, torch.Tensor) else value)))
    pipe = pipe_of('bgc')
    step = TrainingStep(parts, D, DP, loss, batch_size=4, augment_pipe=pipe, augment_p=0.6, ada_target=0.6, ada_interval=4, ada_kimg=500)
    g = torch.Generator(device='cpu').manual_seed(100)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)
    n = 4
    batch = dict(real_img=u(n, 3, 512, 512), gen_z=torch.zeros([n, 0], device=dev), style_input=u(n, 45, 128, 128), retain=u(n, 6, 512, 512),
                 pose=u(n, 5, 512, 512), denorm_upper_input=u(n, 3, 512, 512), denorm_lower_input=u(n, 3, 512, 512),
                 denorm_upper_mask=(u(n, 1, 512, 512) > 0).float(), denorm_lower_mask=(u(n, 1, 512, 512) > 0).float(),
                 gt_parsing=torch.randint(0, 7, [n, 1, 512, 512], generator=g).float().to(dev))
    ps = []
    for _ in range(4):
        step.run([batch])
        ps.append(float(pipe.p))
    assert ps[:3] == [pytest.approx(0.6, abs=1e-7)] * 3          # p only changes on multiples of ada_interval
    for name, value in reports:
        if isinstance(value, torch.Tensor):
            assert torch.isfinite(value).all(), name
    signs = torch.cat([v.flatten() for name, v in reports if name == 'Loss/signs/real']).double()
    assert signs.numel() == 5 * n                                 # Dmain x 4 iterations + Dreg at iteration 0
    expect = max(np.float32(0.6) + np.float32(np.sign(float(signs.mean()) - 0.6) * 4 * 4 / (500 * 1000)), 0)
    assert ps[3] == pytest.approx(float(expect), abs=1e-7) and ps[3] != pytest.approx(0.6, abs=1e-7)
