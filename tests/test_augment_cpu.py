"""CPU tests of ADA's AugmentPipe (training/augment.py): the buffers and the CPU route against fixtures made by the reference's own
AugmentPipe (tests/golden/make_golden_augment.py -> g11_augment.npz), sample_params without host reads, and the ADA heuristic of
TrainingStep on stub networks."""

import numpy as np
import pytest
import torch

import augment_cases as AC
import stubs
from detgen import det_tensor

FIX = 'g11_augment.npz'
SHAPES = {'small': [2, 3, 64, 96], 'large': [1, 3, 256, 256]}
PCTS = (0.1, 0.5, 0.83)


def image(shape):
    return det_tensor('aug.x.' + 'x'.join(str(s) for s in shape), shape, 'uniform')


def pipe_of(spec, **kw):
    from training.augment import AugmentPipe, AUGPIPE_SPECS
    return AugmentPipe(**AUGPIPE_SPECS[spec], **kw).requires_grad_(False)


def maxabs(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(np.asarray(b)).double()).abs().max())


def matches(g, key, y, kind, tol=1e-5):
    """`y` against the fixture's digest of the reference's image `key` (augment_cases.py); raises on a miss."""
    return AC.check(y, g[key + '/px'], g[key + '/sum'], AC.STRIDE[kind], tol)


def test_buffers_and_state_dict_keys_match_reference(golden):
    from training.augment import AugmentPipe
    g = golden(FIX)
    pipe = AugmentPipe()
    assert np.array_equal(pipe.Hz_geom.numpy(), g['buffers/Hz_geom'])
    assert np.array_equal(pipe.Hz_fbank.numpy(), g['buffers/Hz_fbank'])
    assert list(pipe.state_dict().keys()) == [str(k) for k in g['buffers/state_dict_keys']]


def test_specs_are_the_reference_names():
    from training.augment import AUGPIPE_SPECS
    assert list(AUGPIPE_SPECS) == ['blit', 'geom', 'color', 'filter', 'noise', 'cutout', 'bg', 'bgc', 'bgcf', 'bgcfn', 'bgcfnc']


@pytest.mark.parametrize('spec', ['blit', 'geom', 'color', 'bgc'])
@pytest.mark.parametrize('pct', PCTS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_cpu_route_deterministic_cases(golden, spec, pct, shape):
    y = pipe_of(spec)(image(SHAPES[shape]), debug_percentile=pct)
    matches(golden(FIX), f'det/{spec}/{pct}/{shape}', y, shape)


@pytest.mark.parametrize('pct', PCTS)
def test_cpu_route_color_one_channel(golden, pct):
    y = pipe_of('color')(image([2, 1, 64, 96]), debug_percentile=pct)
    matches(golden(FIX), f'det/color/{pct}/1ch', y, '1ch')


def test_color_rejects_other_channel_counts():
    with pytest.raises(ValueError):
        pipe_of('color')(torch.zeros([1, 2, 8, 8]))


@pytest.mark.parametrize('k,p', list(enumerate((0.0, 0.6, 1.0))))
def test_cpu_route_seeded_cases(golden, k, p):
    g = golden(FIX)
    pipe = pipe_of('bgc')
    pipe.p.fill_(p)
    torch.manual_seed(1234 + k)
    G_inv, margins, C = pipe.sample_params(2, 64, 96, torch.device('cpu'))
    assert np.array_equal(G_inv.numpy(), g[f'seed/bgc/{p}/G_inv'])
    assert np.array_equal(C.numpy(), g[f'seed/bgc/{p}/C'])
    torch.manual_seed(1234 + k)
    matches(g, f'seed/bgc/{p}/y', pipe(image(SHAPES['small'])), 'small')


def test_p0_still_resamples(golden):
    """At p = 0 the reference still runs the geometric block (G_inv is not I_3 by identity): sym6 up-then-down is not the identity."""
    x = image(SHAPES['small'])
    pipe = pipe_of('bgc')
    pipe.p.zero_()
    torch.manual_seed(1234)
    params = pipe.sample_params(2, 64, 96, torch.device('cpu'))
    exact = pipe.apply(x.double(), (params[0].double(), params[1], params[2].double()))
    assert maxabs(exact, x) > 1e-7             # ~1.6e-7: the float32-rounded sym6 taps are nearly, not exactly, orthogonal
    torch.manual_seed(1234)
    y = pipe(x)
    assert not torch.equal(y, x)
    matches(golden(FIX), 'seed/bgc/0.0/y', y, 'small')


def test_cpu_route_input_gradient(golden):
    g = golden(FIX)
    x = image(SHAPES['small']).requires_grad_(True)
    y = pipe_of('bgc')(x, debug_percentile=0.5)
    matches(g, 'grad/bgc/y', y, 'small')
    dx, = torch.autograd.grad(y, x, det_tensor('aug.grad.dy', y.shape))
    matches(g, 'grad/bgc/dx', dx, 'small')


def test_sample_params_reads_nothing_to_the_host(monkeypatch):
    pipe = pipe_of('bgc')
    pipe.p.fill_(0.6)
    calls = []

    def refuse(name):
        def f(self, *a, **k):
            calls.append(name)
            raise AssertionError(f'sample_params called Tensor.{name}')
        return f
    for name in ('item', 'tolist', '__int__', '__float__', '__bool__', '__index__', 'numpy'):
        monkeypatch.setattr(torch.Tensor, name, refuse(name))
    G_inv, margins, C = pipe.sample_params(4, 64, 96, torch.device('cpu'))
    monkeypatch.undo()
    assert not calls
    assert G_inv.shape == (4, 3, 3) and C.shape == (4, 4, 4) and margins.dtype == torch.int32 and margins.shape == (4,)


def test_identity_blocks_are_skipped():
    G_inv, margins, C = pipe_of('color').sample_params(2, 16, 16, torch.device('cpu'))
    assert G_inv is None and margins is None and C is not None
    G_inv, margins, C = pipe_of('blit').sample_params(2, 16, 16, torch.device('cpu'))
    assert G_inv is not None and C is None


def test_cpu_route_supports_every_stage():
    pipe = pipe_of('bgcfnc')
    pipe.p.fill_(1.0)
    torch.manual_seed(0)
    y = pipe(image([2, 3, 32, 32]))
    assert y.shape == (2, 3, 32, 32) and torch.isfinite(y).all()


# ---------------------------------------------------------------------------- ADA in the training step

class SignD(torch.nn.Module):
    """Discriminator stub whose logits have a chosen sign per sample (`signs`, set by the test before each iteration)."""
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones([]))
        self.signs = torch.ones([4])

    def forward(self, img, c, **_):
        return (self.signs * self.w)[:, None] + 0 * img.mean(dim=(1, 2, 3))[:, None]


def _loss(nets, report=None):
    from training.loss import StyleGAN2Loss
    return StyleGAN2Loss(device=torch.device('cpu'), **nets, augment_pipe=None, style_mixing_prob=0, r1_gamma=10, l1_weight=50, mask_weight=1.0,
                         report=report)


def test_ada_heuristic_follows_closed_form():
    from training.training_step import TrainingStep
    nets = stubs.build()
    nets['D'] = SignD()
    G_parts = {k: v for k, v in nets.items() if k.startswith('G_')}
    pipe = pipe_of('bgc')
    seen = []
    loss = _loss(nets, report=lambda name, value: seen.append(name))
    interval, kimg, batch, target, p0 = 4, 0.1, 4, 0.6, 0.1
    step = TrainingStep(G_parts, nets['D'], nets['D_parsing'], loss, batch_size=batch, augment_pipe=pipe, augment_p=p0, ada_target=target,
                        ada_interval=interval, ada_kimg=kimg)
    assert loss.augment_pipe is pipe
    # three windows of 4 iterations: all real logits positive (mean 1 > target: p up), mean 0.5 (< target: down), all negative (down, clamped at 0)
    windows = [[1., 1., 1., 1.], [1., 1., 1., -1.], [-1., -1., -1., -1.]]
    p = np.float32(p0)
    b = stubs.batch()
    trajectory = []
    for it in range(12):
        nets['D'].signs = torch.tensor(windows[it // interval])
        before = float(pipe.p)
        step.run([b])
        after = float(pipe.p)
        if (it + 1) % interval == 0:
            mean = float(np.mean(windows[it // interval]))
            p = np.float32(max(np.float32(p + np.float32(np.sign(mean - target) * batch * interval / (kimg * 1000))), 0))
            assert after == pytest.approx(float(p), abs=1e-7)
        else:
            assert after == before
        assert after >= 0
        trajectory.append(after)
    assert trajectory[3] > p0 and trajectory[7] < trajectory[3] and trajectory[11] == 0.0
    assert seen.count('Loss/signs/real') == 13                 # once per Dmain phase and once in Dreg (iteration 0): D, not D_parsing


def test_augment_pipe_refuses_graphs():
    from training.training_step import TrainingStep
    nets = stubs.build()
    G_parts = {k: v for k, v in nets.items() if k.startswith('G_')}
    with pytest.raises(ValueError):
        TrainingStep(G_parts, nets['D'], nets['D_parsing'], _loss(nets), batch_size=4, graphs=True, augment_pipe=pipe_of('bgc'))


def test_no_pipe_no_ada_state():
    from training.training_step import TrainingStep
    nets = stubs.build()
    G_parts = {k: v for k, v in nets.items() if k.startswith('G_')}
    loss = _loss(nets)
    report = loss.report
    step = TrainingStep(G_parts, nets['D'], nets['D_parsing'], loss, batch_size=4, ada_target=0.6)
    assert step.augment_pipe is None and step.ada_stats is None and loss.augment_pipe is None and loss.report is report
    step.run([stubs.batch()])
    assert step.ada_stats is None
