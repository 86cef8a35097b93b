"""CPU tests of AugmentPipe's late stages (imgfilter, noise, cutout; training/augment.py ``sample_late`` / ``apply_late``,
``augment_ops.late``) against fixtures made by the reference's own AugmentPipe (tests/golden/make_golden_augment_late.py ->
g13_augment_late.npz), and of the training driver's ``--augpipe`` / ``--aug fixed`` / ``--p`` options."""

import json
import math
import os

import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_late_cases as LC

FIX = 'g13_augment_late.npz'
TOL = 1e-5


def pipe_of(key_or_spec, p=1.0):
    from training.augment import AugmentPipe
    pipe = AugmentPipe(**LC.SPECS[key_or_spec]).requires_grad_(False)
    pipe.p.copy_(torch.as_tensor(float(p)))
    return pipe


def run_case(key, pipe=None, x=None):
    """The call that made `key` in the fixture: (y, the generator's next draw)."""
    kind, spec, val, shape = key.split('/')
    x = LC.image(LC.SHAPES[shape]) if x is None else x
    torch.manual_seed(LC.seed_of(key))
    if kind == 'det':
        y = (pipe or pipe_of(spec))(x, debug_percentile=float(val))
    else:
        y = (pipe or pipe_of(spec, float(val)))(x)
    return y, torch.rand(1)


def matches(g, key, y, tol=TOL):
    return AC.check(y, g[key + '/px'], g[key + '/sum'], LC.STRIDE[key.split('/')[-1]], tol)


def test_specs_are_the_drivers():
    from training.augment import AUGPIPE_SPECS
    for spec in ('filter', 'noise', 'cutout', 'bgcfnc'):
        assert LC.SPECS[spec] == AUGPIPE_SPECS[spec]


@pytest.mark.parametrize('key', LC.det_keys() + LC.seed_keys())
def test_cpu_route_matches_reference_and_its_random_stream(golden, key):
    g = golden(FIX)
    y, nxt = run_case(key)
    matches(g, key, y)
    assert torch.equal(nxt, torch.as_tensor(g[key + '/next']))


@pytest.mark.parametrize('key', ['det/bgcfnc/0.83/small', 'seed/bgcfnc/0.6/small', 'seed/filter/1.0/tiles', 'det/noise/0.5/min', 'det/cutout/0.1/tiles'])
def test_sample_late_and_apply_late_equal_forward(golden, key):
    kind, spec, val, shape = key.split('/')
    x = LC.image(LC.SHAPES[shape])
    y, nxt = run_case(key)
    pct = float(val) if kind == 'det' else None
    pipe = pipe_of(spec, 1.0 if kind == 'det' else float(val))
    n, c, h, w = x.shape
    torch.manual_seed(LC.seed_of(key))
    params = pipe.sample_params(n, h, w, x.device, debug_percentile=pct, num_channels=c)
    z = x
    from torch_utils.ops import augment_ops
    if params[0] is not None:
        z = augment_ops.geometric(z, params[0], params[1], pipe.Hz_geom)
    if params[2] is not None:
        z = augment_ops.color(z, params[2])
    late = pipe.sample_late(n, c, h, w, x.device, debug_percentile=pct)
    z = pipe.apply_late(z, late)
    assert torch.equal(z, y)
    assert torch.equal(torch.rand(1), nxt) and torch.equal(nxt, torch.as_tensor(golden(FIX)[key + '/next']))
    taps, noise, sigma, cut = late
    on = LC.SPECS[spec]
    assert (taps is not None) == ('imgfilter' in on) and (noise is not None) == (sigma is not None) == ('noise' in on) and (cut is not None) == ('cutout' in on)
    if taps is not None:
        assert taps.shape == (n, 43) and taps.dtype == torch.float32
    if noise is not None:
        assert noise.shape == x.shape and sigma.shape == (n,)
    if cut is not None:
        assert cut.shape == (n, 4)


@pytest.mark.parametrize('name', list(LC.GRAD_CASES))
def test_input_gradient_matches_reference(golden, name):
    g = golden(FIX)
    spec, shape, kw, p = LC.GRAD_CASES[name]
    key = LC.grad_key(name)
    x = LC.image(LC.SHAPES[shape]).requires_grad_(True)
    torch.manual_seed(LC.seed_of(key))
    y = pipe_of(spec, p)(x, **kw)
    matches(g, key, y)
    dx, = torch.autograd.grad(y, x, LC.grad_dy(name, y.shape))
    AC.check(dx, g[f'grad/{name}/dx/px'], g[f'grad/{name}/dx/sum'], LC.STRIDE[shape], TOL)


def test_late_op_is_differentiable_twice_in_float64():
    from torch_utils.ops import augment_ops
    pipe = pipe_of('bgcfnc')
    torch.manual_seed(3)
    taps, noise, sigma, cut = pipe.sample_late(1, 2, 24, 25, torch.device('cpu'))
    x = LC.image([1, 2, 24, 25]).double().requires_grad_(True)
    y = augment_ops.late(x, taps, noise, sigma, cut)
    assert y.dtype == torch.float64
    gx, = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    ggx, = torch.autograd.grad(gx.square().sum(), x)
    assert torch.isfinite(ggx).all() and float(ggx.abs().max()) > 0
    assert not any(t.requires_grad for t in (taps, noise, sigma, cut))


def test_set_native_late_changes_no_key_and_no_cpu_result():
    from training.augment import AugmentPipe
    pipe = pipe_of('bgcfnc')
    assert pipe.native_late is False and 'native_late' not in AugmentPipe.__init__.__code__.co_varnames
    keys = list(pipe.state_dict().keys())
    y0, n0 = run_case('seed/bgcfnc/0.6/small', pipe=pipe_of('bgcfnc', 0.6))
    assert pipe.set_native_late(True) is pipe and pipe.native_late is True
    assert list(pipe.state_dict().keys()) == keys == ['p', 'Hz_geom', 'Hz_fbank']
    y1, n1 = run_case('seed/bgcfnc/0.6/small', pipe=pipe_of('bgcfnc', 0.6).set_native_late(True))
    assert torch.equal(y0, y1) and torch.equal(n0, n1)
    assert pipe.set_native_late(False).native_late is False


# ---------------------------------------------------------------------------- the training driver's options

BASE = ['--data', 'nowhere', '--outdir', 'nowhere']


def test_parse_args_defaults_and_choices():
    from training import training_loop as T
    from training.augment import AUGPIPE_SPECS
    a = T.parse_args(BASE)
    assert (a.aug, a.p, a.augpipe, a.target) == ('ada', None, 'bgc', 0.6)
    a = T.parse_args(BASE + ['--aug', 'fixed', '--p', '0.25', '--augpipe', 'bgcfnc'])
    assert (a.aug, a.p, a.augpipe) == ('fixed', 0.25, 'bgcfnc')
    for name in AUGPIPE_SPECS:
        assert T.parse_args(BASE + ['--augpipe', name]).augpipe == name
    with pytest.raises(SystemExit):
        T.parse_args(BASE + ['--augpipe', 'everything'])


RULES = [
    (dict(aug='fixed'), ['--aug', 'fixed'], '--aug=fixed requires specifying --p'),
    (dict(aug='ada', p=0.5), ['--p', '0.5'], '--p can only be specified with --aug=fixed'),
    (dict(aug='noaug', p=0.5), ['--aug', 'noaug', '--p', '0.5'], '--p can only be specified with --aug=fixed'),
    (dict(aug='fixed', p=1.5), ['--aug', 'fixed', '--p', '1.5'], '--p must be between 0 and 1'),
    (dict(aug='fixed', p=-0.1), ['--aug', 'fixed', '--p', '-0.1'], '--p must be between 0 and 1'),
    (dict(aug='noaug', augpipe='bgcfnc'), ['--aug', 'noaug', '--augpipe', 'bgcfnc'], '--augpipe cannot be specified with --aug=noaug'),
]


@pytest.mark.parametrize('kw,argv,text', RULES)
def test_option_rules_raise_before_anything_is_built(tmp_path, monkeypatch, kw, argv, text):
    from training import training_loop as T

    def no_networks(*a, **k):
        raise AssertionError('networks were built before the options were checked')
    monkeypatch.setattr(T, 'build_networks', no_networks)
    with pytest.raises(ValueError) as e:
        T.training_loop(str(tmp_path / 'run'), str(tmp_path / 'nowhere'), device='cpu', **kw)
    assert str(e.value) == text
    with pytest.raises(SystemExit) as e:
        T.main(['--data', str(tmp_path / 'nowhere'), '--outdir', str(tmp_path / 'run'), '--device', 'cpu'] + argv)
    assert str(e.value) == text
    assert not os.path.exists(str(tmp_path / 'run'))


def test_driver_runs_a_fixed_bgcfnc_pipe(tmp_path):
    from training import training_loop as T
    from test_train_loader import write_train_root
    from test_snapshot_grid_cpu import WIDTH
    root = write_train_root(str(tmp_path / 'train'))
    run = str(tmp_path / 'run')
    step = T.training_loop(run, root, batch=1, batch_gpu=1, kimg=0.001, tick=0.001, snap=None, image_snap=0, workers=0, device='cpu', width=WIDTH,
                           aug='fixed', p=0.5, augpipe='bgcfnc', dataset_kwargs=dict(shuffle=False))
    pipe = step.augment_pipe
    assert pipe is not None and pipe.imgfilter == 1 and pipe.noise == 1 and pipe.cutout == 1 and pipe.native_late is False     # a CPU run
    assert step.ada_target is None
    lines = [json.loads(line) for line in open(os.path.join(run, 'stats.jsonl'))]
    assert lines
    for line in lines:
        assert line['Progress/augment'] == 0.5
        losses = {k: v for k, v in line.items() if k.startswith('Loss/')}
        assert losses and all(math.isfinite(v) for v in losses.values()), line
