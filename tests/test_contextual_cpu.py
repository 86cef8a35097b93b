"""CPU tests of the contextual term (training/contextual_loss.py, torch_utils/ops/contextual_ops.py on their torch route): parity with the fixture
made by the reference's own classes (g14_contextual.npz) and with the float64 restatement (contextual_ref.py), the closed forms, the stacked-groups
call, the checkpoint reader, the term inside StyleGAN2Loss on the stub networks, and the driver's options and refusals."""

import copy
import math

import pytest
import torch

import contextual_cases as CC
import contextual_ref as CR
import stubs
import vgg_cases as VC
from detgen import det_tensor

FIX = 'g14_contextual.npz'


@pytest.fixture(scope='module')
def state_dict():
    from training.synthetic import vgg19_conv_state_dict
    return vgg19_conv_state_dict()


@pytest.fixture(scope='module')
def contextual(state_dict):
    from training.contextual_loss import ContextualLoss, VGG19ConvFeatures
    return ContextualLoss(VGG19ConvFeatures(state_dict))


# ---------------------------------------------------------------------------- the op

@pytest.mark.parametrize('case', CC.CPU_OP_CASES)
def test_cpu_route_reproduces_the_fixture_and_the_restatement(golden, case):
    """The same torch operators as the reference's class ran when the fixture was made: 1e-6 of the value / of max|dx| is left for another thread count
    or aten build.  Against float64 the route is held to twice the deviation the fixture stores for the reference's float32 run (at least 1e-6)."""
    from torch_utils.ops.contextual_ops import contextual_loss
    g = golden(FIX)
    x, y, groups = CC.op_inputs(case)
    x.requires_grad_(True)
    loss = contextual_loss(x, y, groups=groups)
    assert loss.shape == (x.shape[0],)
    dx, = torch.autograd.grad((loss * CC.op_weights(case).float()).sum(), x)
    assert float((loss.detach().double() - torch.as_tensor(g[f'{case}/loss_ref']).double()).abs().max()) <= 1e-6 * float(g[f'{case}/loss_ref'].max())
    VC.check(g, f'{case}/dx_ref', dx, 1e-6)
    want, dx64 = CR.loss_and_grad(x, y, groups=groups, weights=CC.op_weights(case))
    assert float((torch.as_tensor(g[f'{case}/loss']) - want).abs().max()) <= 1e-12                  # the stored float64 values are the restatement's
    assert float((loss.detach().double() - want).abs().max()) <= max(1e-6, 2 * float(g[f'{case}/loss_dev']))
    VC.check(g, f'{case}/dx', dx, max(1e-6, 2 * float(g[f'{case}/dx_dev'])))
    VC.check(g, f'{case}/dx', dx64, 1e-7)                                                            # (the digest stores float32 elements: 2^-24)


def test_fixture_holds_every_case_inside_its_conditions(golden):
    g = golden(FIX)
    for case in CC.OP_CASES:
        assert float(g[f'{case}/loss'].min()) >= 1e-2 and float(g[f'{case}/gap_d']) >= 1e-6 and float(g[f'{case}/gap_a']) >= 1e-5, case
        assert g[f'{case}/loss'].shape == (CC.OP_CASES[case][0],)
    for case in CC.TRUNK_CASES:
        assert float(g[f'{case}/dx_dev']) <= 1e-3
        assert min(float(g[f'{case}/relu_margin']), float(g[f'{case}/pool_margin'])) >= CC.TRUNK_MARGIN


def test_closed_forms():
    from torch_utils.ops.contextual_ops import contextual_loss
    x, y = det_tensor('cx.c1.x', [2, 1, 5, 7]).relu() * 30 + 1, det_tensor('cx.c1.y', [2, 1, 5, 7]).relu() * 30
    assert float((contextual_loss(x, y) - math.log(35)).abs().max()) <= 1e-5                        # C = 1: every A is 1 / P
    assert float((CR.contextual_loss(x, y) - math.log(35)).abs().max()) <= 1e-12
    x, y = det_tensor('cx.p1.x', [3, 21, 1, 1]).relu() * 30 + 1, det_tensor('cx.p1.y', [3, 21, 1, 1]).relu() * 30
    assert bool((contextual_loss(x, y) == 0).all()) and bool((CR.contextual_loss(x, y) == 0).all())  # P = 1: A is 1


def test_groups_equal_per_group_calls():
    from torch_utils.ops.contextual_ops import contextual_loss
    x, y, groups = CC.op_inputs('groups')
    n = y.shape[0]
    a = x.clone().requires_grad_(True)
    both = contextual_loss(a, y, groups=groups)
    da, = torch.autograd.grad(both.sum(), a)
    for k in range(groups):
        xs = x[k * n:(k + 1) * n].clone().requires_grad_(True)
        one = contextual_loss(xs, y)
        ds, = torch.autograd.grad(one.sum(), xs)
        assert torch.allclose(one, both[k * n:(k + 1) * n], rtol=1e-6, atol=0)
        assert float((ds - da[k * n:(k + 1) * n]).abs().max()) <= 1e-5 * float(ds.abs().max())
    yg = y.clone().requires_grad_(True)
    contextual_loss(x.clone().requires_grad_(True), yg, groups=groups).sum().backward()
    assert yg.grad is None                                                                          # no gradient reaches y
    for bad in (lambda: contextual_loss(x, y, groups=3), lambda: contextual_loss(x[0], y[0]), lambda: contextual_loss(x, y, h=0, groups=groups)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------- checkpoint reader and trunk

def test_load_vgg19_conv_round_trip_and_errors(state_dict, tmp_path):
    from training.contextual_loss import CONVS, load_vgg19_conv
    path = str(tmp_path / 'vgg19_conv.pth')
    torch.save(state_dict, path)
    sd = load_vgg19_conv(path)
    assert sorted(sd) == sorted(f'{name}.{leaf}' for name, _, _ in CONVS for leaf in ('weight', 'bias')) and len(sd) == 28
    assert not any(k.startswith('conv5_3') or k.startswith('conv5_4') for k in sd)                  # later layers are ignored
    for k, v in sd.items():
        assert v.dtype == torch.float32 and v.is_contiguous() and torch.equal(v, state_dict[k])
    torch.save({k: v for k, v in state_dict.items() if k != 'conv4_1.bias'}, path)
    with pytest.raises(KeyError, match=r'conv4_1\.bias'):
        load_vgg19_conv(path)
    torch.save(dict(state_dict, **{'conv2_2.weight': state_dict['conv2_2.weight'][:, :64]}), path)
    with pytest.raises(ValueError, match=r'conv2_2\.weight'):
        load_vgg19_conv(path)


def test_weights_are_buffers_not_parameters(contextual):
    assert list(contextual.parameters()) == []
    assert len(list(contextual.buffers())) == 28
    assert contextual.state_dict() == {}


@pytest.mark.parametrize('case', list(CC.TRUNK_CASES))
def test_trunk_and_combined_term_reproduce_the_fixture(golden, contextual, case):
    g = golden(FIX)
    x, y = CC.trunk_inputs(case)
    x.requires_grad_(True)
    for name, t in zip(CC.TAP_NAMES, contextual.features(x)):
        VC.check(g, f'{case}/{name}', t, max(1e-6, 2 * float(g[f'{case}/{name}_dev'])))
    loss = contextual([x], y)
    assert loss.shape == (1,)
    dx, = torch.autograd.grad(loss[0], x)
    assert abs(float(loss[0].detach()) - float(g[f'{case}/loss_ref'])) <= 1e-5 * float(g[f'{case}/loss_ref'])      # the reference's float32 run
    assert abs(float(loss[0].detach()) - float(g[f'{case}/loss'])) <= max(1e-6, 2 * float(g[f'{case}/loss_dev']))
    VC.check(g, f'{case}/dx', dx, max(1e-6, 2 * float(g[f'{case}/dx_dev'])))


def test_use_22_adds_the_fourth_level(state_dict):
    from training.contextual_loss import ContextualLoss, VGG19ConvFeatures
    from torch_utils.ops.contextual_ops import contextual_loss
    feats = VGG19ConvFeatures(state_dict)
    x, y = det_tensor('cx.u22.x', [1, 3, 32, 32], 'uniform'), det_tensor('cx.u22.y', [1, 3, 32, 32], 'uniform')
    three, four = ContextualLoss(feats)([x], y), ContextualLoss(feats, use_22=True)([x], y)
    pool = torch.nn.functional.avg_pool2d
    extra = contextual_loss(pool(feats(x)[1], 4), pool(feats(y)[1], 4)).mean()
    assert float(four[0]) == pytest.approx(float(three[0]) + float(extra), rel=1e-6)
    fx, fy = [t.double() for t in feats(x)], [t.double() for t in feats(y)]
    assert float(four[0]) == pytest.approx(float(CR.combine(fx, fy, use_22=True)[0]), rel=1e-4)


# ---------------------------------------------------------------------------- the term inside StyleGAN2Loss (stub networks, 32 x 32 images)

RES = 32


def _loss(nets, reports=None, **kw):
    from training.loss import StyleGAN2Loss
    report = None if reports is None else (lambda name, value: reports.__setitem__(name, value))
    return StyleGAN2Loss(device=torch.device('cpu'), **nets, augment_pipe=None, style_mixing_prob=0, r1_gamma=10, pl_weight=0, l1_weight=50,
                         mask_weight=1.0, report=report, **kw)


def _g_grads(nets):
    return {f'{m}.{n}': (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone())
            for m, mod in nets.items() if m.startswith('G_') for n, p in mod.named_parameters()}


def test_gmain_runs_with_the_term_and_reports_both_names(contextual):
    nets = stubs.build()
    batch = stubs.batch(res=RES)
    stubs.set_phase_trainable(nets, 'Gmain')
    grads, reports = {}, {}
    for key, kw in (('plain', dict()), ('off', dict(contextual_weight=0, contextual=contextual)), ('on', dict(contextual_weight=1, contextual=contextual))):
        stubs.zero_grads(nets)
        reports[key] = {}
        _loss(nets, reports[key], **kw).accumulate_gradients(phase='Gmain', sync=True, gain=1, **batch)
        grads[key] = _g_grads(nets)
    new = {'Loss/G/contextual', 'Loss/G/contextual_finetune'}
    assert set(reports['on']) == set(reports['plain']) | new and not new & set(reports['off'])
    # weight 0: the reports and gradients of the existing phase, bit for bit
    assert set(reports['off']) == set(reports['plain'])
    for name in reports['plain']:
        assert torch.equal(torch.as_tensor(reports['off'][name]), torch.as_tensor(reports['plain'][name])), name
        assert torch.equal(torch.as_tensor(reports['on'][name]), torch.as_tensor(reports['plain'][name])), name
    for name in grads['plain']:
        assert torch.equal(grads['off'][name], grads['plain'][name]), name

    # the term alone, through the same generator call
    stubs.zero_grads(nets)
    loss = _loss(nets)
    real_c, cat_feats = loss.G_style_encoding(batch['style_input'], batch['retain'])
    img, fine, _, _ = loss.run_G(batch['gen_z'], real_c, batch['pose'], cat_feats, batch['denorm_upper_mask'], batch['denorm_lower_mask'],
                                 batch['denorm_upper_input'], batch['denorm_lower_input'], batch['gt_parsing'])
    c_img, c_fine = contextual([img], batch['real_img'])[0], contextual([fine], batch['real_img'])[0]
    (0.5 * (c_img + c_fine)).backward()
    alone = _g_grads(nets)
    assert float(reports['on']['Loss/G/contextual'].detach()) == pytest.approx(float(c_img.detach()), rel=1e-5)
    assert float(reports['on']['Loss/G/contextual_finetune'].detach()) == pytest.approx(float(c_fine.detach()), rel=1e-5)
    assert float(c_img.detach()) > 0
    moved = 0
    for name, g_on in grads['on'].items():
        diff = g_on - grads['plain'][name]
        # float32 gradients accumulated in one backward pass against the difference of two: 1e-4 of the larger side
        bar = 1e-4 * max(float(g_on.abs().max()), float(alone[name].abs().max()), 1e-30)
        assert float((diff - alone[name]).abs().max()) <= bar, name
        moved += float(alone[name].abs().max()) > 0
    assert moved >= len(alone) // 2


def test_no_contextual_tensor_in_networks_optimizers_or_snapshots(contextual, tmp_path):
    from training.training_loop import save_snapshot
    from training.training_step import TrainingStep
    nets = stubs.build()
    before = {k: set(m.state_dict()) for k, m in nets.items()}
    G_parts = {k: v for k, v in nets.items() if k.startswith('G_')}
    step = TrainingStep(G_parts, nets['D'], nets['D_parsing'], _loss(nets, contextual_weight=1, contextual=contextual), batch_size=4)
    step.run([stubs.batch(res=RES)])
    assert {k: set(m.state_dict()) for k, m in nets.items()} == before
    ids = {id(b) for b in contextual.buffers()} | {b.data_ptr() for b in contextual.buffers()}
    net_ids = {id(p) for m in nets.values() for p in m.parameters()}
    for ph in step.phases:
        for group in ph.opt.param_groups:
            for p in group['params']:
                assert id(p) in net_ids and id(p) not in ids and p.data_ptr() not in ids
    G = torch.nn.ModuleDict(G_parts)
    path = str(tmp_path / 'snap.pt')
    save_snapshot(path, G, nets['D'], nets['D_parsing'], copy.deepcopy(G), 0.0, 4)
    snap = torch.load(path, map_location='cpu', weights_only=True)
    shapes = {tuple(b.shape) for b in contextual.buffers() if b.ndim == 4}
    for key in ('G', 'D', 'D_parsing', 'G_ema'):
        assert not any('contextual' in k.lower() or 'conv5_2' in k for k in snap[key])
        assert not any(tuple(v.shape) in shapes for v in snap[key].values())
    assert set(snap['G']) == set(G.state_dict())


# ---------------------------------------------------------------------------- driver

def test_parse_args_accepts_contextual_ckpt():
    from training.training_loop import parse_args
    a = parse_args(['--data', 'd', '--outdir', 'o', '--contextual_weight', '2', '--contextual_ckpt', 'vgg19_conv.pth'])
    assert a.contextual_weight == 2 and a.contextual_ckpt == 'vgg19_conv.pth'
    assert parse_args(['--data', 'd', '--outdir', 'o']).contextual_ckpt is None                     # no implicit default path


def test_refusals_before_any_network(contextual, tmp_path, monkeypatch):
    from training import training_loop as T
    from training.loss import StyleGAN2Loss
    with pytest.raises(NotImplementedError, match='vgg19_conv.pth'):
        StyleGAN2Loss(device=torch.device('cpu'), **stubs.build(), contextual_weight=1)
    StyleGAN2Loss(device=torch.device('cpu'), **stubs.build(), contextual_weight=1, contextual=contextual)

    def no_networks(*args, **kw):
        raise AssertionError('a network was built before the refusal')
    monkeypatch.setattr(T, 'build_networks', no_networks)
    with pytest.raises(NotImplementedError, match='contextual_ckpt'):
        T.training_loop(str(tmp_path / 'run'), str(tmp_path / 'data'), contextual_weight=1, device='cpu')
    with pytest.raises(FileNotFoundError, match='missing.pth'):
        T.training_loop(str(tmp_path / 'run'), str(tmp_path / 'data'), contextual_weight=1, contextual_ckpt=str(tmp_path / 'missing.pth'), device='cpu')
