"""CPU tests of the VGG19 perceptual term (training/vgg_loss.py, torch_utils/ops/vgg_ops.py on their aten route): the checkpoint reader, parity with
the fixture made by the reference's own VGGLoss (g12_vgg.npz), the stacked-groups call, the term inside StyleGAN2Loss on the stub networks of
test_training_host.py, and the driver's options and refusals."""

import copy
import os

import pytest
import torch

import stubs
import vgg_cases as VC
from detgen import det_tensor

FIX = 'g12_vgg.npz'


@pytest.fixture(scope='module')
def state_dict():
    from training.synthetic import vgg19_state_dict
    return vgg19_state_dict(classifier=True)


@pytest.fixture(scope='module')
def vgg(state_dict):
    from training.vgg_loss import VGG19Features, VGGLoss
    return VGGLoss(VGG19Features(state_dict))


# ---------------------------------------------------------------------------- checkpoint reader

def test_load_vgg19_round_trip(state_dict, tmp_path):
    from training.vgg_loss import CONVS, load_vgg19
    path = str(tmp_path / 'vgg19.pth')
    torch.save(state_dict, path)
    assert os.path.getsize(path) < 100 * 2 ** 20                  # the zero classifier entries are zero-stride views: a checkpoint of the convolutions' size
    sd = load_vgg19(path)
    assert sorted(sd) == sorted(f'features.{i}.{leaf}' for i, _, _ in CONVS for leaf in ('weight', 'bias')) and len(sd) == 26
    assert not any(k.startswith('classifier') or k.startswith('features.3') for k in sd)      # features.30+ and classifier.* are ignored
    for k, v in sd.items():
        assert v.dtype == torch.float32 and v.is_contiguous() and torch.equal(v, state_dict[k])
    assert sd['features.0.weight'].shape == (64, 3, 3, 3) and sd['features.28.weight'].shape == (512, 512, 3, 3)


def test_load_vgg19_names_what_is_wrong(state_dict, tmp_path):
    from training.vgg_loss import load_vgg19
    path = str(tmp_path / 'bad.pth')
    sd = {k: v for k, v in state_dict.items() if k.startswith('features.')}
    torch.save({k: v for k, v in sd.items() if k != 'features.19.bias'}, path)
    with pytest.raises(KeyError, match=r'features\.19\.bias'):
        load_vgg19(path)
    torch.save(dict(sd, **{'features.7.weight': sd['features.7.weight'][:, :64]}), path)
    with pytest.raises(ValueError, match=r'features\.7\.weight'):
        load_vgg19(path)


def test_weights_are_buffers_not_parameters(vgg):
    assert list(vgg.parameters()) == []
    assert len(list(vgg.buffers())) == 26
    assert vgg.state_dict() == {}                                 # nothing of it enters a snapshot, even of a module that owned it


# ---------------------------------------------------------------------------- parity with the reference's VGGLoss

@pytest.mark.parametrize('case', list(VC.CASES))
def test_cpu_route_reproduces_the_fixture(golden, vgg, case):
    """The same aten operators on the same weights as the reference's classes ran when the fixture was made.  Measured where it was made: taps, loss and
    dx all deviate by exactly 0.  The bar leaves 1e-6 of the tensor's maximum for another thread count or aten build (a float32 convolution summed in
    another order)."""
    g = golden(FIX)
    x, y = VC.inputs(case)
    x.requires_grad_(True)
    for name, t in zip(VC.TAP_NAMES, vgg.features(x)):
        pix, sums, scale = VC.check(g, f'{case}/{name}', t, 1e-6)
        print(f'{case}/{name}: max-abs {pix:.2e}, sums {sums:.2e} (scale {scale:.2f})')
    loss = vgg([x], y)
    assert loss.shape == (1,)
    dx, = torch.autograd.grad(loss[0], x)
    rel = abs(float(loss[0].detach()) - float(g[f'{case}/loss'])) / float(g[f'{case}/loss'])
    pix, sums, scale = VC.check(g, f'{case}/dx', dx, 1e-6)
    print(f'{case}: loss relative {rel:.2e}; dx max-abs {pix:.2e}, sums {sums:.2e} (scale {scale:.2e})')
    assert rel <= 1e-6


def test_stacked_groups_equal_single_calls(vgg):
    x1, y = VC.inputs('A')
    x2 = det_tensor('vgg.x2.A', VC.CASES['A'], 'uniform')
    a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    both = vgg([a, b], y)
    assert both.shape == (2,)
    da, db = torch.autograd.grad(both[0] * 0.7 + both[1] * 1.3, [a, b])
    for k, (x, d, w) in enumerate(((x1, da, 0.7), (x2, db, 1.3))):
        xs = x.clone().requires_grad_(True)
        one = vgg([xs], y)
        ds, = torch.autograd.grad(one[0] * w, xs)
        # float32 on both sides; a batch of another size may be summed in another order: 1e-6 of the value, 1e-5 of the gradient's maximum
        assert abs(float(one[0].detach()) - float(both[k].detach())) <= 1e-6 * float(one[0].detach())
        assert float((ds - d).abs().max()) <= 1e-5 * float(ds.abs().max())
    assert vgg(x1, y).shape == (1,)                               # a bare tensor is one group
    with pytest.raises(ValueError):
        vgg([x1[:, :, :32]], y)


def test_cpu_ops_follow_aten():
    from torch_utils.ops import vgg_ops
    x = det_tensor('vgg.cpu.pool', [2, 3, 7, 9]).requires_grad_(True)
    y = vgg_ops.maxpool2x2(x)
    assert torch.equal(y, torch.nn.functional.max_pool2d(x, 2, 2)) and y.shape == (2, 3, 3, 4)
    a, b = det_tensor('vgg.cpu.a', [4, 3, 5, 6]).requires_grad_(True), det_tensor('vgg.cpu.b', [2, 3, 5, 6]).requires_grad_(True)
    m = vgg_ops.l1_mean(a, b, groups=2)
    want = torch.stack([(a[:2] - b).abs().mean(), (a[2:] - b).abs().mean()])
    assert m.shape == (2,) and torch.allclose(m, want, rtol=1e-6, atol=0)
    m.sum().backward()
    assert b.grad is None                                         # the target's features are detached
    assert torch.equal(a.grad, torch.cat([torch.sign(a[:2] - b), torch.sign(a[2:] - b)]).detach() / b.numel())
    with pytest.raises(ValueError):
        vgg_ops.l1_mean(a, b, groups=3)


# ---------------------------------------------------------------------------- the term inside StyleGAN2Loss (stub networks, 32 x 32 images)

RES = 32


def _loss(nets, reports=None, **kw):
    from training.loss import StyleGAN2Loss
    report = None if reports is None else (lambda name, value: reports.__setitem__(name, value))
    return StyleGAN2Loss(device=torch.device('cpu'), **nets, augment_pipe=None, style_mixing_prob=0, r1_gamma=10, pl_weight=0, l1_weight=50,
                         contextual_weight=0, mask_weight=1.0, report=report, **kw)


def _g_grads(nets):
    return {f'{m}.{n}': (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone())
            for m, mod in nets.items() if m.startswith('G_') for n, p in mod.named_parameters()}


def test_gmain_adds_exactly_the_weighted_term(vgg):
    w = 20.0
    nets = stubs.build()
    batch = stubs.batch(res=RES)
    stubs.set_phase_trainable(nets, 'Gmain')
    grads, reports = {}, {}
    for key, kw in (('off', dict(vgg_weight=0)), ('on', dict(vgg_weight=w, vgg=vgg))):
        stubs.zero_grads(nets)
        reports[key] = {}
        _loss(nets, reports[key], **kw).accumulate_gradients(phase='Gmain', sync=True, gain=1, **batch)
        grads[key] = _g_grads(nets)
    assert 'Loss/G/vgg' not in reports['off'] and 'Loss/G/vgg_finetune' not in reports['off']
    assert set(reports['on']) == set(reports['off']) | {'Loss/G/vgg', 'Loss/G/vgg_finetune'}
    for name in reports['off']:                                   # the other reports do not move
        assert torch.equal(torch.as_tensor(reports['on'][name]), torch.as_tensor(reports['off'][name])), name

    # the term alone, through the same generator call
    stubs.zero_grads(nets)
    loss = _loss(nets, vgg_weight=0)
    real_c, cat_feats = loss.G_style_encoding(batch['style_input'], batch['retain'])
    img, fine, _, _ = loss.run_G(batch['gen_z'], real_c, batch['pose'], cat_feats, batch['denorm_upper_mask'], batch['denorm_lower_mask'],
                                 batch['denorm_upper_input'], batch['denorm_lower_input'], batch['gt_parsing'])
    v_img, v_fine = vgg([img], batch['real_img'])[0], vgg([fine], batch['real_img'])[0]
    (w / 2 * (v_img + v_fine)).backward()
    alone = _g_grads(nets)
    assert float(reports['on']['Loss/G/vgg'].detach()) == pytest.approx(w * float(v_img.detach()), rel=1e-6)
    assert float(reports['on']['Loss/G/vgg_finetune'].detach()) == pytest.approx(w * float(v_fine.detach()), rel=1e-6)
    moved = 0
    for name, g_on in grads['on'].items():
        diff = g_on - grads['off'][name]
        # float32 gradients accumulated in one backward pass against the difference of two: 1e-5 of the larger side
        bar = 1e-5 * max(float(g_on.abs().max()), float(alone[name].abs().max()), 1e-30)
        assert float((diff - alone[name]).abs().max()) <= bar, name
        moved += float(alone[name].abs().max()) > 0
    assert moved >= len(alone) // 2                               # the term reaches the generator's parameters


def test_no_vgg_tensor_in_networks_optimizers_or_snapshots(vgg, tmp_path):
    from training.training_loop import save_snapshot
    from training.training_step import TrainingStep
    nets = stubs.build()
    before = {k: set(m.state_dict()) for k, m in nets.items()}
    G_parts = {k: v for k, v in nets.items() if k.startswith('G_')}
    step = TrainingStep(G_parts, nets['D'], nets['D_parsing'], _loss(nets, vgg_weight=20, vgg=vgg), batch_size=4)
    step.run([stubs.batch(res=RES)])
    assert {k: set(m.state_dict()) for k, m in nets.items()} == before
    vgg_ids = {id(b) for b in vgg.buffers()} | {b.data_ptr() for b in vgg.buffers()}
    net_ids = {id(p) for m in nets.values() for p in m.parameters()}
    for ph in step.phases:
        for group in ph.opt.param_groups:
            for p in group['params']:
                assert id(p) in net_ids and id(p) not in vgg_ids and p.data_ptr() not in vgg_ids
    G = torch.nn.ModuleDict(G_parts)
    path = str(tmp_path / 'snap.pt')
    save_snapshot(path, G, nets['D'], nets['D_parsing'], copy.deepcopy(G), 0.0, 4)
    snap = torch.load(path, map_location='cpu', weights_only=True)
    shapes = {tuple(b.shape) for b in vgg.buffers() if b.ndim == 4}
    for key in ('G', 'D', 'D_parsing', 'G_ema'):
        assert not any('vgg' in k.lower() for k in snap[key])
        assert not any(tuple(v.shape) in shapes for v in snap[key].values())
    assert set(snap['G']) == set(G.state_dict())


# ---------------------------------------------------------------------------- driver

def test_parse_args_accepts_vgg_ckpt():
    from training.training_loop import parse_args
    a = parse_args(['--data', 'd', '--outdir', 'o', '--vgg_weight', '20', '--vgg_ckpt', 'vgg19.pth'])
    assert a.vgg_weight == 20 and a.vgg_ckpt == 'vgg19.pth'
    assert parse_args(['--data', 'd', '--outdir', 'o']).vgg_ckpt is None          # no implicit default path


def test_refusals(vgg, tmp_path, monkeypatch):
    from training import training_loop as T
    from training.loss import StyleGAN2Loss
    with pytest.raises(NotImplementedError, match='checkpoint'):
        StyleGAN2Loss(device=torch.device('cpu'), **stubs.build(), vgg_weight=20)
    with pytest.raises(NotImplementedError):
        StyleGAN2Loss(device=torch.device('cpu'), **stubs.build(), vgg_weight=20, vgg=vgg, contextual_weight=1)
    StyleGAN2Loss(device=torch.device('cpu'), **stubs.build(), vgg_weight=20, vgg=vgg)

    def no_networks(*args, **kw):
        raise AssertionError('a network was built before the refusal')
    monkeypatch.setattr(T, 'build_networks', no_networks)
    with pytest.raises(NotImplementedError, match='vgg_ckpt'):
        T.training_loop(str(tmp_path / 'run'), str(tmp_path / 'data'), vgg_weight=20, device='cpu')
    with pytest.raises(FileNotFoundError, match='missing.pth'):
        T.training_loop(str(tmp_path / 'run'), str(tmp_path / 'data'), vgg_weight=20, vgg_ckpt=str(tmp_path / 'missing.pth'), device='cpu')
