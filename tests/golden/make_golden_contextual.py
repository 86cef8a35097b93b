#!/usr/bin/env python3
"""Generate ``g14_contextual.npz`` by running THE REFERENCE's ``ContextualLoss_forward`` and ``VGG19_feature_color_torchversion``
(training/loss_fullbody.py:481-618) on the CPU.

Runs only in the build container (needs /root/reference; never on the GPU box); imports the reference the way ``make_golden_vgg.py`` does.
``./checkpoints/vgg19_conv.pth`` is not available: the trunk is constructed and ``load_state_dict``'s ``synthetic.vgg19_conv_state_dict()``
directly, no checkpoint file.  This fixture therefore pins the COMPUTATION, not the pretrained network.

Stored per op case of ``contextual_cases.OP_CASES`` (x, y, G = ``op_inputs(case)``, per-sample weights w = ``op_weights(case)``):
    loss_ref [S]     the reference class's per-sample loss (float32; y repeated over the groups)
    dx_ref/*         digest of its gradient d(sum_s w_s loss_s)/dx
    loss [S], dx/*   the same from the float64 restatement (tests/contextual_ref.py)
    loss_dev         max_s |loss_ref - loss|;  dx_dev = max|dx_ref - dx| / max|dx|: the float32 composition's own distance from float64
    gap_d, gap_a     the smallest arg-min / relative arg-max gaps over the rows
Per trunk case: digests of the five float64 taps of x (``<tap>/*``) with the float32 reference's deviation ``<tap>_dev`` (of the tap's maximum),
the combined loss (``contextual_ref.combine`` on float64 taps; ``loss_ref`` = the reference classes in float32 combined the same way), ``dx/*``,
``dx_ref/*`` and their deviations, and ``relu_margin`` / ``pool_margin`` (``contextual_ref.trunk_margins``).

The generator ASSERTS the conditions under which the fixture's bars mean something; a case that misses one is replaced, never skipped.

Usage:  python tests/golden/make_golden_contextual.py
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import contextual_cases as CC  # noqa: E402
import contextual_ref as CR  # noqa: E402
import detgen  # noqa: E402
import vgg_cases as VC  # noqa: E402

REF = '/root/reference'
if not os.path.isdir(REF):
    sys.exit('make_golden_contextual.py needs /root/reference (build container only)')
torch.version.cuda = '10.0'
sys.path.insert(0, REF)
os.chdir(REF)
torch.set_num_threads(8)

import training.loss_fullbody as RL  # noqa: E402

META = dict(reference='xiezhy6/PASTA-GAN-plusplus @ /root/reference', torch=torch.__version__, numpy=np.__version__,
            weights='training.synthetic.vgg19_conv_state_dict (not the pretrained vgg19_conv.pth)')


def maxabs(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


def op_case(out, case, crit):
    x, y, groups = CC.op_inputs(case)
    w = CC.op_weights(case)
    x32 = x.clone().requires_grad_(True)
    loss_ref = crit(x32, y.repeat([groups, 1, 1, 1]))
    dx_ref, = torch.autograd.grad((loss_ref * w.float()).sum(), x32)
    loss, dx = CR.loss_and_grad(x, y, groups=groups, weights=w)
    gap_d, gap_a = CR.gaps(x, y.repeat([groups, 1, 1, 1]))
    top = float(dx.abs().max())
    assert float(loss.min()) >= 1e-2, (case, loss)
    assert gap_d >= 1e-6 and gap_a >= 1e-5, (case, gap_d, gap_a)
    out[f'{case}/loss_ref'] = loss_ref.detach().numpy()
    out[f'{case}/loss'] = loss.numpy()
    VC.put(out, f'{case}/dx_ref', dx_ref)
    VC.put(out, f'{case}/dx', dx)
    out[f'{case}/loss_dev'] = np.float64(maxabs(loss_ref, loss))
    out[f'{case}/dx_dev'] = np.float64(maxabs(dx_ref, dx) / top)
    out[f'{case}/gap_d'], out[f'{case}/gap_a'] = np.float64(gap_d), np.float64(gap_a)
    print(f'{case}: loss {loss.numpy()}, float32 deviation {out[f"{case}/loss_dev"]:.2e}; dx max {top:.3e}, float32 deviation {out[f"{case}/dx_dev"]:.2e} '
          f'of it; gaps {gap_d:.2e} / {gap_a:.2e}')


def ref_combined(trunk, crit, x, y):
    pool = torch.nn.functional.avg_pool2d
    fx, fy = trunk(x, list(CC.TAP_NAMES), preprocess=True), [t.detach() for t in trunk(y, list(CC.TAP_NAMES), preprocess=True)]
    loss = 8 * crit(fx[4], fy[4]).mean() + 4 * crit(fx[3], fy[3]).mean() + 2 * crit(pool(fx[2], 2), pool(fy[2], 2)).mean()
    return fx, loss


def trunk_case(out, case, crit):
    sd = detgen._mod.vgg19_conv_state_dict()
    trunk = RL.VGG19_feature_color_torchversion(vgg_normal_correct=True)
    trunk.load_state_dict(sd)
    trunk.requires_grad_(False)
    x, y = CC.trunk_inputs(case)
    relu_margin, pool_margin = CR.trunk_margins(sd, x)
    assert min(relu_margin, pool_margin) >= CC.TRUNK_MARGIN, (case, relu_margin, pool_margin)
    out[f'{case}/relu_margin'], out[f'{case}/pool_margin'] = np.float64(relu_margin), np.float64(pool_margin)
    x32 = x.clone().requires_grad_(True)
    taps32, loss32 = ref_combined(trunk, crit, x32, y)
    dx32, = torch.autograd.grad(loss32, x32)
    trunk.double()
    x64 = x.double().requires_grad_(True)
    taps64 = trunk(x64, list(CC.TAP_NAMES), preprocess=True)
    with torch.no_grad():
        tapsy = trunk(y.double(), list(CC.TAP_NAMES), preprocess=True)
    loss64 = CR.combine(taps64, tapsy)[0]
    dx64, = torch.autograd.grad(loss64, x64)
    for name, t32, t64 in zip(CC.TAP_NAMES, taps32, taps64):
        VC.put(out, f'{case}/{name}', t64)
        out[f'{case}/{name}_dev'] = np.float64(maxabs(t32, t64) / float(t64.detach().abs().max()))
    top = float(dx64.abs().max())
    out[f'{case}/loss_ref'], out[f'{case}/loss'] = np.float64(loss32.detach()), np.float64(loss64.detach())
    out[f'{case}/loss_dev'] = np.float64(abs(float(loss32.detach()) - float(loss64.detach())))
    VC.put(out, f'{case}/dx_ref', dx32)
    VC.put(out, f'{case}/dx', dx64)
    out[f'{case}/dx_dev'] = np.float64(maxabs(dx32, dx64) / top)
    print(f'{case}: loss {float(loss64.detach()):.6f}, float32 deviation {out[f"{case}/loss_dev"]:.2e}; dx max {top:.3e}, float32 deviation '
          f'{out[f"{case}/dx_dev"]:.2e} of it; taps ' + ', '.join(f'{out[f"{case}/{n}_dev"]:.1e}' for n in CC.TAP_NAMES))
    assert out[f'{case}/dx_dev'] <= 1e-3, (case, out[f'{case}/dx_dev'])


def main():
    out = {}
    crit = RL.ContextualLoss_forward(PONO=True)
    for case in CC.OP_CASES:
        op_case(out, case, crit)
    for case in CC.TRUNK_CASES:
        trunk_case(out, case, crit)
    path = os.path.join(HERE, 'g14_contextual.npz')
    arrays = {k: np.asarray(v) for k, v in out.items()}
    arrays['__meta__'] = np.array(repr(META))
    np.savez_compressed(path, **arrays)
    print(f'wrote {path}: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
