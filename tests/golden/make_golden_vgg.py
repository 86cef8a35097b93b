#!/usr/bin/env python3
"""Generate ``g12_vgg.npz`` by running THE REFERENCE's ``VGGLoss`` / ``VGG19_Feature`` (training/loss_fullbody.py:336-386) on the CPU.

Runs only in the build container (needs /root/reference; never on the GPU box); imports the reference the way ``make_golden_augment.py``
does.  The reference's constructor reads ``./checkpoints/vgg19-dcbb9e9d.pth`` with a strict ``load_state_dict``; the pretrained file is not
available, so a temporary checkpoint made from ``synthetic.vgg19_state_dict(classifier=True)`` is written to a scratch directory outside the
repository and the classes are constructed from there.  This fixture therefore pins the COMPUTATION (slices, taps, weights of the five
terms, no input normalisation), not the pretrained network.

Stored per case of ``vgg_cases.CASES``, for ``x, y = vgg_cases.inputs(case)``: digests of the five tap features of `x`, the loss scalar
``VGGLoss(x, y)`` and the digest of its gradient with respect to `x`.

Usage:  python tests/golden/make_golden_vgg.py
"""

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import detgen  # noqa: E402
import vgg_cases as VC  # noqa: E402

REF = '/root/reference'
if not os.path.isdir(REF):
    sys.exit('make_golden_vgg.py needs /root/reference (build container only)')
torch.version.cuda = '10.0'
sys.path.insert(0, REF)
os.chdir(REF)
torch.set_num_threads(8)

import training.loss_fullbody as RL  # noqa: E402

META = dict(reference='xiezhy6/PASTA-GAN-plusplus @ /root/reference', torch=torch.__version__, numpy=np.__version__,
            weights='training.synthetic.vgg19_state_dict (not the pretrained vgg19-dcbb9e9d.pth)')


def main():
    out = {}
    with tempfile.TemporaryDirectory() as scratch:
        os.makedirs(os.path.join(scratch, 'checkpoints'))
        torch.save(detgen._mod.vgg19_state_dict(classifier=True), os.path.join(scratch, 'checkpoints', 'vgg19-dcbb9e9d.pth'))
        os.chdir(scratch)
        try:
            crit = RL.VGGLoss(device=torch.device('cpu'), requires_grad=False)
        finally:
            os.chdir(REF)
    for case in VC.CASES:
        x, y = VC.inputs(case)
        x.requires_grad_(True)
        for name, f in zip(VC.TAP_NAMES, crit.vgg(x)):
            VC.put(out, f'{case}/{name}', f)
        loss = crit(x, y)
        dx, = torch.autograd.grad(loss, x)
        out[f'{case}/loss'] = np.float64(loss.detach())
        VC.put(out, f'{case}/dx', dx)

    path = os.path.join(HERE, 'g12_vgg.npz')
    arrays = {k: np.asarray(v) for k, v in out.items()}
    arrays['__meta__'] = np.array(repr(META))
    np.savez_compressed(path, **arrays)
    print(f'wrote {path}: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
