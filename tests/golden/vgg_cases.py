"""What g12_vgg.npz stores of the VGG19 perceptual loss, shared by its generator (make_golden_vgg.py) and the tests: the cases, their name-keyed
inputs and, of every large tensor, a digest in the manner of ``augment_cases.py``: every `step`-th element of the flattened tensor (about
2048 of them), K weighted sums over EVERY element (dot products with name-keyed ``detgen`` weights) and the tensor's max-abs, so that the fixture
stays small while an error anywhere still shows.

Bars: a max-abs bar `tol` on the elements becomes `tol * sum|w_k|` on the k-th sum (the worst case of an error of `tol` everywhere)."""

import numpy as np
import torch

from detgen import det_tensor

CASES = {'A': [2, 3, 64, 96], 'B': [1, 3, 136, 152]}      # B: pooled sizes 136 -> 68 -> 34 -> 17 -> 8 and 152 -> 76 -> 38 -> 19 -> 9 exercise the floor
TAP_NAMES = ('relu1_1', 'relu2_1', 'relu3_1', 'relu4_1', 'relu5_1')
K = 2
SAMPLES = 2048


def inputs(case):
    shape = CASES[case]
    tag = 'x'.join(str(s) for s in shape)
    return det_tensor(f'vgg.x.{tag}', shape, 'uniform'), det_tensor(f'vgg.y.{tag}', shape, 'uniform')


def subsample(t):
    flat = t.reshape(-1)
    return flat[::max(1, flat.numel() // SAMPLES) | 1]


def weights(shape):
    tag = 'x'.join(str(int(s)) for s in shape)
    return [det_tensor(f'vgg.proj.{k}.{tag}', list(shape), 'uniform').double() for k in range(K)]


def projections(t):
    t = torch.as_tensor(t).detach().cpu().double()
    return np.array([float((t * w).sum()) for w in weights(t.shape)])


def put(out, key, t):
    t = torch.as_tensor(t).detach().cpu()
    out[key + '/px'] = subsample(t).float().numpy()
    out[key + '/sum'] = projections(t)
    out[key + '/max'] = np.float64(t.abs().max())


def deviation(g, key, t):
    """(max-abs over the stored elements, worst weighted-sum error as the uniform element error that would explain it, stored max-abs)."""
    t = torch.as_tensor(t).detach().cpu().double()
    pix = float((subsample(t) - torch.as_tensor(np.asarray(g[key + '/px'])).double()).abs().max())
    mass = np.array([float(w.abs().sum()) for w in weights(t.shape)])
    sums = float(np.max(np.abs(projections(t) - np.asarray(g[key + '/sum'])) / mass))
    return pix, sums, float(g[key + '/max'])


def check(g, key, t, rel_tol):
    """Asserts that `t` matches the stored digest within `rel_tol` x the stored tensor's max-abs; returns deviation()'s triple."""
    pix, sums, scale = deviation(g, key, t)
    assert pix <= rel_tol * scale, f'{key}: stored elements: max-abs {pix:.3e} > {rel_tol:.0e} * {scale:.3e}'
    assert sums <= rel_tol * scale, f'{key}: weighted sums: equivalent uniform error {sums:.3e} > {rel_tol:.0e} * {scale:.3e}'
    return pix, sums, scale
