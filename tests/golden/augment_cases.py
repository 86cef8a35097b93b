"""What g11_augment.npz stores of an augmented image, shared by its generator (make_golden_augment.py) and the tests: a strided
subsample of the pixels, and K weighted sums over EVERY pixel (dot products with name-keyed ``detgen`` weights), so that the
fixture stays small while an error anywhere in the image still shows.

Bars: a max-abs bar `tol` on the pixels becomes `tol * sum|w_k|` on the k-th sum (the worst case of an error of `tol` everywhere)."""

import numpy as np
import torch

from detgen import det_tensor

STRIDE = {'small': 4, 'large': 8, '1ch': 4}     # [2, 3, 64, 96] / [1, 3, 256, 256] / [2, 1, 64, 96]
K = 4


def subsample(y, stride):
    return y[:, :, 1::stride, 2::stride]


def weights(shape):
    tag = 'x'.join(str(int(s)) for s in shape)
    return [det_tensor(f'aug.proj.{k}.{tag}', list(shape), 'uniform').double() for k in range(K)]


def projections(y):
    y = torch.as_tensor(y).detach().cpu().double()
    return np.array([float((y * w).sum()) for w in weights(y.shape)])


def digest(y, stride):
    """(strided pixels, weighted sums) of `y` as the fixture stores them."""
    y = torch.as_tensor(y).detach().cpu()
    return subsample(y, stride).float().numpy(), projections(y)


def check(y, stored_pixels, stored_sums, stride, tol):
    """Asserts that `y` matches the stored digest within the max-abs bar `tol`; returns (pixel max-abs, worst sum error / its bar)."""
    y = torch.as_tensor(y).detach().cpu().double()
    pix = float((subsample(y, stride) - torch.as_tensor(np.asarray(stored_pixels)).double()).abs().max())
    bars = np.array([tol * float(w.abs().sum()) for w in weights(y.shape)])
    sums = np.abs(projections(y) - np.asarray(stored_sums))
    assert pix <= tol, f'strided pixels: max-abs {pix:.3e} > {tol:.0e}'
    assert np.all(sums <= bars), f'weighted sums: errors {sums} > bars {bars}'
    return pix, float(np.max(sums / bars))
