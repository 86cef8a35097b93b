"""What g14_contextual.npz stores of the contextual loss, shared by its generator (make_golden_contextual.py) and the tests: the op cases, the
trunk cases and their name-keyed inputs.  Large tensors are stored as ``vgg_cases.put`` digests.

Op inputs: ``y = 30 relu(n_y)`` and ``x = mix y + (1 - mix) 30 relu(n_x)`` with name-keyed normal n: ReLU'd features at a VGG-like scale, `x`
correlated with `y` as a generated image is with its target.  mix <= 0.3 keeps every row away from an arg-min / arg-max tie (the generator asserts the
gaps); mix >= 0.7 saturates (loss 0, gradient ~ 1e-18) and is no parity case."""

import torch

from detgen import det_tensor

SCALE = 30.0
# name -> (S, N, C, H, W, mix); G = S // N
OP_CASES = {
    'small': (2, 2, 21, 5, 7, 0.3),
    'groups': (4, 2, 64, 9, 13, 0.2),
    'edges': (1, 1, 128, 33, 31, 0.3),          # P = 1023: crosses every tile edge
    'deep': (1, 1, 512, 32, 32, 0.3),           # the full K depth of the VGG features
    'blocks': (2, 1, 36, 48, 48, 0.25),         # several row blocks per sample, G = 2
}
CPU_OP_CASES = ('small', 'groups', 'edges')     # the ones the CPU test runs (the float32 composition of the others takes seconds)
# name -> (shape, draw).  An end-to-end gradient is a parity case only if no ReLU mask and no pool arg-max of the trunk hangs on a float32 rounding: the
# generator asserts that the float64 trunk keeps every pre-activation and every pool window's top-two gap at least TRUNK_MARGIN of the layer's maximum
# away from the decision (contextual_ref.trunk_margins) -- twice the 1e-6 the taps are held to.  With ~ 1e5 units that holds for about one name-keyed
# draw in eight at this size (draws 0 .. 18 miss it; [2, 3, 64, 96] has ~ 4e6 units and margins of 1e-7 in every draw tried).
TRUNK_CASES = {'T': ([1, 3, 32, 32], 19)}
TRUNK_MARGIN = 2e-6
TAP_NAMES = ('r12', 'r22', 'r32', 'r42', 'r52')
LOSS_WEIGHTS = (1.0, 0.7, 1.3, 0.9)             # d(sum_s w_s loss_s)/dx is the stored gradient: distinct per-sample weights


def op_inputs(case):
    s, n, c, h, w, mix = OP_CASES[case]
    y = SCALE * torch.relu(det_tensor(f'cx.{case}.y', [n, c, h, w]))
    noise = SCALE * torch.relu(det_tensor(f'cx.{case}.x', [s, c, h, w]))
    x = mix * y.repeat([s // n, 1, 1, 1]) + (1 - mix) * noise
    return x, y, s // n


def op_weights(case):
    return torch.tensor(LOSS_WEIGHTS[:OP_CASES[case][0]], dtype=torch.float64)


def trunk_inputs(case):
    shape, draw = TRUNK_CASES[case]
    tag = 'x'.join(str(v) for v in shape) + f'.{draw}'
    return det_tensor(f'cx.trunk.x.{tag}', shape, 'uniform'), det_tensor(f'cx.trunk.y.{tag}', shape, 'uniform')
