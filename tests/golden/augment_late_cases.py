"""The case list of g13_augment_late.npz, shared by its generator (make_golden_augment_late.py) and the tests: shapes, specs, keys, the
seed of every call and the digest strides (the digest itself is ``augment_cases.py``'s)."""

import zlib

from detgen import det_tensor

SHAPES = {'small': [2, 3, 64, 96], 'min': [1, 3, 22, 23], 'tiles': [3, 1, 70, 150]}
STRIDE = {'small': 4, 'min': 2, 'tiles': 4}
BGC = dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1)
SPECS = {   # the reference's train.py augpipe_specs entries used here, and the gradient case's filter + cutout pipe
    'filter': dict(imgfilter=1),
    'noise': dict(noise=1),
    'cutout': dict(cutout=1),
    'bgcfnc': dict(BGC, imgfilter=1, noise=1, cutout=1),
    'filtercut': dict(imgfilter=1, cutout=1),
}
DET_PCTS = {'filter': (0.1, 0.83), 'noise': (0.1, 0.5, 0.83), 'cutout': (0.1, 0.5, 0.83)}
SEEDED_P = (0.6, 1.0)
# name -> (spec, shape, forward keywords, p)
GRAD_CASES = {'bgcfnc': ('bgcfnc', 'small', dict(debug_percentile=0.83), 1.0), 'filtercut': ('filtercut', 'tiles', dict(), 1.0)}


def det_keys():
    keys = [f'det/{spec}/{pct}/{shape}' for spec, pcts in DET_PCTS.items() for pct in pcts for shape in SHAPES]
    return keys + [f'det/bgcfnc/{pct}/small' for pct in (0.1, 0.5, 0.83)]


def seed_keys():
    return [f'seed/{spec}/{p}/{shape}' for spec in ('filter', 'bgcfnc') for p in SEEDED_P for shape in ('small', 'tiles')]


def grad_key(name):
    return f'grad/{name}/y/{GRAD_CASES[name][1]}'


def seed_of(key):
    """torch.manual_seed of the call that made `key`."""
    return 4000 + zlib.crc32(key.encode()) % 1000


def image(shape):
    return det_tensor('aug.x.' + 'x'.join(str(s) for s in shape), shape, 'uniform')


def grad_dy(name, shape):
    return det_tensor(f'aug.late.grad.dy.{name}', list(shape))
