"""The try-on loader's front half on the GPU: a ``collate_raw`` batch (decoded files and key-point tables, ``TryOnTestSet.raw``) in, a
``collate_unrouted`` batch out -- every map ``TryOnTestSet.unrouted`` builds per pixel, bit for bit, without the host's 100 ms per pair.

``front_batch(raw_batch, part)``:

* on a GPU batch, three native launches (csrc/tryon_front.hip) and no host sync: ``pg_tryon_front_stats`` (label-group counts, first rows, the skin
  histogram), ``pg_tryon_front_bit_rows`` (the arm bands and the canvas mask as bit rows, the pass along x of their dilation / erosion) and
  ``pg_tryon_front_compose`` (every data-dependent decision of ``_host_<part>`` resolved on the device, every map written).  The number of launches
  depends neither on the batch size nor on the mode;
* on a CPU batch, the loader's own host code on the decoded arrays (``dataset.unrouted_from_raw``): no second implementation of the arithmetic.

``route``, ``batch_inputs`` and ``triptych`` of training/tryon.py consume the result unchanged.

part='outfit' (``TryOnTestSet(part='outfit')``: the lower garment from a second clothes image) adds two inputs, lower_img and lower_parsing, and one
output, lower_clothes; the same three launches read and write them."""

import ctypes

import torch

from torch_utils import custom_ops
from torch_utils.ops import _native as nat
from . import dataset as ds_mod
from .tryon import MODE_CODE

STATS, PRIMS = 788, ds_mod.PRIMS                      # PG_FRONT_STATS, PG_FRONT_PRIMS
LAUNCHES = ('stats', 'bit_rows', 'compose')

launch_counter = None     # a dict(stats=0, bit_rows=0, compose=0) counts the native launches of this module (tests, tools/tryon_bench.py)

_IN = ('person_img', 'clothes_img', 'person_parsing', 'clothes_parsing', 'garment_parsing', 'pose_prims', 'bands', 'band_absent', 'hip_top')
_SCRATCH = ('stats', 'bit_rows')
_OUT = ('upper_img', 'lower_img', 'upper_mask', 'lower_mask', 'sleeve', 'image', 'clothes', 'pose', 'retain_mask', 'canvas', 'bound', 'skin', 'label')
_LOWER_IN = ds_mod._RAW_LOWER_ARRAYS                  # outfit batches only: the lower clothes' image and parsing -> lower_src_img, lower_src_parsing
_LOWER = ('lower_src_img', 'lower_src_parsing', 'lower_clothes')      # the struct's last fields (NULL in the other modes)


class FrontIO(ctypes.Structure):
    """Mirror of ``pg_front_io`` (include/pasta_gan_ops.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in _IN + _SCRATCH + _OUT + _LOWER]


_plugin = None


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('tryon_front_plugin')
        lib = plugin.lib
        lib.pg_tryon_front_stats.restype = ctypes.c_int
        lib.pg_tryon_front_stats.argtypes = [ctypes.POINTER(FrontIO)] + [ctypes.c_int] * 3 + [ctypes.c_void_p]
        for fn in (lib.pg_tryon_front_bit_rows, lib.pg_tryon_front_compose):
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.POINTER(FrontIO)] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        _plugin = plugin
    return _plugin


def _count(name):
    if launch_counter is not None:
        launch_counter[name] += 1


_DTYPES = dict(person_img=torch.uint8, clothes_img=torch.uint8, person_parsing=torch.uint8, clothes_parsing=torch.uint8, garment_parsing=torch.uint8,
               pose_prims=torch.int32, bands=torch.float64, band_absent=torch.int32, hip_top=torch.int32, lower_img=torch.uint8, lower_parsing=torch.uint8)


def _check(raw, part):
    """Shapes, dtypes, devices and layout of an uploaded ``collate_raw`` batch -> (device, n, H, W)."""
    if part not in MODE_CODE:
        raise ValueError(f'part must be one of {sorted(MODE_CODE)}, not {part!r}')
    img = raw['person_img']
    if not (isinstance(img, torch.Tensor) and img.dim() == 4 and img.shape[3] == 3):
        raise nat.NativeOpError('tryon_front: person_img must be a [N, H, W, 3] tensor')
    dev, (n, H, W, _) = img.device, img.shape
    shapes = dict(person_img=(n, H, W, 3), clothes_img=(n, H, W, 3), person_parsing=(n, H, W), clothes_parsing=(n, H, W), garment_parsing=(n, H, W),
                  pose_prims=(n, PRIMS, 8), bands=(n, 4, 4, 2), band_absent=(n, 4), hip_top=(n, 2), lower_img=(n, H, W, 3), lower_parsing=(n, H, W))
    for k in _IN + (_LOWER_IN if part == 'outfit' else ()):
        t = raw.get(k)
        if t is None and k == 'garment_parsing':
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == _DTYPES[k] and t.device == dev and tuple(t.shape) == shapes[k] and t.is_contiguous()):
            raise nat.NativeOpError(f'tryon_front: {k} must be a contiguous {_DTYPES[k]} tensor of shape {shapes[k]} on {dev}')
    return dev, n, H, W


def front_batch(raw, part):
    """An uploaded ``collate_raw`` batch -> the dict of an uploaded ``collate_unrouted`` batch (same keys, dtypes, shapes, devices)."""
    dev, n, _, _ = _check(raw, part)
    outfit = part == 'outfit'
    names = {k: raw[k] for k in ds_mod._NAME_KEYS + (ds_mod._LOWER_NAME_KEYS if outfit else ())}
    if dev.type != 'cuda':
        arrays = {k: (None if raw[k] is None else raw[k].numpy()) for k in _IN + (_LOWER_IN if outfit else ())}
        items = []
        for i in range(n):
            item = {k: (None if v is None else v[i]) for k, v in arrays.items()}
            item.update({k: v[i] for k, v in names.items()})
            items.append(ds_mod.unrouted_from_raw(item, part))
        return ds_mod.collate_unrouted(items)

    plan = plan_batch(raw, part)
    for name in LAUNCHES:
        launch(plan, name)
    plan['out'].update(names)
    return plan['out']


def plan_batch(raw, part):
    """The outputs, the scratch and the ``pg_front_io`` of one GPU batch; ``launch(plan, name)`` enqueues one of `LAUNCHES` (in that order they make
    ``front_batch``; tools/tryon_front_bench.py times each alone)."""
    dev, n, H, W = _check(raw, part)
    sleeve, full, outfit = raw['garment_parsing'] is not None, part in ('full', 'outfit'), part == 'outfit'
    u8 = lambda *shape: torch.empty([n, *shape], dtype=torch.uint8, device=dev)
    out = dict(upper_img=u8(H, H, 3), lower_img=u8(H, H, 3), upper_mask=u8(H, H, 3), lower_mask=u8(H, H, 3), sleeve=u8(H, H, 1) if sleeve else None,
               image=u8(H, H, 3), clothes=u8(H, H, 3), pose=u8(H, H, 3), retain_mask=u8(H, H, 1), bound=u8(H), canvas=None if full else u8(H, H, 3),
               **(dict(lower_clothes=u8(H, H, 3)) if outfit else {}),            # (the key order of ``collate_unrouted``)
               skin=torch.empty([n, 3], dtype=torch.float32, device=dev), label=torch.empty([n], dtype=torch.int32, device=dev))
    scratch = dict(stats=torch.empty([n, STATS], dtype=torch.int32, device=dev),
                   bit_rows=torch.empty([n, 5, H, (H + 31) // 32], dtype=torch.int32, device=dev))
    p = lambda t: None if t is None else t.data_ptr()
    io = FrontIO(*[p(raw[k]) for k in _IN], *[p(scratch[k]) for k in _SCRATCH], *[p(out[k]) for k in _OUT],
                 *([p(raw['lower_img']), p(raw['lower_parsing']), p(out['lower_clothes'])] if outfit else []))
    return dict(io=io, out=out, scratch=scratch, raw=raw, dev=dev, dims=(n, H, W), left=(H - W) // 2, mode=MODE_CODE[part])


def launch(plan, name):
    lib, io, (n, H, W) = _init().lib, ctypes.byref(plan['io']), plan['dims']
    stream = nat.stream_of(plan['raw']['person_img'])
    with torch.cuda.device(plan['dev']):
        if name == 'stats':
            nat.check(lib.pg_tryon_front_stats(io, n, H, W, stream), 'pg_tryon_front_stats')
        else:
            nat.check(getattr(lib, 'pg_tryon_front_' + name)(io, n, H, W, plan['left'], plan['mode'], stream), 'pg_tryon_front_' + name)
    _count(name)


def launch_bytes(n, H, W, part, sleeve):
    """Bytes each launch has to move for a batch (computed from the shapes; tools/tryon_bench.py divides them by the measured device times)."""
    px, words = H * W, (H + 31) // 32
    outfit = part == 'outfit'
    full = part == 'full' or outfit
    maps3 = 7 + (0 if full else 1) + (1 if outfit else 0)                     # the three-channel maps compose writes
    return dict(stats=n * ((3 if outfit else 2) * px + 4 * STATS),            # the parsings; the skin pixels of the image come on top
                bit_rows=n * ((0 if full else px) + (4 if full else 5) * H * words * 4),
                compose=n * (px * (8 + (4 if outfit else 0) + (1 if sleeve else 0)) + H * H * (3 * maps3 + 1 + (1 if sleeve else 0)) + H))
