"""The try-on test driver: a network snapshot and test pairs in, the reference's result images out (reference test.py / test.sh).

Per batch, on a GPU:

1. ``TryOnTestSet.unrouted`` items (a DataLoader with `workers` processes, ``collate_unrouted``, pinned) are uploaded asynchronously -- or, with
   ``front='native'``, ``TryOnTestSet.raw`` items (``collate_raw``), from which ``tryon_front.front_batch`` builds the same batch on the device (three
   native launches);
2. ``patch_routing.normalize_batch(..., part=dataset.part)`` routes the whole batch (three native launches);
3. ``pg_tryon_row_extent_u8`` finds the first / last row of the canvases the bound rules read, ``pg_tryon_inputs`` writes the seven float32
   generator inputs of ``dataset.to_generator_inputs`` (two launches, no host work between them);
4. ``G(..., noise_mode='const')``, keeping the second output (finetune_img) as test.py does;
5. ``pg_tryon_triptych_u8`` packs clothes | person | result (columns 96:416 of each) as uint8 RGB, and one asynchronous copy brings those bytes to
   pinned host memory -- the batch's only host sync is waiting for that copy;
6. a thread pool encodes the PNGs (Pillow, RGB, compress_level=1) while the next batch runs.

The outfit mode (``--testpart outfit``; this package's own: the top of one clothes image, the trousers or skirt of another, pairs-file lines of
``<upper> <lower> <person>``) goes the same way; the routing takes the lower clothes' key points for the lower parts, the bound rule is the full mode's,
and step 5 packs four panels, upper clothes | lower clothes | person | result (``pg_tryon_panels_u8``), into ``person___upper___lower.png``.

``device='cpu'`` runs the same flow through plain torch and NumPy: ``normalize_batch``'s CPU route, the inputs as ``to_generator_inputs`` computes them,
and ``triptych_numpy``.

The result arithmetic is pinned against a restatement of test.py:162-181 (tests/test_tryon_cpu.py, tests/test_tryon_gpu.py).  test.py runs on a GPU,
where torch computes ``u / 127.5`` as ``u * (1.0f / 127.5f)``; the clothes and person columns of both routes use that product, so their bytes are the
reference's, including the round trip's one-below results.  NaN in the generator output becomes 0 (NumPy leaves that cast undefined)."""

import argparse
import concurrent.futures
import ctypes
import os

import numpy as np
import torch

from torch_utils import custom_ops
from torch_utils.ops import _native as nat
from . import checkpoint
from . import dataset as ds_mod
from . import networks
from . import patch_routing

MODE_CODE = {'upper': 0, 'lower': 1, 'full': 2, 'outfit': 3}      # enum pg_tryon_mode
X0, CW = 96, 320                                      # the columns test.py keeps of each image (test.py:179-180)
_INV = np.float32(1.0) / np.float32(127.5)            # torch's GPU `t / 127.5` multiplies by this

launch_counter = None     # a dict(row_extent=0, inputs=0, triptych=0, panels=0) counts the native launches of this module (tests, tools/tryon_bench.py)


class TryonIO(ctypes.Structure):
    """Mirror of ``pg_tryon_io`` (include/pasta_gan_ops.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in ('image', 'pose', 'retain_mask', 'denorm_upper', 'denorm_lower', 'norm_img', 'norm_img_lower', 'skin',
                                                     'label', 'bound_rows', 'extents', 'c', 'retain', 'pose_out', 'denorm_upper_out', 'denorm_lower_out',
                                                     'upper_mask_out', 'lower_mask_out')]


_plugin = None


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('tryon_plugin')
        lib = plugin.lib
        lib.pg_tryon_row_extent_u8.restype = ctypes.c_int
        lib.pg_tryon_row_extent_u8.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
        lib.pg_tryon_inputs.restype = ctypes.c_int
        lib.pg_tryon_inputs.argtypes = [ctypes.POINTER(TryonIO)] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        lib.pg_tryon_triptych_u8.restype = ctypes.c_int
        lib.pg_tryon_triptych_u8.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        lib.pg_tryon_panels_u8.restype = ctypes.c_int
        lib.pg_tryon_panels_u8.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        _plugin = plugin
    return _plugin


def _count(name):
    if launch_counter is not None:
        launch_counter[name] = launch_counter.get(name, 0) + 1


def _check_u8(name, t, dev, ndim):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device == dev and t.dim() == ndim and t.is_contiguous()):
        raise nat.NativeOpError(f'tryon: {name} must be a contiguous {ndim}-D uint8 tensor on {dev}')


# ------------------------------------------------------------------------------------------------------------- native entry points

def row_extents(canvases):
    """First and last row holding a non-zero byte of every canvas [M, H, W, C] uint8 -> int32 [M, 2] (-1 / -1 when empty).  GPU: one launch of
    pg_tryon_row_extent_u8; CPU: plain torch."""
    if canvases.device.type != 'cuda':
        rows = (canvases != 0).flatten(2).any(dim=2)                                       # [M, H]
        idx = torch.arange(rows.shape[1], dtype=torch.int32)
        lo = torch.where(rows, idx, rows.shape[1]).amin(dim=1)
        hi = torch.where(rows, idx, -1).amax(dim=1)
        return torch.stack([torch.where(hi >= 0, lo, -1), hi], dim=1).to(torch.int32)
    _check_u8('canvases', canvases, canvases.device, 4)
    m, h, w, c = canvases.shape
    ext = torch.empty([m, 2], dtype=torch.int32, device=canvases.device)
    with torch.cuda.device(canvases.device):
        nat.check(_init().lib.pg_tryon_row_extent_u8(canvases.data_ptr(), m, h, w, c, ext.data_ptr(), nat.stream_of(canvases)), 'pg_tryon_row_extent_u8')
    _count('row_extent')
    return ext


def generator_inputs(src, norm_img, norm_img_lower, denorm_upper, denorm_lower, extents, part):
    """The keyword arguments of ``GeneratorFull_v20.forward`` for a batch, in ONE launch of pg_tryon_inputs -- bit for bit what
    ``dataset.to_generator_inputs`` computes on the GPU from the loader's 16-tuple.

    src: a ``collate_unrouted`` batch on the GPU (image, pose, retain_mask, skin, label, bound); norm_img [N, h, w, 30], norm_img_lower [N, h, w, 15],
    denorm_upper / denorm_lower [N, H, W, 3] uint8 NHWC; extents int32 [N, 2] of the canvas the mode's bound rule reads (see ``final_bound``)."""
    image = src['image']
    dev = image.device
    n, H, W, _ = image.shape
    h, w = int(norm_img.shape[1]), int(norm_img.shape[2])
    for name, t, nd in (('image', image, 4), ('pose', src['pose'], 4), ('retain_mask', src['retain_mask'], 4), ('denorm_upper', denorm_upper, 4),
                        ('denorm_lower', denorm_lower, 4), ('norm_img', norm_img, 4), ('norm_img_lower', norm_img_lower, 4), ('bound', src['bound'], 2)):
        _check_u8(name, t, dev, nd)
    skin, label = src['skin'], src['label']
    if skin.dtype != torch.float32 or label.dtype != torch.int32 or extents.dtype != torch.int32 or skin.device != dev or label.device != dev:
        raise nat.NativeOpError('tryon: skin must be float32, label and extents int32, on the images\' device')
    f32 = lambda *shape: torch.empty([n, *shape], dtype=torch.float32, device=dev)
    out = dict(z=torch.zeros([n, 0], device=dev), c=f32(45, h, w), retain=f32(6, H, W), pose=f32(5, H, W), denorm_upper_input=f32(3, H, W),
               denorm_lower_input=f32(3, H, W), denorm_upper_mask=f32(1, H, W), denorm_lower_mask=f32(1, H, W))
    p = lambda t: t.data_ptr()
    io = TryonIO(p(image), p(src['pose']), p(src['retain_mask']), p(denorm_upper), p(denorm_lower), p(norm_img), p(norm_img_lower), p(skin.contiguous()),
                 p(label.contiguous()), p(src['bound']), p(extents.contiguous()), p(out['c']), p(out['retain']), p(out['pose']),
                 p(out['denorm_upper_input']), p(out['denorm_lower_input']), p(out['denorm_upper_mask']), p(out['denorm_lower_mask']))
    with torch.cuda.device(dev):
        nat.check(_init().lib.pg_tryon_inputs(ctypes.byref(io), n, H, W, h, w, MODE_CODE[part], nat.stream_of(image)), 'pg_tryon_inputs')
    _count('inputs')
    return out


def triptych(finetune_img, clothes, image):
    """clothes | person | result, columns 96:416 of each, uint8 RGB [N, H, 960, 3] (test.py:162-181).  GPU: one launch of pg_tryon_triptych_u8
    (result stays on the GPU); CPU: ``triptych_numpy`` (a CPU tensor)."""
    if finetune_img.device.type != 'cuda':
        return torch.from_numpy(triptych_numpy(finetune_img.detach().numpy(), clothes.numpy(), image.numpy()))
    dev = finetune_img.device
    _check_u8('clothes', clothes, dev, 4)
    _check_u8('image', image, dev, 4)
    fin = finetune_img.detach().to(torch.float32).contiguous()
    n, _, H, W = fin.shape
    out = torch.empty([n, H, 3 * CW, 3], dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(_init().lib.pg_tryon_triptych_u8(fin.data_ptr(), clothes.data_ptr(), image.data_ptr(), out.data_ptr(), n, H, W, X0, CW,
                                                   nat.stream_of(fin)), 'pg_tryon_triptych_u8')
    _count('triptych')
    return out


def panels(finetune_img, sources):
    """source 0 | ... | source k-1 | result, columns 96:416 of each, uint8 RGB [N, H, (k + 1) * 320, 3]; every panel with `triptych`'s arithmetic.  The
    outfit mode's sources are (upper clothes, lower clothes, person).  GPU: one launch of pg_tryon_panels_u8; CPU: ``panels_numpy``."""
    sources = list(sources)
    if finetune_img.device.type != 'cuda':
        return torch.from_numpy(panels_numpy(finetune_img.detach().numpy(), [s.numpy() for s in sources]))
    dev = finetune_img.device
    fin = finetune_img.detach().to(torch.float32).contiguous()
    n, _, H, W = fin.shape
    for i, s in enumerate(sources):
        _check_u8(f'sources[{i}]', s, dev, 4)
        if tuple(s.shape) != (n, H, W, 3):
            raise nat.NativeOpError(f'tryon: sources[{i}] must have shape {(n, H, W, 3)}, not {tuple(s.shape)}')
    k = len(sources)
    out = torch.empty([n, H, (k + 1) * CW, 3], dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * k)(*[s.data_ptr() for s in sources])
    with torch.cuda.device(dev):
        nat.check(_init().lib.pg_tryon_panels_u8(fin.data_ptr(), ptrs, k, out.data_ptr(), n, H, W, X0, CW, nat.stream_of(fin)), 'pg_tryon_panels_u8')
    _count('panels')
    return out


# ------------------------------------------------------------------------------------------------------------- the CPU route

def triptych_numpy(finetune_img, clothes, image):
    """test.py:162-181 in NumPy for a batch: finetune_img float32 [N, 3, H, W], clothes / image uint8 [N, H, W, 3] -> uint8 [N, H, 960, 3]."""
    return panels_numpy(finetune_img, [clothes, image])


def panels_numpy(finetune_img, sources):
    """`triptych_numpy`'s statements for any number of source images: finetune_img float32 [N, 3, H, W], sources uint8 [N, H, W, 3] each ->
    uint8 [N, H, (k + 1) * 320, 3]."""
    gen = (finetune_img.transpose(0, 2, 3, 1) + 1.0) * 127.5
    gen = np.clip(gen, 0, 255)
    gen = np.where(np.isnan(gen), np.float32(0), gen).astype(np.uint8)                    # NaN -> 0 (documented rule)
    src = lambda u: (((u.astype(np.float32) * _INV - np.float32(1)) + 1.0) * 127.5).astype(np.uint8)
    sl = slice(X0, X0 + CW)
    return np.ascontiguousarray(np.concatenate([src(s)[:, :, sl] for s in sources] + [gen[:, :, sl]], axis=2))


def final_bound(bound_rows, extents, label, part):
    """The post-routing bound rules on the host rows [N, H] uint8 (what pg_tryon_inputs applies): upper -- ``bound[0:ymax] *= 0`` with ymax the last
    row of denorm_upper_img_wo_sleeve (dataset.py:2688-2690); full and outfit -- ``bound[ymin:] += 255`` from the routed lower garment, and
    ``bound * 0`` for a dress (label 2, dataset.py:1895-1907); lower -- unchanged.  An extent of -1 (empty canvas) changes nothing."""
    b = bound_rows.to(torch.int32)
    rows = torch.arange(b.shape[1], dtype=torch.int32, device=b.device)[None]
    ext = extents.to(torch.int32).to(b.device)
    if part == 'upper':
        ymax = ext[:, 1:2]
        b = torch.where((ymax >= 0) & (rows < ymax), 0, b)
    elif part in ('full', 'outfit'):
        ymin = ext[:, 0:1]
        b = torch.where((ymin >= 0) & (rows >= ymin), (b + 255) % 256, b)
        b = torch.where(label.to(b.device)[:, None] == 2, 0, b)
    return b.to(torch.uint8)


def _canvases(batch, routed, part):
    """(denorm_upper, denorm_lower, the canvas whose row extents the mode's bound rule reads) of a routed batch."""
    if part == 'upper':
        return routed[2], batch['canvas'], routed[3]                       # (the person's own lower garment; denorm_upper_img_wo_sleeve)
    if part == 'lower':
        return batch['canvas'], routed[3], routed[3]                       # (the person's own top; the extents are not read)
    return routed[2], routed[3], routed[3]


def loader_tuple(batch, routed, extents, part):
    """The first 14 entries of the ``TryOnTestSet.__getitem__`` batch (CHW, skin / label maps float64) rebuilt from an unrouted batch and its routing,
    on the batch's device: ``to_generator_inputs(loader_tuple(...), device)`` is the existing path on the same data.  Entry 3 (clothes_pose, which
    the generator does not read) repeats the pose map."""
    den_up, den_lo, _ = _canvases(batch, routed, part)
    chw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    n, H, W, _ = batch['image'].shape
    mask = lambda t: (chw(t).to(torch.int32).sum(dim=1, keepdim=True) > 0).to(torch.uint8)
    skin = batch['skin'].to(torch.float64)[:, :, None, None].expand(n, 3, H, W)          # (float32 medians: their cast to float32 is exact)
    label = (batch['label'].to(torch.float64) / 2.0 * 255)[:, None, None, None].expand(n, 1, H, W)
    bound = final_bound(batch['bound'], extents, batch['label'], part)[:, None, :, None].expand(n, 1, H, W)
    return (chw(batch['image']), chw(batch['clothes']), chw(batch['pose']), chw(batch['pose']), chw(routed[0]), chw(routed[1]), chw(den_up), chw(den_lo),
            mask(den_up), mask(den_lo), chw(batch['retain_mask']), skin, label, bound)


# ------------------------------------------------------------------------------------------------------------- one batch

def _routing_samples(batch):
    """The samples of ``normalize_batch``; an outfit batch's carry the lower clothes' key points as an eighth entry."""
    sl = batch['sleeve']
    lower = [(kp,) for kp in batch['lower_kp']] if 'lower_kp' in batch else [()] * len(batch['person_name'])
    return [(batch['upper_img'][i], batch['lower_img'][i], batch['upper_mask'][i], batch['lower_mask'][i], None if sl is None else sl[i],
             batch['clothes_kp'][i], batch['person_kp'][i]) + lower[i] for i in range(len(batch['person_name']))]


def upload(batch, device):
    """The tensors of a (pinned) ``collate_unrouted`` batch on `device`, asynchronously."""
    return {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def route(batch, part):
    """``normalize_batch`` of an uploaded batch, then the row extents of the canvas the mode's bound rule reads."""
    dev = batch['image'].device
    samples = _routing_samples(batch) if dev.type == 'cuda' else [tuple(t.numpy() if isinstance(t, torch.Tensor) else t for t in s)
                                                                  for s in _routing_samples(batch)]
    routed = patch_routing.normalize_batch(samples, 2, device=dev, part=part)
    return routed, row_extents(_canvases(batch, routed, part)[2])


def batch_inputs(batch, routed, extents, part):
    """The generator's keyword arguments: pg_tryon_inputs on a GPU, ``to_generator_inputs`` of the rebuilt loader tuple on the CPU."""
    if batch['image'].device.type != 'cuda':
        return ds_mod.to_generator_inputs(loader_tuple(batch, routed, extents, part), 'cpu')
    den_up, den_lo, _ = _canvases(batch, routed, part)
    return generator_inputs(batch, routed[0], routed[1], den_up, den_lo, extents, part)


def pack(finetune_img, batch, part):
    """The result image of a batch: the triptych, or in the outfit mode the four panels upper clothes | lower clothes | person | result."""
    if part == 'outfit':
        return panels(finetune_img, (batch['clothes'], batch['lower_clothes'], batch['image']))
    return triptych(finetune_img, batch['clothes'], batch['image'])


def tryon_batch(batch, G, part):
    """One uploaded batch -> triptych uint8 [N, 512, 960, 3] (outfit: the four panels, [N, 512, 1280, 3]) on the batch's device (routing, inputs,
    generator, packing)."""
    routed, ext = route(batch, part)
    inp = batch_inputs(batch, routed, ext, part)
    with torch.no_grad():
        _, finetune_img, _ = G(**inp, noise_mode='const')
    return pack(finetune_img, batch, part)


# ------------------------------------------------------------------------------------------------------------- driver

def build_generator(snapshot, device='cpu'):
    """G_ema of a reference snapshot (path or binary file object) as this package's ``GeneratorFull_v20``, built from the snapshot's ``init_kwargs``
    (what the reference's train.py:191-202 writes, plus c_dim / img_resolution / img_channels) and loaded strictly by name.  Nothing in the file is
    executed (training/checkpoint.py)."""
    snap = checkpoint.read_snapshot(snapshot)
    g = snap.get('G_ema') if isinstance(snap, dict) else None
    if not isinstance(g, checkpoint.ModuleState):
        raise ValueError('the snapshot holds no G_ema network')
    if g.class_name != 'GeneratorFull_v20':
        raise ValueError(f'G_ema is a {g.class_name}; the try-on driver runs GeneratorFull_v20 only')
    plain = lambda v: {k: plain(x) for k, x in v.items()} if isinstance(v, dict) else v
    G = networks.GeneratorFull_v20(*g.init_args, **plain(dict(g.init_kwargs)))
    checkpoint.load_into(G, g, strict=True)
    return G.eval().requires_grad_(False).to(device)


class _Unrouted(torch.utils.data.Dataset):
    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        return self.dataset.unrouted(idx)


class _Raw(_Unrouted):
    def __getitem__(self, idx):
        return self.dataset.raw(idx)


FRONTS = ('host', 'native')
PRECISIONS = {'fp32': None, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def result_name(person_name, clothes_name, lower_name=None):
    """test.py:183-186: the base names without their 4-character extensions; the outfit mode appends the lower clothes' (person___upper___lower.png)."""
    base = lambda name: name.split('/')[-1][:-4]
    return '___'.join([base(person_name), base(clothes_name)] + ([] if lower_name is None else [base(lower_name)])) + '.png'


def _write_png(path, rgb):
    import PIL.Image
    PIL.Image.fromarray(rgb, 'RGB').save(path, compress_level=1)


def run_tryon(dataset, G, outdir, batch_size=1, device='cuda', workers=0, stats=None, front='host', precision='fp32'):
    """Try every pair of `dataset` (a ``TryOnTestSet``; its ``part`` picks the mode) on generator `G`, writing one PNG per pair into `outdir`.
    Returns the list of files written, in pair order.  `front` picks who builds the pre-routing maps: 'host' -- the loader's workers
    (``TryOnTestSet.unrouted``); 'native' -- the workers only decode (``TryOnTestSet.raw``) and ``tryon_front.front_batch`` builds the maps on the
    device, between the upload and the routing (same images, byte for byte).  `stats`, a dict, receives per-batch host seconds waiting for the
    loader ('load_s'), and on a GPU per-batch CUDA events ('events': (start, routed, inputs, generated, packed) per batch; with the native front
    (start, front, routed, inputs, generated, packed)) -- read them after the call.  `precision`: 'fp32' -- the reference's arithmetic --, or 'bf16' / 'fp16':
    the generator's blocks from 64^2 up run in that type for this call (``GeneratorFull_v20.set_half``; GPU only, a CPU run computes in float32 whatever
    it says); the generator's own setting is put back afterwards."""
    if front not in FRONTS:
        raise ValueError(f'front must be one of {FRONTS}, not {front!r}')
    if precision not in PRECISIONS:
        raise ValueError(f'precision must be one of {tuple(PRECISIONS)}, not {precision!r}')
    before = (G.synthesis.half_dtype, G.synthesis.half_from_res)
    G.set_half(PRECISIONS[precision])
    try:
        return _run_tryon(dataset, G, outdir, batch_size, device, workers, stats, front)
    finally:
        G.set_half(*before)


def _run_tryon(dataset, G, outdir, batch_size, device, workers, stats, front):
    native = front == 'native'
    if native:
        from . import tryon_front
    dev = torch.device(device)
    cuda = dev.type == 'cuda'
    os.makedirs(outdir, exist_ok=True)
    loader = torch.utils.data.DataLoader((_Raw if native else _Unrouted)(dataset), batch_size=batch_size, shuffle=False, num_workers=workers,
                                         collate_fn=ds_mod.collate_raw if native else ds_mod.collate_unrouted, pin_memory=cuda)
    written = []
    pending = []

    def flush(pool, item):                                # wait for one batch's bytes, then hand its PNGs to the pool
        done, host, names = item
        if done is not None:
            done.synchronize()
        arr = host.numpy()
        for i, pair in enumerate(names):
            path = os.path.join(outdir, result_name(*pair))
            pending.append(pool.submit(_write_png, path, arr[i]))
            written.append(path)

    import time
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        inflight = None
        it = iter(loader)
        while True:
            t0 = time.perf_counter()
            host_batch = next(it, None)
            if stats is not None and host_batch is not None:
                stats.setdefault('load_s', []).append(time.perf_counter() - t0)
            if host_batch is None:
                break
            names = list(zip(host_batch['person_name'], host_batch['clothes_name'], *([host_batch['lower_name']] if 'lower_name' in host_batch else [])))
            if cuda:
                with torch.cuda.device(dev):
                    ev = []

                    def mark():
                        if stats is not None:
                            ev.append(torch.cuda.Event(enable_timing=True))
                            ev[-1].record()
                    mark()
                    batch = upload(host_batch, dev)
                    if native:
                        batch = tryon_front.front_batch(batch, dataset.part)
                        mark()
                    routed, ext = route(batch, dataset.part)
                    mark()
                    inp = batch_inputs(batch, routed, ext, dataset.part)
                    mark()
                    with torch.no_grad():
                        _, finetune_img, _ = G(**inp, noise_mode='const')
                    mark()
                    trip = pack(finetune_img, batch, dataset.part)
                    mark()
                    if stats is not None:
                        stats.setdefault('events', []).append(ev)
                    host = torch.empty(trip.shape, dtype=torch.uint8, pin_memory=True)
                    host.copy_(trip, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record()
                item = (done, host, names)
            else:
                item = (None, tryon_batch(tryon_front.front_batch(host_batch, dataset.part) if native else host_batch, G, dataset.part), names)
            if inflight is not None:                      # the previous batch's copy has had this batch's whole enqueue to land
                flush(pool, inflight)
            inflight = item
        if inflight is not None:
            flush(pool, inflight)
        for f in pending:
            f.result()
    return written


# ------------------------------------------------------------------------------------------------------------- command line

def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Try garments on people with a PASTA-GAN++ snapshot (the reference\'s test.py).')
    p.add_argument('--network', required=True, help='network-snapshot-*.pkl (read without executing anything in it)')
    p.add_argument('--dataroot', required=True, help='test data directory (image/, parsing/, garment_parsing/, keypoints/, the pairs file)')
    p.add_argument('--testtxt', default='test_pairs.txt', help='pairs file in --dataroot: "<clothes> <person>" per line ("<upper> <lower> <person>" with '
                   '--testpart outfit)')
    p.add_argument('--testpart', required=True, choices=sorted(MODE_CODE), help='what is transferred: upper garment, lower garment, the full outfit of one '
                   'clothes image, or (outfit) the top of one clothes image and the lower garment of another')
    p.add_argument('--batchsize', type=int, default=1)
    p.add_argument('--use-sleeve-mask', action='store_true')
    p.add_argument('--outdir', required=True, help='where the PNGs go')
    p.add_argument('--device', default='cuda', help="'cuda', 'cuda:<i>' or 'cpu' (plain torch and NumPy)")
    p.add_argument('--workers', type=int, default=0, help='DataLoader worker processes (the reference uses 0)')
    p.add_argument('--precision', choices=sorted(PRECISIONS), default='fp32', help="arithmetic of the generator's blocks from 64x64 up on a GPU: 'fp32' (the "
                   "reference's), 'bf16' (recommended 16-bit type) or 'fp16'")
    p.add_argument('--front', choices=FRONTS, default='host', help="who builds the pre-routing maps: the loader's workers ('host') or the device "
                   "('native': the workers only decode the files)")
    # accepted for the reference's command lines; the reference ignores them for try-on, and so does this driver
    p.add_argument('--seeds', help='ignored (as in the reference)')
    p.add_argument('--trunc', type=float, default=1.0, help='ignored (as in the reference)')
    p.add_argument('--class', dest='class_idx', type=int, help='ignored (as in the reference)')
    p.add_argument('--noise-mode', choices=['const', 'random', 'none'], default='const', help="ignored (as in the reference: always 'const')")
    p.add_argument('--projected-w', help='ignored (as in the reference)')
    args = p.parse_args(argv)
    if args.batchsize < 1:
        p.error('--batchsize must be at least 1')
    return args


def main(argv=None):
    args = parse_args(argv)
    print(f'Loading networks from "{args.network}"...')
    G = build_generator(args.network, args.device)
    dataset = ds_mod.TryOnTestSet(args.dataroot, test_txt=args.testtxt, use_sleeve_mask=args.use_sleeve_mask, part=args.testpart)
    files = run_tryon(dataset, G, args.outdir, batch_size=args.batchsize, device=args.device, workers=args.workers, front=args.front,
                      precision=args.precision)
    print(f'wrote {len(files)} images to {args.outdir}')
    return files
