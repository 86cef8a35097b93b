"""The data fetch of the training loop (reference training_loop_fullbody.py:549-601): `TrainSet` items in, `TrainingStep` rounds out.

Per iteration, on a GPU:

1. ``TrainSet.unrouted`` items (a DataLoader over ``misc.InfiniteSampler`` with `workers` processes, ``collate_train``, pinned) are uploaded
   asynchronously;
2. ``patch_routing.normalize_batch(..., part='train')`` routes the whole batch (three native launches);
3. ``pg_tryon_row_extent_u8`` finds the first row of every sample's routed lower mask of part 0 (one launch), and ``pg_train_fetch`` writes the nine
   float32 tensors of the rounds (one launch): the erase decision of every sample and its random mask are applied while the bytes are read;
4. ``gen_z`` is drawn, and the batch is split into `rounds` dicts keyed as ``StyleGAN2Loss.accumulate_gradients`` names its arguments.

Nothing between the DataLoader's hand-over and the returned tensors waits for the device.  ``device='cpu'`` runs the same flow through
``normalize_batch``'s NumPy route and `fetch_reference`.

`fetch_reference` is the reference's statements in torch, and what the kernel is tested against (tests/test_train_fetch_gpu.py).  The reference
runs them on a GPU, where torch computes ``u / 127.5`` as ``u * (1.0f / 127.5f)``; on CPU tensors `fetch_reference` writes that product out, so both
routes give the same bits (the rule of training/tryon.py)."""

import contextlib
import ctypes

import numpy as np
import torch

from torch_utils import custom_ops
from torch_utils import misc
from torch_utils.ops import _native as nat
from . import dataset as ds_mod
from . import patch_routing
from . import tryon

_INV = np.float32(1.0) / np.float32(127.5)            # torch's GPU `t / 127.5` multiplies by this
KEYS = ('real_img', 'style_input', 'retain', 'pose', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask', 'denorm_lower_mask', 'gt_parsing')

launch_counter = None     # a dict(fetch=0) counts the launches of pg_train_fetch (tests, tools/train_fetch_bench.py); row extents: tryon.launch_counter


class TrainIO(ctypes.Structure):
    """Mirror of ``pg_train_io`` (include/pasta_gan_ops.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in ('image', 'pose', 'retain_mask', 'gt_parsing', 'random_mask', 'denorm_upper', 'denorm_lower', 'norm_img',
                                                     'norm_img_lower', 'skin', 'label', 'bound_rows', 'extents', 'erase', 'band_u', 'real_img', 'style_input',
                                                     'retain', 'pose_out', 'denorm_upper_out', 'denorm_lower_out', 'upper_mask_out', 'lower_mask_out',
                                                     'gt_parsing_out')]


_plugin = None


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('train_fetch_plugin')
        plugin.lib.pg_train_fetch.restype = ctypes.c_int
        plugin.lib.pg_train_fetch.argtypes = [ctypes.POINTER(TrainIO)] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        _plugin = plugin
    return _plugin


def lower_mask_extents(routed):
    """int32 [N, 2]: first / last non-zero row of every sample's routed lower mask of part 0 (the channels of a routed mask are equal, so the first
    row is the reference's ``mask_to_bbox(...)[1]``, dataset.py:1146-1147), -1 / -1 when it is empty."""
    return tryon.row_extents(routed[5][..., 0:3].contiguous())


def _check(name, t, dev, dtype, shape):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise nat.NativeOpError(f'train_fetch: {name} must be a contiguous {dtype} tensor of shape {list(shape)} on {dev}')


def fetch(batch, routed, extents):
    """The nine float32 tensors of `KEYS` for an uploaded ``collate_train`` batch and its routing, in ONE launch of pg_train_fetch -- bit for bit
    what `fetch_reference` computes on the GPU.  routed: the six results of ``normalize_batch(part='train')``; extents: `lower_mask_extents`."""
    image = batch['image']
    dev = image.device
    if dev.type != 'cuda':
        raise nat.NativeOpError('train_fetch: fetch() runs pg_train_fetch on GPU tensors; CPU batches go through fetch_reference()')
    if image.dim() != 4:
        raise nat.NativeOpError('train_fetch: image must be [N, H, W, 3]')
    n, H, W, _ = image.shape
    norm_img, norm_img_lower, denorm_upper, denorm_lower = routed[:4]
    h, w = int(norm_img.shape[1]), int(norm_img.shape[2])
    if W % 4 or w % 4:
        raise nat.NativeOpError(f'train_fetch: widths must be multiples of 4 (W = {W}, w = {w})')
    u8, i32, f32 = torch.uint8, torch.int32, torch.float32
    for name, t, dtype, shape in (('image', image, u8, (n, H, W, 3)), ('pose', batch['pose'], u8, (n, H, W, 3)),
                                  ('retain_mask', batch['retain_mask'], u8, (n, H, W, 1)), ('gt_parsing', batch['gt_parsing'], u8, (n, H, W, 1)),
                                  ('random_mask', batch['random_mask'], u8, (n, H, W, 1)), ('denorm_upper', denorm_upper, u8, (n, H, W, 3)),
                                  ('denorm_lower', denorm_lower, u8, (n, H, W, 3)), ('norm_img', norm_img, u8, (n, h, w, 30)),
                                  ('norm_img_lower', norm_img_lower, u8, (n, h, w, 15)), ('skin', batch['skin'], f32, (n, 3)),
                                  ('label', batch['label'], i32, (n,)), ('bound_train', batch['bound_train'], u8, (n, H)), ('extents', extents, i32, (n, 2)),
                                  ('erase', batch['erase'], i32, (n, 4)), ('band_u', batch['band_u'], f32, (n,))):
        _check(name, t, dev, dtype, shape)
        if dtype == u8 and t.data_ptr() % 4:
            raise nat.NativeOpError(f'train_fetch: {name} must be dword-aligned')
    new = lambda *shape: torch.empty([n, *shape], dtype=f32, device=dev)
    out = dict(real_img=new(3, H, W), style_input=new(45, h, w), retain=new(6, H, W), pose=new(5, H, W), denorm_upper_input=new(3, H, W),
               denorm_lower_input=new(3, H, W), denorm_upper_mask=new(1, H, W), denorm_lower_mask=new(1, H, W), gt_parsing=new(1, H, W))
    p = lambda t: t.data_ptr()
    io = TrainIO(p(image), p(batch['pose']), p(batch['retain_mask']), p(batch['gt_parsing']), p(batch['random_mask']), p(denorm_upper), p(denorm_lower),
                 p(norm_img), p(norm_img_lower), p(batch['skin']), p(batch['label']), p(batch['bound_train']), p(extents), p(batch['erase']), p(batch['band_u']),
                 p(out['real_img']), p(out['style_input']), p(out['retain']), p(out['pose']), p(out['denorm_upper_input']), p(out['denorm_lower_input']),
                 p(out['denorm_upper_mask']), p(out['denorm_lower_mask']), p(out['gt_parsing']))
    with torch.cuda.device(dev):
        nat.check(_init().lib.pg_train_fetch(ctypes.byref(io), n, H, W, h, w, nat.stream_of(image)), 'pg_train_fetch')
    if launch_counter is not None:
        launch_counter['fetch'] += 1
    return out


def erase_lower(norm_img_lower, extents, erase, band_u):
    """``norm_img_lower_for_train`` (dataset.py:1146-1170) of a routed batch [N, h, w, 15] in torch, for the records `erase` int32 [N, 4] /
    `band_u` float32 [N] and the row extents of the routed lower masks; a sample whose mask is empty (extent -1) keeps its patches."""
    n, h = norm_img_lower.shape[:2]
    dev = norm_img_lower.device
    rows = torch.arange(h, dtype=torch.int32, device=dev)[None]                              # [1, h]
    ty = extents[:, 0:1].to(torch.int32)
    kind = torch.where(ty >= 0, erase[:, 0:1], torch.zeros_like(ty))
    by = ty + 1 + torch.floor(band_u[:, None] * (h - ty).to(torch.float32)).to(torch.int32)
    by = torch.minimum(by, torch.full_like(by, h))
    zero0 = (kind == ds_mod.ERASE_DROP_PART0) | ((kind == ds_mod.ERASE_BAND) & (rows >= ty) & (rows < by))       # [N, h]
    zero13 = (kind == ds_mod.ERASE_DROP_PART0) & (erase[:, 1:2] != 0) & (rows < erase[:, 2:3])
    never = torch.zeros_like(zero0)
    zero = torch.stack([zero0, zero13, never, zero13, never], dim=2)[..., None].expand(n, h, 5, 3).reshape(n, h, 15)
    return torch.where(zero[:, :, None, :], torch.zeros_like(norm_img_lower), norm_img_lower)


def loader_tuple(batch, routed, extents):
    """The entries of the ``TrainSet.__getitem__`` batch that the training loop reads (training_loop_fullbody.py:552-554), rebuilt in torch from an
    unrouted batch and its routing on the batch's device, as a dict (CHW; skin / label maps float64)."""
    chw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    n, H, W, _ = batch['image'].shape
    keep = 1 - chw(((batch['random_mask'] > 0) & (batch['erase'][:, 3] != 0)[:, None, None, None]).to(torch.uint8))
    upper, lower = chw(routed[2]) * keep, chw(routed[3]) * keep
    mask = lambda t: (t.to(torch.int32).sum(dim=1, keepdim=True) > 0).to(torch.uint8)
    return dict(image=chw(batch['image']), pose=chw(batch['pose']), norm_img=chw(routed[0]),
                norm_img_lower=chw(erase_lower(routed[1], extents, batch['erase'], batch['band_u'])), denorm_upper_img=upper, denorm_lower_img=lower,
                gt_parsing=chw(batch['gt_parsing']), denorm_upper_mask=mask(upper), denorm_lower_mask=mask(lower), retain_mask=chw(batch['retain_mask']),
                skin=batch['skin'].to(torch.float64)[:, :, None, None].expand(n, 3, H, W),
                lower_label_map=(batch['label'].to(torch.float64) / 2.0 * 255)[:, None, None, None].expand(n, 1, H, W),
                lower_clothes_upper_bound=batch['bound_train'][:, None, :, None].expand(n, 1, H, W))


def fetch_reference(batch, routed, extents=None):
    """training_loop_fullbody.py:556-580 in torch on the batch's device, from the rebuilt loader tuple: the nine tensors of `KEYS`."""
    if extents is None:
        extents = lower_mask_extents(routed)
    t = loader_tuple(batch, routed, extents)
    if batch['image'].device.type == 'cuda':
        unit = lambda x: x.to(torch.float32) / 127.5 - 1
    else:                                                     # the GPU's arithmetic for that statement, written out (module docstring)
        unit = lambda x: x.to(torch.float32) * float(_INV) - 1
    real = unit(t['image'])
    retain_mask = t['retain_mask']
    head = retain_mask * real - (1 - retain_mask)
    return dict(real_img=real, style_input=torch.cat([unit(t['norm_img']), unit(t['norm_img_lower'])], dim=1),
                retain=torch.cat([head, unit(t['skin'])], dim=1),
                pose=torch.cat([unit(t['pose']), unit(t['lower_label_map']), unit(t['lower_clothes_upper_bound'])], dim=1),
                denorm_upper_input=unit(t['denorm_upper_img']), denorm_lower_input=unit(t['denorm_lower_img']),
                denorm_upper_mask=t['denorm_upper_mask'].to(torch.float32), denorm_lower_mask=t['denorm_lower_mask'].to(torch.float32),
                gt_parsing=t['gt_parsing'].to(torch.float32))


# ------------------------------------------------------------------------------------------------------------- one iteration

def upload(batch, device):
    """The tensors of a (pinned) ``collate_train`` batch on `device`, asynchronously."""
    return {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def route(batch):
    """``normalize_batch(part='train')`` of an uploaded batch, then the row extents of the routed lower masks."""
    dev = batch['image'].device
    arr = (lambda t: t) if dev.type == 'cuda' else (lambda t: t.numpy())
    samples = [(arr(batch['upper_img'][i]), arr(batch['lower_img'][i]), arr(batch['upper_mask'][i]), arr(batch['lower_mask'][i]), arr(batch['sleeve'][i]),
                batch['person_kp'][i], batch['person_kp'][i]) for i in range(len(batch['name']))]
    routed = patch_routing.normalize_batch(samples, 2, device=dev, part='train')
    return routed, lower_mask_extents(routed)


def batch_tensors(batch):
    """An uploaded batch -> the nine tensors of `KEYS`: routing + pg_train_fetch on a GPU, routing + `fetch_reference` on the CPU."""
    routed, ext = route(batch)
    if batch['image'].device.type == 'cuda':
        return fetch(batch, routed, ext)
    return fetch_reference(batch, routed, ext)


class _Unrouted(torch.utils.data.Dataset):
    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        return self.dataset.unrouted(idx)


class TrainFeed:
    """An endless iterator of ``TrainingStep.run`` arguments: every ``next()`` loads `batch_gpu * rounds` items of `dataset` (a ``TrainSet``) for this
    rank and returns a list of `rounds` dicts (the nine tensors of `KEYS` plus ``gen_z`` [batch_gpu, z_dim]) on `device`."""

    def __init__(self, dataset, batch_gpu, rounds=1, rank=0, world=1, seed=0, workers=0, device='cuda', z_dim=0, shuffle=True):
        self.device = torch.device(device)
        self.batch_gpu, self.rounds, self.z_dim = int(batch_gpu), int(rounds), int(z_dim)
        cuda = self.device.type == 'cuda'
        sampler = misc.InfiniteSampler(dataset, rank=rank, num_replicas=world, shuffle=shuffle, seed=seed)
        self.loader = iter(torch.utils.data.DataLoader(_Unrouted(dataset), sampler=sampler, batch_size=self.batch_gpu * self.rounds, num_workers=workers,
                                                       collate_fn=ds_mod.collate_train, pin_memory=cuda, prefetch_factor=2 if workers else None))
        self.gen = torch.Generator(device=self.device).manual_seed(seed * world + rank)

    def __iter__(self):
        return self

    def feed(self, host_batch):
        """One ``collate_train`` batch -> the list of rounds (no host synchronisation on a GPU)."""
        with torch.cuda.device(self.device) if self.device.type == 'cuda' else contextlib.nullcontext():
            out = batch_tensors(upload(host_batch, self.device))
            out['gen_z'] = torch.randn([self.batch_gpu * self.rounds, self.z_dim], device=self.device, generator=self.gen)
        split = {k: v.split(self.batch_gpu) for k, v in out.items()}
        return [{k: v[r] for k, v in split.items()} for r in range(self.rounds)]

    def __next__(self):
        return self.feed(next(self.loader))
