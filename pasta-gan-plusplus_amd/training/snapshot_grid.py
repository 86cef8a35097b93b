"""The image snapshots of the training driver (reference training_loop_fullbody.py:77-342 ``denorm_clothes`` / ``setup_snapshot_image_grid`` /
``save_image_grid``, :489-519, :700-719): every visualisation person dressed in every visualisation person's garments, as a gnum x gnum grid with
the persons along the left column and the top row.

Cell i (col = i % gnum, row = i // gnum, gap = gnum // 3) shows person `row`; rows below `gap` swap the lower garment (upper garment of U = row,
lower of L = col), rows below 2 gap the full outfit (U = L = col), the rest the upper garment (U = col, L = row).  Every warp goes through the
person's own ``Ms`` / ``M_invs``; a part whose ``M_inv`` sums to zero contributes nothing.

The reference builds this on the host with ~43 ``cv2.warpPerspective`` calls per cell.  Here, on a GPU, `setup_snapshot_grid` routes the gnum persons with
``normalize_batch(part='train')`` and then runs

* ONE launch of ``pg_patch_denorm_u8`` (csrc/patch_routing.hip; 8 x 8 erode) for every canvas of the grid -- 128 x 128 patches straight to the 512 x 512
  canvases, without the warped intermediates.  Canvases that do not depend on the column (``denorm_upper`` of the lower-garment rows, ``denorm_lower`` of
  the upper-garment rows) are computed once and shared;
* two ``pg_warp_perspective_u8`` launches for the round trip of the lower patches (``patch_lower * (1 - (mask_upper > 0))`` to 512 x 512 and back), two
  more for the bound rules of the full-outfit and upper-garment rows, and two ``pg_tryon_row_extent_u8`` launches for their row extents.

The state kept is uint8, on the device: per person the image, pose map, retain mask, skin medians, label and the two bound rows; per cell the indices of
its two canvases, the 45 channels of style patches, the bound row and the label.  `SnapshotGrid.inputs` stages a chunk's seven float32 generator inputs
with ``pg_tryon_inputs`` in its rows-as-they-are mode (the bound rows are final per cell); `SnapshotGrid.render` runs the generator chunk by chunk and
packs the outputs into the two device grids with ``pg_snapshot_cells_u8`` (csrc/snapshot_grid.hip).

``device='cpu'`` takes the same steps through NumPy / torch with the same arithmetic (``_warp_perspective_cpu``, ``_patch_compose_cpu_``); as in
training/tryon.py, ``u / 127.5`` is written as the product with the rounded reciprocal that torch computes on a GPU, so both routes give the same bits.

The parsing image is ``grey[first index of the maximal logit]``.  The reference takes ``argmax(softmax(x))``: the same index, except where softmax's
rounding merges distinct logits into equal probabilities (then the reference's choice depends on that rounding).  NaN in the
generator output becomes 0 (NumPy leaves that cast undefined)."""

import ctypes

import numpy as np
import torch

from torch_utils import custom_ops
from torch_utils.ops import _native as nat
from . import dataset as ds_mod
from . import patch_routing as P
from . import tryon

LOWER_IDS = (0, 6, 7, 8, 9)
KSIZE = 8                                             # training_loop_fullbody.py:84
MAX_GNUM = 14                                         # :216
CORNER = 128                                          # the top-left cell: ``torch.zeros`` in [-1, 1] (:504) -> rint(127.5) = 128, a mid grey
_INV = np.float32(1.0) / np.float32(127.5)            # torch's GPU `t / 127.5` multiplies by this

launch_counter = None     # a dict(denorm=0, cells=0) counts the launches of pg_patch_denorm_u8 / pg_snapshot_cells_u8 (tests, tools/snapshot_grid_bench.py)

_DENORM_DT = np.dtype([('canvas', 'u8'), ('patch', 'u8', (10,)), ('mask', 'u8', (10,)), ('minv', 'f8', (10, 9)), ('nparts', 'i4'), ('pad_', 'i4')])


class DenormJob(ctypes.Structure):
    """Mirror of ``pg_denorm_job`` (include/pasta_gan_ops.h)."""
    _fields_ = [('canvas', ctypes.c_void_p), ('patch', ctypes.c_void_p * 10), ('mask', ctypes.c_void_p * 10), ('minv', ctypes.c_double * 9 * 10),
                ('nparts', ctypes.c_int), ('pad_', ctypes.c_int)]


assert _DENORM_DT.itemsize == ctypes.sizeof(DenormJob)

_cells_plugin = None


def _routing_lib():
    lib = P._init().lib
    lib.pg_patch_denorm_u8.restype = ctypes.c_int
    lib.pg_patch_denorm_u8.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    return lib


def _cells_lib():
    global _cells_plugin
    if _cells_plugin is None:
        plugin = custom_ops.get_plugin('snapshot_grid_plugin')
        plugin.lib.pg_snapshot_cells_u8.restype = ctypes.c_int
        plugin.lib.pg_snapshot_cells_u8.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
        _cells_plugin = plugin
    return _cells_plugin.lib


def _count(name):
    if launch_counter is not None:
        launch_counter[name] += 1


def _to_dev(values, dtype, dev):
    """A host list as a tensor on `dev`: through pinned memory, asynchronously, on a GPU."""
    t = torch.tensor(values, dtype=dtype)
    return t.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' else t


# ------------------------------------------------------------------------------------------------------------- arithmetic of save_image_grid

def grey_table(classes=7):
    """The bytes ``save_image_grid`` writes for parsing index k: the reference's float32 statements ``k / 6 * 2 - 1`` (training_loop_fullbody.py:717),
    then ``rint((v + 1) * 127.5)`` clipped (:316-317).  Seven classes: [0, 43, 85, 128, 170, 212, 255]."""
    k = np.arange(classes, dtype=np.float32)
    v = k / 6 * 2 - 1.0
    return image_bytes(v)


def image_bytes(x):
    """``save_image_grid``'s conversion for drange [-1, 1] (:314-317) of a float array: float32 ``(x + 1) * 127.5``, rint (half to even), clip, uint8;
    NaN -> 0."""
    v = (np.asarray(x, dtype=np.float32) - np.float32(-1)) * np.float32(255 / 2)
    with np.errstate(invalid='ignore'):
        v = np.rint(v).clip(0, 255)
    return np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)


def cells_numpy(finetune_img, pred_parsing, grey):
    """The bytes of a chunk's cells in NumPy: float32 [n, 3, H, W], [n, C, H, W] -> two uint8 [n, H, W, 3]."""
    img = image_bytes(finetune_img).transpose(0, 2, 3, 1)
    logits = np.asarray(pred_parsing, dtype=np.float32)
    logits = np.where(np.isnan(logits), np.float32(-np.inf), logits)                       # a NaN logit never wins (np.argmax alone would pick it)
    par = np.asarray(grey)[np.argmax(logits, axis=1)]                                      # np.argmax: the first index of the maximum
    return np.ascontiguousarray(img), np.ascontiguousarray(np.repeat(par[..., None], 3, axis=3))


def pack_cells(finetune_img, pred_parsing, grey, grid_img, grid_parsing, first_cell, gh, gw):
    """Write cells first_cell .. first_cell + n - 1 of the two uint8 grid images [(gh + 1) H, (gw + 1) W, 3] in place.  GPU: one launch of
    pg_snapshot_cells_u8; CPU: `cells_numpy`."""
    n, _, H, W = finetune_img.shape
    C = int(pred_parsing.shape[1])
    if finetune_img.device.type != 'cuda':
        img, par = cells_numpy(finetune_img.detach().numpy(), pred_parsing.detach().numpy(), grey.numpy())
        for k in range(n):
            r, c = 1 + (first_cell + k) // gw, 1 + (first_cell + k) % gw
            grid_img[r * H:(r + 1) * H, c * W:(c + 1) * W] = torch.from_numpy(img[k])
            grid_parsing[r * H:(r + 1) * H, c * W:(c + 1) * W] = torch.from_numpy(par[k])
        return
    dev = finetune_img.device
    fin = finetune_img.detach().to(torch.float32).contiguous()
    par = pred_parsing.detach().to(torch.float32).contiguous()
    for name, g in (('grid_img', grid_img), ('grid_parsing', grid_parsing)):
        if not (g.dtype == torch.uint8 and g.device == dev and g.is_contiguous() and tuple(g.shape) == ((gh + 1) * H, (gw + 1) * W, 3)):
            raise nat.NativeOpError(f'snapshot_grid: {name} must be a contiguous uint8 [{(gh + 1) * H}, {(gw + 1) * W}, 3] tensor on {dev}')
    if not (grey.dtype == torch.uint8 and grey.device == dev and grey.numel() == C and tuple(par.shape) == (n, C, H, W) and fin.shape[1] == 3):
        raise nat.NativeOpError('snapshot_grid: grey must hold one byte per parsing class on the images\' device; finetune_img must have 3 channels')
    with torch.cuda.device(dev):
        nat.check(_cells_lib().pg_snapshot_cells_u8(fin.data_ptr(), par.data_ptr(), grey.data_ptr(), grid_img.data_ptr(), grid_parsing.data_ptr(), n, C, H, W,
                                                    gh, gw, int(first_cell), nat.stream_of(fin)), 'pg_snapshot_cells_u8')
    _count('cells')


def save_png(path, array):
    """Write a uint8 HWC (RGB) array as a PNG."""
    import PIL.Image
    PIL.Image.fromarray(np.ascontiguousarray(array), 'RGB').save(path)


# ------------------------------------------------------------------------------------------------------------- device primitives


def warp_batch(srcs, forwards, wh, taps=None):
    """``cv2.warpPerspective(srcs[j], forwards[j], wh)`` of same-sized uint8 [sh, sw, 3] tensors in one launch -> uint8 [J, h, w, 3].  `taps`: the CPU route's
    per-matrix cache (a dict the caller owns; `_warp_perspective_cpu`)."""
    w, h = wh
    dev = srcs[0].device
    if dev.type != 'cuda':
        return torch.stack([P._warp_perspective_cpu(s, m, wh, taps) for s, m in zip(srcs, forwards)])
    out = torch.empty([len(srcs), h, w, 3], dtype=torch.uint8, device=dev)
    t = np.zeros(len(srcs), dtype=P._WARP_DT)
    t['src'], t['dst'] = [s.data_ptr() for s in srcs], [out.data_ptr() + j * h * w * 3 for j in range(len(srcs))]
    t['src_h'], t['src_w'], t['dst_h'], t['dst_w'], t['channels'], t['block_w'] = srcs[0].shape[0], srcs[0].shape[1], h, w, 3, P._block_width(h, w)
    t['minv'] = np.stack([P.invert3x3(m).reshape(9) for m in forwards])
    tab = P._upload_table(t, dev)
    with torch.cuda.device(dev):
        nat.check(P._init().lib.pg_warp_perspective_u8(tab.data_ptr(), len(srcs), h * w, nat.stream_of(out)), 'pg_warp_perspective_u8')
    return out


def denorm_canvases(jobs, H, W, ksize=KSIZE, taps=None):
    """The fused warp, erode and ordered paste: jobs = list of part lists [(patch uint8 [ph, pw, 3], mask uint8 [ph, pw, mc], forward 3x3), ...] in paste
    order (up to 10 parts; at least one job has a part) -> uint8 [len(jobs), H, W, 3].  GPU: ONE launch of pg_patch_denorm_u8; CPU: warp +
    erode-and-paste per part in NumPy."""
    first = next(p for parts in jobs for p in parts)
    dev = first[0].device
    ph, pw = int(first[0].shape[0]), int(first[0].shape[1])
    mc = int(first[1].shape[2])
    out = torch.empty([len(jobs), H, W, 3], dtype=torch.uint8, device=dev)
    if dev.type != 'cuda':
        for j, parts in enumerate(jobs):
            out[j] = 0
            for patch, mask, m in parts:
                P._patch_compose_cpu_(out[j], P._warp_perspective_cpu(patch, m, (W, H), taps),
                                      P._warp_perspective_cpu(mask[:, :, 0].contiguous(), m, (W, H), taps), None, ksize)
        return out
    t = np.zeros(len(jobs), dtype=_DENORM_DT)
    for j, parts in enumerate(jobs):
        if len(parts) > 10:
            raise nat.NativeOpError('snapshot_grid: at most 10 parts per canvas')
        t[j]['canvas'], t[j]['nparts'] = out.data_ptr() + j * H * W * 3, len(parts)
        for k, (patch, mask, m) in enumerate(parts):
            if not (patch.is_contiguous() and mask.is_contiguous() and tuple(patch.shape) == (ph, pw, 3) and tuple(mask.shape) == (ph, pw, mc)):
                raise nat.NativeOpError('snapshot_grid: patches and masks must be contiguous and of one size')
            t[j]['patch'][k], t[j]['mask'][k], t[j]['minv'][k] = patch.data_ptr(), mask.data_ptr(), P.invert3x3(m).reshape(9)
    tab = P._upload_table(t, dev)
    with torch.cuda.device(dev):
        nat.check(_routing_lib().pg_patch_denorm_u8(tab.data_ptr(), len(jobs), H, W, ph, pw, mc, int(ksize), P._block_width(H, W), nat.stream_of(out)),
                  'pg_patch_denorm_u8')
    _count('denorm')
    return out


# ------------------------------------------------------------------------------------------------------------- the grid

def cell_sources(i, gnum):
    """(row, col, U, L, mode) of cell i: the person, and whose upper / lower garment they wear (training_loop_fullbody.py:89-119)."""
    col, row, gap = i % gnum, i // gnum, gnum // 3
    if row < gap:
        return row, col, row, col, 'lower'
    if row < 2 * gap:
        return row, col, col, col, 'full'
    return row, col, col, row, 'upper'


class SnapshotGrid:
    """What `setup_snapshot_grid` keeps (module docstring).  `canvases` uint8 [K, H, W, 3] with `upper_index` / `lower_index` [gnum^2] into it;
    `norm_img` [gnum^2, h, w, 30], `norm_img_lower` [gnum^2, h, w, 15], `bound` [gnum^2, H], `label` int32 [gnum^2]; `persons`: image, pose [gnum, H, W, 3],
    retain_mask [gnum, H, W, 1], skin float32 [gnum, 3], label int32 [gnum], gt_rows / bound_test uint8 [gnum, H], gt_parsing uint8 [gnum, H, W, 1] (the
    loader's 7-class map: the label windows of training/metrics.py); `person_index` [gnum^2]."""

    def __init__(self, gnum, device, persons, canvases, upper_index, lower_index, norm_img, norm_img_lower, bound, label, person_index):
        self.gnum, self.device, self.persons = gnum, device, persons
        self.canvases, self.upper_index, self.lower_index = canvases, upper_index, lower_index
        self.norm_img, self.norm_img_lower, self.bound, self.label, self.person_index = norm_img, norm_img_lower, bound, label, person_index
        self.H, self.W = int(persons['image'].shape[1]), int(persons['image'].shape[2])
        self._grey = {}
        base = torch.zeros([gnum + 1, self.H, gnum + 1, self.W, 3], dtype=torch.uint8, device=device)
        base[1:, :, 0] = persons['image']                                                    # left column
        base[0, :, 0] = CORNER                                                               # the top row starts with the reference's float 0 cell
        base[0, :, 1:] = persons['image'].permute(1, 0, 2, 3)
        # (the side and top cells are never written again: each grid is its own base)
        self.grid_img = base.reshape((gnum + 1) * self.H, (gnum + 1) * self.W, 3)
        self.grid_parsing = self.grid_img.clone()

    def __len__(self):
        return self.gnum * self.gnum

    def upper_canvases(self, lo=0, hi=None):
        return self.canvases.index_select(0, self.upper_index[lo:hi])

    def lower_canvases(self, lo=0, hi=None):
        return self.canvases.index_select(0, self.lower_index[lo:hi])

    def canvas_grids(self):
        """``init_denorm_upper.png`` / ``init_denorm_lower.png``: the canvases in the grid layout, uint8 HWC NumPy arrays."""
        out = []
        g = self.gnum
        for cells in (self.upper_canvases(), self.lower_canvases()):
            grid = self.grid_img.clone().reshape(g + 1, self.H, g + 1, self.W, 3)     # (its side and top cells; every other cell is written)
            grid[1:, :, 1:] = cells.reshape(g, g, self.H, self.W, 3).permute(0, 2, 1, 3, 4)
            out.append(grid.reshape(self.grid_img.shape).cpu().numpy())
        return out

    def inputs(self, lo, hi):
        """The keyword arguments of ``GeneratorFull_v20.forward`` for cells lo .. hi - 1 (float32, on the grid's device)."""
        pidx = self.person_index[lo:hi]
        pp = self.persons
        src = dict(image=pp['image'].index_select(0, pidx), pose=pp['pose'].index_select(0, pidx), retain_mask=pp['retain_mask'].index_select(0, pidx),
                   skin=pp['skin'].index_select(0, pidx), label=self.label[lo:hi], bound=self.bound[lo:hi])
        den_up, den_lo = self.upper_canvases(lo, hi), self.lower_canvases(lo, hi)
        n = hi - lo
        if self.device.type == 'cuda':
            ext = torch.zeros([n, 2], dtype=torch.int32, device=self.device)                   # not read: the rows are taken as they are
            return tryon.generator_inputs(src, self.norm_img[lo:hi], self.norm_img_lower[lo:hi], den_up, den_lo, ext, 'lower')
        return inputs_torch(src, self.norm_img[lo:hi], self.norm_img_lower[lo:hi], den_up, den_lo)

    def grey(self, classes):
        if classes not in self._grey:
            self._grey[classes] = torch.from_numpy(grey_table(classes)).to(self.device)
        return self._grey[classes]

    def render(self, G_ema, batch_gpu, timer=None):
        """Run `G_ema` over the cells in chunks of `batch_gpu` (``noise_mode='const'``, no gradients) and pack the outputs into the two grids ->
        (finetune grid, parsing grid), uint8 HWC NumPy arrays of side (gnum + 1) * 512.  `timer(name)`, if given, is called after each chunk's 'inputs',
        'generator' and 'cells' step."""
        g = self.gnum
        with torch.no_grad():
            for lo in range(0, g * g, batch_gpu):
                hi = min(lo + batch_gpu, g * g)
                inp = self.inputs(lo, hi)
                timer and timer('inputs')
                _, finetune_img, pred_parsing = G_ema(**inp, noise_mode='const')
                timer and timer('generator')
                pack_cells(finetune_img, pred_parsing, self.grey(int(pred_parsing.shape[1])), self.grid_img, self.grid_parsing, lo, g, g)
                timer and timer('cells')
        return self.grid_img.cpu().numpy(), self.grid_parsing.cpu().numpy()


def inputs_torch(src, norm_img, norm_img_lower, den_up, den_lo):
    """What pg_tryon_inputs computes in its rows-as-they-are mode, in torch (the CPU route): ``u / 127.5 - 1`` as the GPU's product."""
    unit = lambda t: t.to(torch.float32) * float(_INV) - 1
    chw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    n, H, W, _ = src['image'].shape
    m = chw(src['retain_mask']).to(torch.float32)
    plane = lambda v: v.to(torch.float32)[:, :, None, None].expand(n, v.shape[1], H, W)
    label = (src['label'].to(torch.float32) * 127.5)[:, None]
    bound = src['bound'].to(torch.float32)[:, None, :, None].expand(n, 1, H, W)
    mask = lambda t: (chw(t).to(torch.int32).sum(dim=1, keepdim=True) > 0).to(torch.float32)
    return dict(z=torch.zeros([n, 0], device=src['image'].device), c=torch.cat([unit(chw(norm_img)), unit(chw(norm_img_lower))], dim=1),
                retain=torch.cat([unit(chw(src['image'])) * m - (1 - m), unit(plane(src['skin']))], dim=1),
                pose=torch.cat([unit(chw(src['pose'])), unit(plane(label)), unit(bound)], dim=1).contiguous(),
                denorm_upper_input=unit(chw(den_up)), denorm_lower_input=unit(chw(den_lo)), denorm_upper_mask=mask(den_up), denorm_lower_mask=mask(den_lo))


def setup_snapshot_grid(training_set, device, gnum=None):
    """The snapshot grid of `training_set` (a ``TrainSet`` with at least 3 entries in ``vis_index``) on `device`: the first `gnum` visualisation persons
    (default: min(14, len(vis_index))).  None of the tuple fields read depends on the loader's erase record: the grid is a function of the dataset."""
    dev = torch.device(device)
    if gnum is None:
        gnum = min(MAX_GNUM, len(training_set.vis_index))
    if gnum < 3 or gnum > len(training_set.vis_index):
        raise ValueError(f'snapshot_grid: gnum = {gnum} needs 3 <= gnum <= len(vis_index) = {len(training_set.vis_index)}')
    g, gap = gnum, gnum // 3
    items = [training_set.unrouted(i, ds_mod.NO_ERASE) for i in training_set.vis_index[:g]]
    cuda = dev.type == 'cuda'
    taps = None if cuda else {}                               # the CPU route's warp taps per matrix; gone with this call
    batch = ds_mod.collate_train(items, pin=cuda)
    up = lambda k: batch[k].to(dev, non_blocking=True)
    arr = (lambda t: t) if cuda else (lambda t: t.numpy())
    samples = [(arr(up('upper_img')[i]), arr(up('lower_img')[i]), arr(up('upper_mask')[i]), arr(up('lower_mask')[i]), arr(up('sleeve')[i]),
                items[i]['person_kp'], items[i]['person_kp']) for i in range(g)]
    H, W = int(batch['image'].shape[1]), int(batch['image'].shape[2])
    with torch.cuda.device(dev) if cuda else torch.no_grad():
        img, img_lower, _, _, masks, masks_lower = P.normalize_batch(samples, 2, device=dev, part='train')
        h, w = int(img.shape[1]), int(img.shape[2])
        mats = [P.crop_matrices(it['person_kp'], H, W, 2) for it in items]
        Ms, M_invs = np.stack([m[0] for m in mats]), np.stack([m[1] for m in mats])
        present = M_invs.reshape(g, 10, 9).sum(axis=2) != 0                                  # `if M_inv.sum() == 0: ... continue`
        by_part = lambda t, k: t.reshape(g, h, w, k, 3).permute(0, 3, 1, 2, 4).contiguous()   # [g, k, h, w, 3]: one contiguous patch per part
        PU, MU, PL, ML = by_part(img, 10), by_part(masks, 10), by_part(img_lower, 5), by_part(masks_lower, 5)

        # rows of the lower-garment mode: 255 from the first row of the person's own lower garment (gt_parsing in {2, 3}) on
        gt_rows = np.zeros((g, H), dtype=np.uint8)
        for i, it in enumerate(items):
            ys = np.where(np.isin(it['gt_parsing'], (2, 3)).any(axis=(1, 2)))[0]
            if ys.size:
                gt_rows[i, ys[0]:] = 255
        persons = dict(image=up('image'), pose=up('pose'), retain_mask=up('retain_mask'), skin=up('skin'), label=up('label'),
                       gt_rows=torch.from_numpy(gt_rows).to(dev), bound_test=up('bound_test'), gt_parsing=up('gt_parsing'))

        cells = [cell_sources(i, g) for i in range(g * g)]

        # ---- the canvases: one job per distinct (row, garment person), every job in one launch
        keys, jobs, upper_index, lower_index = {}, [], [], []
        for row, col, U, L, mode in cells:
            for kind, who, index in (('up', U, upper_index), ('lo', L, lower_index)):
                key = (kind, row, who)
                if key not in keys:
                    keys[key] = len(jobs)
                    if kind == 'up':
                        jobs.append([(PU[who, ii], MU[who, ii], M_invs[row, ii]) for ii in range(10) if present[row, ii]])
                    else:
                        jobs.append([(PL[who, k], ML[who, k], M_invs[row, ii]) for k, ii in enumerate(LOWER_IDS) if present[row, ii]])
                index.append(keys[key])
        canvases = denorm_canvases(jobs, H, W, KSIZE, taps)

        # ---- the style patches: the upper ones as stored (zeros for a missing part), the lower ones minus the upper garment, warped out and back
        row_of = _to_dev([c[0] for c in cells], torch.int64, dev)
        u_of = _to_dev([c[2] for c in cells], torch.int64, dev)
        keep = torch.from_numpy(present.astype(np.uint8)).to(dev)                             # [g, 10]
        cell_PU = PU.index_select(0, u_of) * keep.index_select(0, row_of)[:, :, None, None, None]
        norm_img = cell_PU.permute(0, 2, 3, 1, 4).reshape(g * g, h, w, 30).contiguous()
        trips = [(i, k, ii) for i, (row, col, U, L, mode) in enumerate(cells) for k, ii in enumerate(LOWER_IDS) if present[row, ii]]
        cell_PL = torch.zeros([g * g, 5, h, w, 3], dtype=torch.uint8, device=dev)
        if trips:
            ti, tk, tii = (_to_dev([t[j] for t in trips], torch.int64, dev) for j in range(3))
            tU, tL = _to_dev([cells[t[0]][2] for t in trips], torch.int64, dev), _to_dev([cells[t[0]][3] for t in trips], torch.int64, dev)
            tmp = PL[tL, tk] * (1 - (MU[tU, tii][..., 0:1] > 0).to(torch.uint8))             # [J, h, w, 3]
            out = warp_batch(list(tmp), [M_invs[cells[i][0], ii] for i, _, ii in trips], (W, H), taps)
            back = warp_batch(list(out), [Ms[cells[i][0], ii] for i, _, ii in trips], (w, h), taps)
            del out
            cell_PL[ti, tk] = back
        norm_img_lower = cell_PL.permute(0, 2, 3, 1, 4).reshape(g * g, h, w, 15).contiguous()

        # ---- the bound rows
        rows = torch.arange(H, dtype=torch.int32, device=dev)[None]
        bound = torch.zeros([g * g, H], dtype=torch.uint8, device=dev)
        lower_cells = [i for i, c in enumerate(cells) if c[4] == 'lower']
        if lower_cells:
            bound[:len(lower_cells)] = persons['gt_rows'].index_select(0, row_of[:len(lower_cells)])      # (the lower rows are the first cells)
        full_cells = [i for i, c in enumerate(cells) if c[4] == 'full']
        full_jobs = [(n, j, i, ii) for n, i in enumerate(full_cells) for j, (k, ii) in enumerate(((0, 0), (1, 6), (3, 8))) if present[cells[i][0], ii]]
        if full_cells:
            acc = torch.zeros([len(full_cells), 3, H, W, 3], dtype=torch.uint8, device=dev)
            if full_jobs:
                srcs = [cell_PL[i, (0, 1, 3)[j]] for _, j, i, _ in full_jobs]
                warped = warp_batch(srcs, [M_invs[cells[i][0], ii] for _, _, i, ii in full_jobs], (W, H), taps)
                acc[_to_dev([f[0] for f in full_jobs], torch.int64, dev), _to_dev([f[1] for f in full_jobs], torch.int64, dev)] = warped
                del warped
            total = acc[:, 0] + acc[:, 1] + acc[:, 2]                                         # uint8 sums wrap around, as NumPy's `+=` does
            ymin = tryon.row_extents(total.contiguous())[:, 0:1]
            bound[full_cells[0]:full_cells[-1] + 1] = torch.where((ymin >= 0) & (rows >= ymin), 255, 0).to(torch.uint8)
            del acc, total
        upper_cells = [i for i, c in enumerate(cells) if c[4] == 'upper']
        torso = [i for i in upper_cells if present[cells[i][0], 0]]
        b_test = persons['bound_test'].index_select(0, row_of[upper_cells[0]:])
        if torso:
            warped = warp_batch([cell_PU[i, 0] for i in torso], [M_invs[cells[i][0], 0] for i in torso], (W, H), taps)
            ymax = torch.full([len(upper_cells), 1], -1, dtype=torch.int32, device=dev)
            ymax[_to_dev([i - upper_cells[0] for i in torso], torch.int64, dev)] = tryon.row_extents(warped)[:, 1:2]
            b_test = torch.where((ymax >= 0) & (rows < ymax), 0, b_test.to(torch.int32)).to(torch.uint8)
            del warped
        bound[upper_cells[0]:] = b_test

        label_of = _to_dev([c[1] if c[4] != 'upper' else c[0] for c in cells], torch.int64, dev)
        label = persons['label'].index_select(0, label_of)
        return SnapshotGrid(g, dev, persons, canvases, _to_dev(upper_index, torch.int64, dev), _to_dev(lower_index, torch.int64, dev), norm_img,
                            norm_img_lower, bound, label, row_of)
