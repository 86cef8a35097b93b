"""The paired reconstruction metrics restricted to label regions, and the confusion count of two label maps, on MI355X.

A *job* of ``region_metrics_table`` is ``(a, b, labels)``: a pair of uint8 [h, w, C] images as in ``image_metrics`` (C in {1, 3}, h, w >= 11, views
with channel stride 1 and pixel stride >= C) and a uint8 [h, w] label view (any positive row stride, pixel stride >= 1).  A *region* is a set of
label values out of 0..31; a pixel is in the region when its label is (a label >= 32 is in no region); regions may overlap; 1..8 regions per call.
Per job and region:

* ``n`` = pixels in the region; ``sad`` / ``ssd`` = sum |a - b| / sum (a - b)^2 over those pixels and all channels, exact int64;
* ``l1`` = sad / (255 n C);  ``mse`` = ssd / (n C);  ``psnr`` = 10 log10(255^2 / mse): NaN for n = 0, psnr +inf for ssd = 0 with n > 0;
* ``positions`` = the valid SSIM positions (y < h - 10, x < w - 10) whose centre pixel (y + 5, x + 5) is in the region;
  ``ssim`` = the sum of ``image_metrics``' SSIM map over those positions and all channels / (positions C): NaN for positions = 0.

``region_metrics_table(jobs, regions)`` returns a dict of device tensors: ``n``, ``sad``, ``ssd``, ``positions`` int64 [J, R]; ``l1``, ``mse``,
``psnr``, ``ssim`` float64 [J, R].  A region holding every label gives the ``sad`` / ``ssd`` of ``image_metrics.pair_metrics_table`` and its SSIM.

``label_confusion_table(jobs, pred_lut, target_lut, classes)``: jobs are ``(pred, target)`` uint8 [h, w] views (h, w >= 1); the two 256-entry
look-up tables map a byte to a class index < `classes` (<= 16) or to ``IGNORE`` = 255 -- the snapshot grid stores a predicted class as a grey byte in
an RGB cell, the loader's target holds the class itself.  Returns int64 [J, K, K] indexed [job, target class, predicted class], counting the pixels
at which both sides map to a class.  ``parsing_scores(confusion)`` -> pixel accuracy, per-class IoU and their mean.

Dispatch follows ``image_metrics``: GPU tensors run ``csrc/region_metrics.hip`` (``pg_region_pair_metrics_u8``: one launch over the whole table
plus a finishing launch, no atomics, bit-identical run to run; ``pg_label_confusion_u8``: one launch, integer atomics into a zeroed table; job
tables go up through pinned memory and nothing is read to the host), CPU tensors run the same definitions in torch, float64 / int64.  A bad
argument raises ``NativeOpError`` on the GPU and ``ValueError`` on the CPU."""

import ctypes

import numpy as np
import torch

from .. import custom_ops
from . import _native as nat
from . import image_metrics

MAX_REGIONS, MAX_LABEL, MAX_CLASSES, IGNORE = 8, 31, 16, 255
HALF = image_metrics.WINDOW // 2

_RPAIR_DT = np.dtype([('a', 'u8'), ('b', 'u8'), ('labels', 'u8'), ('a_row_stride', 'i8'), ('b_row_stride', 'i8'), ('l_row_stride', 'i8'),
                      ('a_pix_stride', 'i4'), ('b_pix_stride', 'i4'), ('l_pix_stride', 'i4'), ('h', 'i4'), ('w', 'i4'), ('channels', 'i4')])
_LPAIR_DT = np.dtype([('pred', 'u8'), ('target', 'u8'), ('p_row_stride', 'i8'), ('t_row_stride', 'i8'), ('p_pix_stride', 'i4'), ('t_pix_stride', 'i4'),
                      ('h', 'i4'), ('w', 'i4')])


class RegionPair(ctypes.Structure):
    """Mirror of ``pg_region_pair`` (include/pasta_gan_ops.h)."""
    _fields_ = [('a', ctypes.c_void_p), ('b', ctypes.c_void_p), ('labels', ctypes.c_void_p), ('a_row_stride', ctypes.c_int64),
                ('b_row_stride', ctypes.c_int64), ('l_row_stride', ctypes.c_int64), ('a_pix_stride', ctypes.c_int), ('b_pix_stride', ctypes.c_int),
                ('l_pix_stride', ctypes.c_int), ('h', ctypes.c_int), ('w', ctypes.c_int), ('channels', ctypes.c_int)]


class LabelPair(ctypes.Structure):
    """Mirror of ``pg_label_pair`` (include/pasta_gan_ops.h)."""
    _fields_ = [('pred', ctypes.c_void_p), ('target', ctypes.c_void_p), ('p_row_stride', ctypes.c_int64), ('t_row_stride', ctypes.c_int64),
                ('p_pix_stride', ctypes.c_int), ('t_pix_stride', ctypes.c_int), ('h', ctypes.c_int), ('w', ctypes.c_int)]


assert _RPAIR_DT.itemsize == ctypes.sizeof(RegionPair) and _LPAIR_DT.itemsize == ctypes.sizeof(LabelPair)

_plugin = None
launch_counter = None     # a dict(regions=0, confusion=0) counts the calls of pg_region_pair_metrics_u8 / pg_label_confusion_u8 (tests, tools)


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('region_metrics_plugin')
        p, i = ctypes.c_void_p, ctypes.c_int
        plugin.lib.pg_region_pair_metrics_workspace.argtypes = [p, i, i]
        plugin.lib.pg_region_pair_metrics_workspace.restype = ctypes.c_int64
        plugin.lib.pg_region_pair_metrics_u8.argtypes = [p, p, i, p, i, p, p, p, p]
        plugin.lib.pg_region_pair_metrics_u8.restype = ctypes.c_int
        plugin.lib.pg_label_confusion_u8.argtypes = [p, p, i, p, p, i, p, p]
        plugin.lib.pg_label_confusion_u8.restype = ctypes.c_int
        _plugin = plugin
    return _plugin


def _count(name):
    if launch_counter is not None:
        launch_counter[name] += 1


def region_bits(regions, err=ValueError):
    """`regions` (1..8 iterables of label values in 0..31) -> uint32 [R]: bit v of word r = label v is in region r."""
    try:
        regions = [[int(v) for v in r] for r in regions]
    except TypeError:
        raise err('region_metrics: regions must be a sequence of iterables of label values') from None
    if not 1 <= len(regions) <= MAX_REGIONS:
        raise err(f'region_metrics: 1 to {MAX_REGIONS} regions per call, got {len(regions)}')
    bits = np.zeros(len(regions), dtype=np.uint32)
    for r, values in enumerate(regions):
        for v in values:
            if not 0 <= v <= MAX_LABEL:
                raise err(f'region_metrics: a region holds label values 0..{MAX_LABEL}, got {v}')
            bits[r] |= np.uint32(1 << v)
    return bits


def _check_labels(t, h, w, dev, what):
    err = image_metrics._error(dev)
    if not isinstance(t, torch.Tensor) or t.device != dev:
        raise err(f'region_metrics: {what} must be a tensor on the images\' device')
    if t.dtype != torch.uint8:
        raise err(f'region_metrics: {what} must be uint8, got {t.dtype}')
    if t.ndim != 2 or (h is not None and tuple(t.shape) != (h, w)):
        raise err(f'region_metrics: {what} must be a [h, w] view' + (f' of the images\' {h} x {w}' if h is not None else '') + f', got {list(t.shape)}')
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise err(f'region_metrics: {what} is empty')
    if t.stride(0) < 1 or t.stride(1) < 1:
        raise err(f'region_metrics: {what} needs positive row and pixel strides, got {t.stride()}')


def _table_cpu(jobs, bits):
    R = len(bits)
    counts = torch.zeros([4, len(jobs), R], dtype=torch.int64)
    ssim_sum = torch.zeros([len(jobs), R], dtype=torch.float64)
    member = torch.tensor([[(int(b) >> v) & 1 for v in range(MAX_LABEL + 1)] + [0] * (256 - MAX_LABEL - 1) for b in bits], dtype=torch.bool)     # [R, 256]
    for j, (a, b, labels) in enumerate(jobs):
        d = a.to(torch.int64) - b.to(torch.int64)
        ad, sq = d.abs().sum(dim=2), (d * d).sum(dim=2)                                   # [h, w]: over the channels
        ssim = image_metrics._ssim_map_cpu(a, b)[:, 0].sum(dim=0)                         # [h - 10, w - 10]
        h, w = labels.shape
        for r in range(R):
            m = member[r][labels.to(torch.int64)]
            centre = m[HALF:h - HALF, HALF:w - HALF]
            counts[0, j, r], counts[1, j, r], counts[2, j, r], counts[3, j, r] = m.sum(), ad[m].sum(), sq[m].sum(), centre.sum()
            ssim_sum[j, r] = ssim[centre].sum()
    return counts, ssim_sum


def region_metrics_table(jobs, regions):
    """`jobs`: a non-empty sequence of (a, b, labels) on one device (module docstring), shapes may differ between jobs; `regions`: 1..8 iterables of
    label values in 0..31.  Returns the dict of [J, R] tensors."""
    jobs = list(jobs)
    if not jobs:
        raise ValueError('region_metrics: no pairs')
    dev = jobs[0][0].device
    err = image_metrics._error(dev)
    bits = region_bits(regions, err)
    shapes = []
    for a, b, labels in jobs:
        if a.device != dev:
            raise err('region_metrics: every pair must be on one device')
        h, w, c = image_metrics._check_pair(a, b)
        _check_labels(labels, h, w, dev, 'labels')
        shapes.append((h, w, c))
    n, R = len(jobs), len(bits)
    if dev.type != 'cuda':
        counts, ssim_sum = _table_cpu(jobs, bits)
        chans = torch.tensor([[c] for _, _, c in shapes], dtype=torch.float64)
    else:
        lib = _init().lib
        t = np.zeros(n, dtype=_RPAIR_DT)
        for k, i in (('a', 0), ('b', 1), ('labels', 2)):
            t[k] = [job[i].data_ptr() for job in jobs]
        for k, i in (('a', 0), ('b', 1), ('l', 2)):
            t[k + '_row_stride'], t[k + '_pix_stride'] = [job[i].stride(0) for job in jobs], [job[i].stride(1) for job in jobs]
        t['h'], t['w'], t['channels'] = [s[0] for s in shapes], [s[1] for s in shapes], [s[2] for s in shapes]
        host = t.ctypes.data_as(ctypes.c_void_p)
        nbytes = int(lib.pg_region_pair_metrics_workspace(host, n, R))
        if nbytes < 0:
            nat.check(nbytes, 'pg_region_pair_metrics_workspace')
        from training.patch_routing import _upload_table             # the pinned staging of every job table of this package
        tab = _upload_table(t, dev)
        work = torch.empty([nbytes // 8], dtype=torch.int64, device=dev)
        counts = torch.empty([4, n, R], dtype=torch.int64, device=dev)
        ssim_sum = torch.empty([n, R], dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            st = lib.pg_region_pair_metrics_u8(host, tab.data_ptr(), n, bits.ctypes.data_as(ctypes.c_void_p), R, work.data_ptr(), counts.data_ptr(),
                                               ssim_sum.data_ptr(), nat.stream_of(counts))
        nat.check(st, 'pg_region_pair_metrics_u8')
        _count('regions')
        chans = torch.from_numpy(np.array([[c] for _, _, c in shapes], dtype=np.float64)).pin_memory().to(dev, non_blocking=True)
    cn, sad, ssd, positions = counts[0], counts[1], counts[2], counts[3]
    samples = cn.to(torch.float64) * chans                                                # n C: 0 -> 0 / 0 = NaN below
    l1 = sad.to(torch.float64) / (255.0 * samples)
    mse = ssd.to(torch.float64) / samples
    psnr = 10.0 * torch.log10(255.0 ** 2 / mse)                                           # mse == 0 -> +inf, NaN -> NaN
    return dict(n=cn, sad=sad, ssd=ssd, positions=positions, l1=l1, mse=mse, psnr=psnr, ssim=ssim_sum / (positions.to(torch.float64) * chans))


def _lut(values, classes, err, what):
    try:
        lut = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values).astype(np.int64).reshape(-1)
    except (TypeError, ValueError):
        raise err(f'region_metrics: {what} must hold 256 integers') from None
    if lut.shape != (256,):
        raise err(f'region_metrics: {what} must hold 256 entries, got {lut.size}')
    if ((lut < 0) | ((lut >= classes) & (lut != IGNORE))).any():
        raise err(f'region_metrics: {what} maps a byte to a class index < {classes} or to {IGNORE} (ignore)')
    return np.ascontiguousarray(lut.astype(np.uint8))


def label_confusion_table(jobs, pred_lut, target_lut, classes):
    """`jobs`: a non-empty sequence of (pred, target) uint8 [h, w] views on one device, shapes may differ between jobs; the look-up tables and
    `classes` as in the module docstring.  Returns int64 [J, classes, classes]: [job, target class, predicted class]."""
    jobs = list(jobs)
    if not jobs:
        raise ValueError('region_metrics: no pairs')
    dev = jobs[0][0].device
    err = image_metrics._error(dev)
    K = int(classes)
    if not 1 <= K <= MAX_CLASSES:
        raise err(f'region_metrics: 1 to {MAX_CLASSES} classes, got {classes}')
    plut, tlut = _lut(pred_lut, K, err, 'pred_lut'), _lut(target_lut, K, err, 'target_lut')
    for pred, target in jobs:
        _check_labels(pred, None, None, dev, 'pred')
        _check_labels(target, int(pred.shape[0]), int(pred.shape[1]), dev, 'target')
    n = len(jobs)
    if dev.type != 'cuda':
        out = torch.zeros([n, K, K], dtype=torch.int64)
        pl, tl = torch.from_numpy(plut.astype(np.int64)), torch.from_numpy(tlut.astype(np.int64))
        for j, (pred, target) in enumerate(jobs):
            pc, tc = pl[pred.to(torch.int64)], tl[target.to(torch.int64)]
            ok = (pc != IGNORE) & (tc != IGNORE)
            out[j] = torch.bincount(tc[ok] * K + pc[ok], minlength=K * K).reshape(K, K)
        return out
    lib = _init().lib
    t = np.zeros(n, dtype=_LPAIR_DT)
    t['pred'], t['target'] = [p.data_ptr() for p, _ in jobs], [q.data_ptr() for _, q in jobs]
    t['p_row_stride'], t['t_row_stride'] = [p.stride(0) for p, _ in jobs], [q.stride(0) for _, q in jobs]
    t['p_pix_stride'], t['t_pix_stride'] = [p.stride(1) for p, _ in jobs], [q.stride(1) for _, q in jobs]
    t['h'], t['w'] = [p.shape[0] for p, _ in jobs], [p.shape[1] for p, _ in jobs]
    from training.patch_routing import _upload_table
    tab = _upload_table(t, dev)
    out = torch.zeros([n, K, K], dtype=torch.int64, device=dev)                           # the kernel adds to it
    with torch.cuda.device(dev):
        st = lib.pg_label_confusion_u8(t.ctypes.data_as(ctypes.c_void_p), tab.data_ptr(), n, plut.ctypes.data_as(ctypes.c_void_p),
                                       tlut.ctypes.data_as(ctypes.c_void_p), K, out.data_ptr(), nat.stream_of(out))
    nat.check(st, 'pg_label_confusion_u8')
    _count('confusion')
    return out


def parsing_scores(confusion):
    """`confusion`: an integer [K, K] table [target class, predicted class] (a [J, K, K] stack is pooled over J) -> dict of float64 tensors on its
    device: ``acc`` = trace / total; ``iou`` [K], iou[k] = c[k, k] / (row k + column k - c[k, k]), NaN where that is 0 / 0 (a class neither present
    nor predicted); ``miou`` = the mean of the IoUs that are not NaN.  Everything is NaN for an all-zero table.  No host read."""
    c = confusion.to(torch.float64)
    if c.ndim == 3:
        c = c.sum(dim=0)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f'region_metrics: a confusion table is [K, K] or [J, K, K], got {list(confusion.shape)}')
    diag = c.diagonal()
    iou = diag / (c.sum(dim=1) + c.sum(dim=0) - diag)                                     # 0 / 0 = NaN
    return dict(acc=diag.sum() / c.sum(), iou=iou, miou=torch.nanmean(iou))
