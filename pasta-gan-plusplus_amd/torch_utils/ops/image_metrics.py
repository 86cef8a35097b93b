"""Paired reconstruction metrics of uint8 images: mean absolute error, PSNR and SSIM (Wang et al. 2004), on MI355X.

A *pair* is two uint8 images of one shape [h, w, C], C in {1, 3}, h, w >= 11.  Per pair:

* ``sad`` = sum |a - b| and ``ssd`` = sum (a - b)^2 over all pixels and channels, exact int64;
* ``l1`` = sad / (255 h w C);  ``mse`` = ssd / (h w C);  ``psnr`` = 10 log10(255^2 / mse), +inf for identical images;
* ``ssim``: separable 11-tap Gaussian window (sigma 1.5, taps normalised to sum 1), "valid" positions only -- (h - 10)(w - 10) per channel, nothing
  padded --, population moments under the window, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, the map
  ``((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2))``, mean over positions and channels.

``pair_metrics(a, b)`` takes [J, h, w, C] tensors, which may be views -- windows of a larger image, with any strides as long as the channel stride is 1
and the pixel stride at least C.  ``pair_metrics_table(jobs)`` takes (a, b) pairs of [h, w, C] views, whose shapes may differ from pair to pair.  Both
return a dict of device tensors: ``sad``, ``ssd`` int64 [J]; ``l1``, ``mse``, ``psnr``, ``ssim`` float64 [J].

Dispatch follows the other ops: GPU tensors run ``csrc/image_metrics.hip`` (``pg_image_pair_metrics_u8``: one launch over the whole table plus a
finishing launch; no atomics, so two runs give the same bits; the job table goes up through pinned memory and nothing is read to the host), CPU
tensors run the same definition in torch, float64.  A bad shape raises ``NativeOpError`` on the GPU and ``ValueError`` on the CPU."""

import ctypes

import numpy as np
import torch

from .. import custom_ops
from . import _native as nat

WINDOW, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2

_PAIR_DT = np.dtype([('a', 'u8'), ('b', 'u8'), ('a_row_stride', 'i8'), ('b_row_stride', 'i8'), ('a_pix_stride', 'i4'), ('b_pix_stride', 'i4'),
                     ('h', 'i4'), ('w', 'i4'), ('channels', 'i4'), ('pad_', 'i4')])


class MetricPair(ctypes.Structure):
    """Mirror of ``pg_metric_pair`` (include/pasta_gan_ops.h)."""
    _fields_ = [('a', ctypes.c_void_p), ('b', ctypes.c_void_p), ('a_row_stride', ctypes.c_int64), ('b_row_stride', ctypes.c_int64),
                ('a_pix_stride', ctypes.c_int), ('b_pix_stride', ctypes.c_int), ('h', ctypes.c_int), ('w', ctypes.c_int), ('channels', ctypes.c_int),
                ('pad_', ctypes.c_int)]


assert _PAIR_DT.itemsize == ctypes.sizeof(MetricPair)

_plugin = None
launch_counter = None     # a dict(pairs=0) counts the calls of pg_image_pair_metrics_u8 (tests, tools/image_metrics_bench.py)


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('image_metrics_plugin')
        p, i = ctypes.c_void_p, ctypes.c_int
        plugin.lib.pg_image_pair_metrics_workspace.argtypes = [p, i]
        plugin.lib.pg_image_pair_metrics_workspace.restype = ctypes.c_int64
        plugin.lib.pg_image_pair_metrics_u8.argtypes = [p, p, i, p, p, p, p, p]
        plugin.lib.pg_image_pair_metrics_u8.restype = ctypes.c_int
        _plugin = plugin
    return _plugin


def gaussian_taps():
    """The 11 taps, float64, normalised to sum 1."""
    x = torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2
    g = torch.exp(-x * x / (2 * SIGMA * SIGMA))
    return g / g.sum()


def _error(dev):
    return nat.NativeOpError if dev.type == 'cuda' else ValueError


def _check_pair(a, b):
    """-> (h, w, C) of a valid pair of [h, w, C] views; raises otherwise."""
    assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)
    err = _error(a.device)
    if a.device != b.device:
        raise err('image_metrics: both images of a pair must be on one device')
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise err(f'image_metrics: uint8 images only, got {a.dtype} and {b.dtype}')
    if a.ndim != 3 or tuple(a.shape) != tuple(b.shape):
        raise err(f'image_metrics: a pair is two [h, w, C] images of one shape, got {list(a.shape)} and {list(b.shape)}')
    h, w, c = (int(v) for v in a.shape)
    if c not in (1, 3):
        raise err(f'image_metrics: 1 or 3 channels, got {c}')
    if h < WINDOW or w < WINDOW:
        raise err(f'image_metrics: the SSIM window needs h, w >= {WINDOW}, got {h} x {w}')
    for t in (a, b):
        if (c > 1 and t.stride(2) != 1) or t.stride(1) < c or t.stride(0) < 1:
            raise err(f'image_metrics: a view needs channel stride 1, pixel stride >= {c} and a positive row stride, got strides {t.stride()}')
    return h, w, c


def _finish(sad, ssd, ssim, count):
    """The derived figures from the raw sums; `count` = h w C per pair (float64 [J])."""
    l1 = sad.to(torch.float64) / (255.0 * count)
    mse = ssd.to(torch.float64) / count
    psnr = 10.0 * torch.log10(255.0 ** 2 / mse)                      # mse == 0 -> +inf
    return dict(sad=sad, ssd=ssd, l1=l1, mse=mse, psnr=psnr, ssim=ssim.to(torch.float64))


def _ssim_cpu(a, b):
    """Mean SSIM of one pair of [h, w, C] uint8 CPU tensors, float64 (0-dim tensor)."""
    return _ssim_map_cpu(a, b).mean()


def _ssim_map_cpu(a, b):
    """The SSIM map of one pair of [h, w, C] uint8 CPU tensors: float64 [C, 1, h - 10, w - 10]."""
    g = gaussian_taps()
    x = a.to(torch.float64).permute(2, 0, 1)[:, None]                # [C, 1, h, w]
    y = b.to(torch.float64).permute(2, 0, 1)[:, None]

    def blur(t):
        t = torch.nn.functional.conv2d(t, g.reshape(1, 1, 1, WINDOW))
        return torch.nn.functional.conv2d(t, g.reshape(1, 1, WINDOW, 1))
    mx, my = blur(x), blur(y)
    vx, vy, cxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def _table_cpu(jobs):
    sad, ssd, ssim = [], [], []
    for a, b in jobs:
        d = a.to(torch.int64) - b.to(torch.int64)
        sad.append(d.abs().sum())
        ssd.append((d * d).sum())
        ssim.append(_ssim_cpu(a, b))
    return torch.stack(sad), torch.stack(ssd), torch.stack(ssim)


def pair_metrics_table(jobs):
    """`jobs`: a non-empty sequence of (a, b), each a pair of uint8 [h, w, C] tensors or views (module docstring) on one device; the shapes may
    differ between pairs.  Returns the dict of [J] tensors."""
    jobs = list(jobs)
    if not jobs:
        raise ValueError('image_metrics: no pairs')
    dev = jobs[0][0].device
    shapes = []
    for a, b in jobs:
        if a.device != dev:
            raise _error(dev)('image_metrics: every pair must be on one device')
        shapes.append(_check_pair(a, b))
    n = len(jobs)
    if dev.type != 'cuda':
        sad, ssd, ssim = _table_cpu(jobs)
        return _finish(sad, ssd, ssim, torch.tensor([h * w * c for h, w, c in shapes], dtype=torch.float64))
    lib = _init().lib
    t = np.zeros(n, dtype=_PAIR_DT)
    t['a'], t['b'] = [a.data_ptr() for a, _ in jobs], [b.data_ptr() for _, b in jobs]
    t['a_row_stride'], t['b_row_stride'] = [a.stride(0) for a, _ in jobs], [b.stride(0) for _, b in jobs]
    t['a_pix_stride'], t['b_pix_stride'] = [a.stride(1) for a, _ in jobs], [b.stride(1) for _, b in jobs]
    t['h'], t['w'], t['channels'] = [s[0] for s in shapes], [s[1] for s in shapes], [s[2] for s in shapes]
    host = t.ctypes.data_as(ctypes.c_void_p)
    nbytes = int(lib.pg_image_pair_metrics_workspace(host, n))
    if nbytes < 0:
        nat.check(nbytes, 'pg_image_pair_metrics_workspace')
    from training.patch_routing import _upload_table                 # the pinned staging of every job table of this package
    tab = _upload_table(t, dev)
    work = torch.empty([nbytes // 8], dtype=torch.int64, device=dev)
    sums = torch.empty([2, n], dtype=torch.int64, device=dev)
    ssim = torch.empty([n], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = lib.pg_image_pair_metrics_u8(host, tab.data_ptr(), n, work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), ssim.data_ptr(),
                                          nat.stream_of(ssim))
    nat.check(st, 'pg_image_pair_metrics_u8')
    if launch_counter is not None:
        launch_counter['pairs'] += 1
    count = torch.from_numpy(np.array([h * w * c for h, w, c in shapes], dtype=np.float64)).pin_memory().to(dev, non_blocking=True)
    return _finish(sums[0], sums[1], ssim, count)


def pair_metrics(a, b):
    """`a`, `b`: uint8 [J, h, w, C] tensors or views on one device -> the dict of [J] tensors (module docstring)."""
    assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)
    err = _error(a.device)
    if a.ndim != 4 or tuple(a.shape) != tuple(b.shape):
        raise err(f'image_metrics: a and b must be [J, h, w, C] of one shape, got {list(a.shape)} and {list(b.shape)}')
    if a.shape[0] < 1:
        raise err('image_metrics: no pairs')
    return pair_metrics_table([(a[j], b[j]) for j in range(a.shape[0])])

