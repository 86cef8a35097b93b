"""Restatement of the reconstruction metrics (torch_utils/ops/image_metrics.py) in NumPy, the yardstick of tests/test_image_metrics_{cpu,gpu}.py.

sad / ssd are exact Python integers.  SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, taps normalised to sum 1, "valid" positions,
population moments, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, mean over positions and channels) is written twice in float64 -- `ssim_separable`
filters rows then columns, `ssim_window` sums the 121 taps of every window explicitly -- and once in float32: `ssim_f32` is the separable form on
inputs minus 127.5, every operation rounded to float32, the precision yardstick of the GPU tests (what a careful float32 evaluation achieves)."""

import numpy as np

WINDOW, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def taps(dtype=np.float64):
    x = np.arange(WINDOW, dtype=np.float64) - WINDOW // 2
    g = np.exp(-x * x / (2 * SIGMA * SIGMA))
    return (g / g.sum()).astype(dtype)


def sums(a, b):
    """(sad, ssd) of two uint8 arrays of one shape, Python integers."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int(np.abs(d).sum()), int((d * d).sum())


def _planes(a, dtype):
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[0] >= WINDOW and a.shape[1] >= WINDOW
    return np.moveaxis(a, 2, 0).astype(dtype)                        # [C, h, w]


def _filter_separable(x, g):
    """'valid' filtering of [C, h, w] along w, then along h, in x's dtype (one rounding per multiply and per add, taps in order)."""
    h, w = x.shape[1], x.shape[2]
    t = np.zeros((x.shape[0], h, w - WINDOW + 1), dtype=x.dtype)
    for k in range(WINDOW):
        t = t + g[k] * x[:, :, k:k + w - WINDOW + 1]
    out = np.zeros((x.shape[0], h - WINDOW + 1, w - WINDOW + 1), dtype=x.dtype)
    for k in range(WINDOW):
        out = out + g[k] * t[:, k:k + h - WINDOW + 1, :]
    return out


def _filter_window(x, g):
    """The same filter as an explicit sum over the 121 taps of the outer-product window."""
    h, w = x.shape[1], x.shape[2]
    win = np.outer(g, g)
    out = np.zeros((x.shape[0], h - WINDOW + 1, w - WINDOW + 1), dtype=x.dtype)
    for i in range(WINDOW):
        for j in range(WINDOW):
            out = out + win[i, j] * x[:, i:i + h - WINDOW + 1, j:j + w - WINDOW + 1]
    return out


def _ssim(x, y, g, filt, origin):
    dt = x.dtype.type
    x, y = x - dt(origin), y - dt(origin)
    ex, ey = filt(x, g), filt(y, g)
    vx, vy, cxy = filt(x * x, g) - ex * ex, filt(y * y, g) - ey * ey, filt(x * y, g) - ex * ey
    mx, my = ex + dt(origin), ey + dt(origin)
    c1, c2 = dt(C1), dt(C2)
    m = ((dt(2) * mx * my + c1) * (dt(2) * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return m


def ssim_separable(a, b):
    return float(_ssim(_planes(a, np.float64), _planes(b, np.float64), taps(), _filter_separable, 0.0).mean())


def ssim_window(a, b):
    return float(_ssim(_planes(a, np.float64), _planes(b, np.float64), taps(), _filter_window, 0.0).mean())


def ssim_f32(a, b, origin=127.5):
    """The separable form in float32 on inputs minus `origin` (127.5: the yardstick; 0: the raw-level evaluation the kernel must beat); the map's
    mean is taken in float64."""
    m = _ssim(_planes(a, np.float32), _planes(b, np.float32), taps(np.float32), _filter_separable, origin)
    assert m.dtype == np.float32
    return float(m.astype(np.float64).mean())


def metrics(a, b):
    """dict(sad, ssd, l1, mse, psnr, ssim) of one pair, float64 restatement."""
    a, b = np.asarray(a), np.asarray(b)
    sad, ssd = sums(a, b)
    n = a.size
    mse = ssd / n
    return dict(sad=sad, ssd=ssd, l1=sad / (255.0 * n), mse=mse, psnr=float('inf') if ssd == 0 else 10.0 * np.log10(255.0 ** 2 / mse),
                ssim=ssim_separable(a, b))
