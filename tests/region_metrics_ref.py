"""Restatement of the per-region reconstruction metrics and the label confusion count (torch_utils/ops/region_metrics.py) in NumPy, on the functions
of tests/image_metrics_ref.py: the yardstick of tests/test_region_metrics_{cpu,gpu}.py.

A region is a set of label values 0..31; a pixel belongs to it when its label does.  n / sad / ssd are exact Python integers over the region's pixels
(and all channels).  SSIM: the float64 SSIM map of the whole pair ("valid" positions), a boolean centre mask -- position (y, x) counts when pixel
(y + 5, x + 5) is in the region -- and the masked mean over positions and channels.  `ssim32` is the same masked mean of the float32 map on inputs
minus 127.5 (``image_metrics_ref.ssim_f32``'s map): |ssim32 - ssim| is the e32 of the GPU tests' bar, per (case, region)."""

import numpy as np

import image_metrics_ref as R

HALF = R.WINDOW // 2
NAN = float('nan')


def membership(labels, region):
    labels = np.asarray(labels)
    assert labels.dtype == np.uint8 and labels.ndim == 2 and all(0 <= int(v) <= 31 for v in region)
    return np.isin(labels, [int(v) for v in region])


def ssim_map(a, b, dtype=np.float64):
    """The SSIM map [C, h - 10, w - 10], float64: evaluated in float64 on raw levels, or in float32 on inputs minus 127.5."""
    if dtype == np.float64:
        return R._ssim(R._planes(a, np.float64), R._planes(b, np.float64), R.taps(), R._filter_separable, 0.0)
    m = R._ssim(R._planes(a, np.float32), R._planes(b, np.float32), R.taps(np.float32), R._filter_separable, 127.5)
    assert m.dtype == np.float32
    return m.astype(np.float64)


def region_metrics(a, b, labels, region, maps=None):
    """dict(n, sad, ssd, positions, l1, mse, psnr, ssim, ssim32) of one pair and one region; NaN where a figure is undefined.  `maps`: the pair's
    (float64 map, float32 map) when the caller has them already."""
    a, b, labels = np.asarray(a), np.asarray(b), np.asarray(labels)
    assert a.shape == b.shape and labels.shape == a.shape[:2]
    h, w, c = a.shape
    m = membership(labels, region)
    n = int(m.sum())
    sad, ssd = R.sums(a[m], b[m])
    centre = m[HALF:h - HALF, HALF:w - HALF]
    positions = int(centre.sum())
    m64, m32 = maps if maps is not None else (ssim_map(a, b), ssim_map(a, b, np.float32))
    assert m64.shape == (c,) + centre.shape
    out = dict(n=n, sad=sad, ssd=ssd, positions=positions, l1=NAN, mse=NAN, psnr=NAN, ssim=NAN, ssim32=NAN)
    if n:
        mse = ssd / (n * c)
        out.update(l1=sad / (255.0 * n * c), mse=mse, psnr=float('inf') if ssd == 0 else 10.0 * np.log10(255.0 ** 2 / mse))
    if positions:
        out.update(ssim=float(m64[:, centre].mean()), ssim32=float(m32[:, centre].mean()))
    return out


def confusion(pred, target, pred_lut, target_lut, classes):
    """int64 [K, K] indexed [target class, predicted class]: the pixels at which both look-ups give a class (255 = ignore)."""
    pc, tc = np.asarray(pred_lut)[np.asarray(pred)].astype(np.int64), np.asarray(target_lut)[np.asarray(target)].astype(np.int64)
    ok = (pc != 255) & (tc != 255)
    assert (pc[ok] < classes).all() and (tc[ok] < classes).all()
    out = np.zeros((classes, classes), dtype=np.int64)
    np.add.at(out, (tc[ok], pc[ok]), 1)
    return out


def parsing_scores(c):
    """(acc, iou [K], miou) of a [K, K] confusion table; NaN where undefined."""
    c = np.asarray(c, dtype=np.float64)
    total, diag = c.sum(), np.diag(c)
    den = c.sum(axis=1) + c.sum(axis=0) - diag
    iou = np.array([diag[k] / den[k] if den[k] > 0 else NAN for k in range(len(c))])
    have = ~np.isnan(iou)
    return (diag.sum() / total if total > 0 else NAN), iou, (float(iou[have].mean()) if have.any() else NAN)
