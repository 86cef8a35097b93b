"""Reconstruction metrics of the two drivers: mean absolute error, PSNR and SSIM between a person dressed in their own garments and their photograph
(the paired figures of the try-on literature; definitions in torch_utils/ops/image_metrics.py).  The reference's ``metrics/`` (FID, KID, PR, PPL, IS)
need detector networks this package cannot obtain, and its own training loop has the calls commented out (training_loop_fullbody.py:738-747); these
three need nothing but the images both drivers already produce.

* `grid_reconstruction(grid)` -- the training driver: the diagonal cells of the snapshot grid are reconstructions (``cell_sources(i * gnum + i, gnum)``
  has U == L == row == col in all three row bands) and the grid's left column holds the photographs, so after ``SnapshotGrid.render`` the gnum pairs are
  windows of ``grid.grid_img`` on the device: no generator work, one launch, one host read.
* `evaluate_results(results_dir)` -- the try-on driver's ``<person>___<clothes>.png`` triptychs (clothes | person | result): the middle panel against
  the right one, for the self-pairs (person == clothes) or for every file.

Dataset-level figures are the means of the per-pair l1, psnr and ssim."""

import glob
import json
import os

import numpy as np
import torch

from torch_utils.ops import image_metrics
from . import tryon

NAMES = ('l1', 'psnr', 'ssim')
NEEDS_DETECTOR = ('fid', 'kid', 'pr', 'ppl', 'is', 'lpips')


def parse_metrics(text):
    """The value of ``--metrics`` (the reference's option, train.py:401): 'none' / '' -> None, else a tuple out of l1, psnr, ssim.  The reference's own
    values (fid50k_full, kid50k_full, pr50k3_full, ppl2_wend, is50k, ...) are refused with the reason."""
    if text is None or isinstance(text, str) and text.strip().lower() in ('', 'none'):
        return None
    names = tuple(n.strip().lower() for n in (text.split(',') if isinstance(text, str) else text) if n.strip())
    for n in names:
        if n not in NAMES:
            if any(n.startswith(p) for p in NEEDS_DETECTOR):
                raise ValueError(f'--metrics {n}: FID / KID / PR / PPL / IS (and LPIPS) need a pretrained detector network, which this package '
                                 f'cannot obtain; the supported metrics are {", ".join(NAMES)}')
            raise ValueError(f'--metrics {n}: unknown metric; the supported metrics are {", ".join(NAMES)}')
    return tuple(n for n in NAMES if n in names) or None


def panel_window(W):
    """(x0, cw): the columns the try-on triptych keeps of each image (training/tryon.py); an image narrower than that is taken whole."""
    return (tryon.X0, tryon.CW) if W >= tryon.X0 + tryon.CW else (0, W)


def grid_pairs(grid):
    """The gnum (reconstruction, photograph) pairs of a rendered `SnapshotGrid` as strided views of ``grid.grid_img``: diagonal cell (i + 1, i + 1)
    and left-column cell (i + 1, 0), columns x0 : x0 + cw of each."""
    H, W = grid.H, grid.W
    x0, cw = panel_window(W)
    img = grid.grid_img
    return [(img[(i + 1) * H:(i + 2) * H, (i + 1) * W + x0:(i + 1) * W + x0 + cw], img[(i + 1) * H:(i + 2) * H, x0:x0 + cw]) for i in range(grid.gnum)]


def grid_reconstruction(grid, names=NAMES):
    """``{'Metric/recon_<name>': float}`` of a `SnapshotGrid` whose `render` has just run.  One host read."""
    res = image_metrics.pair_metrics_table(grid_pairs(grid))
    means = torch.stack([res[n].mean() for n in names]).cpu().tolist()
    return {f'Metric/recon_{n}': float(v) for n, v in zip(names, means)}


def _read_png(path):
    import PIL.Image
    with PIL.Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


def result_files(results_dir, pairs='self'):
    """The triptychs of `results_dir`: sorted paths of the files named ``<p>___<c>.png``; pairs='self' keeps p == c only."""
    if pairs not in ('self', 'all'):
        raise ValueError("pairs must be 'self' or 'all'")
    out = []
    for path in sorted(glob.glob(os.path.join(glob.escape(results_dir), '*.png'))):
        stem = os.path.basename(path)[:-4]
        if '___' not in stem:
            continue
        p, c = stem.split('___', 1)
        if pairs == 'all' or p == c:
            out.append(path)
    return out


def evaluate_results(results_dir, names=NAMES, pairs='self', device='cuda', batch=16, per_file=None):
    """Person panel against result panel over the triptychs of `results_dir` -> ``{name: mean, ..., 'count': n, 'pairs': pairs}``.  Batches of `batch`
    files go up as uint8 and take one launch each; `per_file`: a path that gets one JSON line per image.  ValueError when no file qualifies or a
    width is not divisible by 3."""
    names = parse_metrics(names)
    if names is None:
        raise ValueError('no metric selected')
    files = result_files(results_dir, pairs)
    if not files:
        raise ValueError(f'no {"self-pair " if pairs == "self" else ""}triptych (<person>___<clothes>.png) in "{results_dir}"')
    dev = torch.device(device)
    cols = {n: [] for n in NAMES}
    for lo in range(0, len(files), max(1, int(batch))):
        jobs = []
        arrays = [_read_png(f) for f in files[lo:lo + max(1, int(batch))]]
        for f, a in zip(files[lo:], arrays):
            if a.shape[1] % 3:
                raise ValueError(f'"{f}": width {a.shape[1]} is not divisible by 3 (not a clothes | person | result triptych)')
        if len({a.shape for a in arrays}) == 1:
            t = torch.from_numpy(np.stack(arrays))
            tensors = list(t.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' else t)
        else:
            tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
        for t in tensors:
            pw = t.shape[1] // 3
            jobs.append((t[:, pw:2 * pw], t[:, 2 * pw:]))
        res = image_metrics.pair_metrics_table(jobs)
        for n in NAMES:
            cols[n].append(res[n])
    table = torch.stack([torch.cat(cols[n]) for n in NAMES]).cpu()            # [3, count]: the one host read
    out = {n: float(table[NAMES.index(n)].mean()) for n in names}
    out.update(count=len(files), pairs=pairs)
    if per_file is not None:
        with open(per_file, 'w') as f:
            for j, path in enumerate(files):
                f.write(json.dumps(dict({'file': os.path.basename(path)}, **{n: float(table[NAMES.index(n), j]) for n in names})) + '\n')
    return out


def main(argv=None):
    import argparse
    import sys
    p = argparse.ArgumentParser(description='L1 / PSNR / SSIM of the try-on driver\'s result images: person panel against result panel.')
    p.add_argument('--results', required=True, help='directory of <person>___<clothes>.png triptychs (tryon.py --outdir)')
    p.add_argument('--metrics', default='l1,psnr,ssim', help='comma-separated out of l1, psnr, ssim')
    p.add_argument('--pairs', choices=['self', 'all'], default='self', help='self: reconstructions only (person == clothes); all: every file')
    p.add_argument('--device', default='cuda')
    p.add_argument('--batch', type=int, default=16, help='images per launch')
    p.add_argument('--per-file', default=None, help='write one JSON line per image to this file')
    a = p.parse_args(argv)
    try:
        out = evaluate_results(a.results, names=a.metrics, pairs=a.pairs, device=a.device, batch=a.batch, per_file=a.per_file)
    except ValueError as e:
        sys.exit(f'calc_metrics: {e}')
    print(json.dumps(out), flush=True)
    return out
