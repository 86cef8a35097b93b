"""Reconstruction metrics of the two drivers: mean absolute error, PSNR and SSIM between a person dressed in their own garments and their photograph
(the paired figures of the try-on literature; definitions in torch_utils/ops/image_metrics.py).  The reference's ``metrics/`` (FID, KID, PR, PPL, IS)
need detector networks this package cannot obtain, and its own training loop has the calls commented out (training_loop_fullbody.py:738-747); these
three need nothing but the images both drivers already produce.

* `grid_reconstruction(grid)` -- the training driver: the diagonal cells of the snapshot grid are reconstructions (``cell_sources(i * gnum + i, gnum)``
  has U == L == row == col in all three row bands) and the grid's left column holds the photographs, so after ``SnapshotGrid.render`` the gnum pairs are
  windows of ``grid.grid_img`` on the device: no generator work, one launch, one host read.
* `evaluate_results(results_dir)` -- the try-on driver's ``<person>___<clothes>.png`` triptychs (clothes | person | result): the middle panel against
  the right one, for the self-pairs (person == clothes) or for every file.

Dataset-level figures are the means of the per-pair l1, psnr and ssim.

Both drivers can restrict the three figures to label regions (`REGIONS`, over the loader's 7-class ``gt_parsing``: most of a panel is background, face
and shoes, which the generator copies; the garments are what try-on changes), and the training driver can score the generator's parsing head
(``parsing``: pixel accuracy and mean IoU of the grid's predicted parsing against ``gt_parsing``) -- torch_utils/ops/region_metrics.py.  A region
figure is the mean over the pairs in which it is defined (l1, psnr: the region holds a pixel; ssim: it holds the centre of a valid window)."""

import glob
import json
import os

import numpy as np
import torch

from torch_utils.ops import image_metrics
from torch_utils.ops import region_metrics
from . import tryon

NAMES = ('l1', 'psnr', 'ssim')
PARSING = 'parsing'                                    # the training driver's extra name: Metric/parsing_acc, Metric/parsing_miou
PARSING_CLASSES = 7
REGIONS = dict(upper=(1, 4), lower=(2, 3), garment=(1, 2, 3, 4), skin=(5, 6), other=(0,))      # label sets over gt_parsing (training/dataset.py)
NEEDS_DETECTOR = ('fid', 'kid', 'pr', 'ppl', 'is', 'lpips')


def parse_metrics(text):
    """The value of ``--metrics`` (the reference's option, train.py:401): 'none' / '' -> None, else a tuple out of l1, psnr, ssim, parsing (in that
    order; `evaluate_results` refuses parsing).  The reference's own values (fid50k_full, kid50k_full, pr50k3_full, ppl2_wend, is50k, ...) are refused
    with the reason."""
    if text is None or isinstance(text, str) and text.strip().lower() in ('', 'none'):
        return None
    names = tuple(n.strip().lower() for n in (text.split(',') if isinstance(text, str) else text) if n.strip())
    for n in names:
        if n not in NAMES + (PARSING,):
            if any(n.startswith(p) for p in NEEDS_DETECTOR):
                raise ValueError(f'--metrics {n}: FID / KID / PR / PPL / IS (and LPIPS) need a pretrained detector network, which this package '
                                 f'cannot obtain; the supported metrics are {", ".join(NAMES)}')
            raise ValueError(f'--metrics {n}: unknown metric; the supported metrics are {", ".join(NAMES)} (and {PARSING} in the training driver)')
    return tuple(n for n in NAMES + (PARSING,) if n in names) or None


def parse_regions(text):
    """The value of ``--metric-regions`` / ``--regions``: None / 'none' / '' -> None, else a tuple of names out of `REGIONS`, in `REGIONS`' order."""
    if text is None or isinstance(text, str) and text.strip().lower() in ('', 'none'):
        return None
    names = tuple(n.strip().lower() for n in (text.split(',') if isinstance(text, str) else text) if n.strip())
    for n in names:
        if n not in REGIONS:
            raise ValueError(f'region {n}: unknown region; the regions are {", ".join(REGIONS)}')
    return tuple(n for n in REGIONS if n in names) or None


def check_region_options(names, regions):
    """Regions restrict l1 / psnr / ssim: ValueError when `regions` are selected and none of the three is."""
    if regions and not any(n in NAMES for n in (names or ())):
        raise ValueError(f'regions ({", ".join(regions)}) restrict l1, psnr and ssim: select at least one of them with --metrics')


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


def grid_labels(grid):
    """The gnum label windows of `grid_pairs`' panels: columns x0 : x0 + cw of ``grid.persons['gt_parsing']``, uint8 [H, cw] views."""
    x0, cw = panel_window(grid.W)
    return [grid.persons['gt_parsing'][i, :, x0:x0 + cw, 0] for i in range(grid.gnum)]


def grid_parsing_pairs(grid):
    """The gnum (predicted parsing, gt_parsing) windows: channel 0 of diagonal cell (i + 1, i + 1) of ``grid.grid_parsing`` (grey bytes, pixel stride 3)
    and `grid_labels`."""
    H, W = grid.H, grid.W
    x0, cw = panel_window(W)
    par = grid.grid_parsing
    return [(par[(i + 1) * H:(i + 2) * H, (i + 1) * W + x0:(i + 1) * W + x0 + cw, 0], lab) for i, lab in enumerate(grid_labels(grid))]


def parsing_luts(classes=PARSING_CLASSES):
    """(pred_lut, target_lut): the grid's grey byte of class k (``snapshot_grid.grey_table``) -> k, label k -> k; every other byte is ignored."""
    from . import snapshot_grid
    pred, target = np.full(256, region_metrics.IGNORE, np.uint8), np.full(256, region_metrics.IGNORE, np.uint8)
    pred[snapshot_grid.grey_table(classes)] = np.arange(classes, dtype=np.uint8)
    target[:classes] = np.arange(classes, dtype=np.uint8)
    return pred, target


def grid_reconstruction(grid, names=NAMES, regions=None):
    """``{'Metric/recon_<name>': float}`` of a `SnapshotGrid` whose `render` has just run.  `regions` (names out of `REGIONS`) adds
    ``Metric/recon_<name>_<region>``: the mean over the diagonal pairs in which the figure is defined, left out when there is none; the name
    'parsing' adds ``Metric/parsing_acc`` and ``Metric/parsing_miou`` from the confusion pooled over the diagonal cells.  One host read."""
    recon = [n for n in names if n in NAMES]
    keys, values = [], []
    if recon:
        res = image_metrics.pair_metrics_table(grid_pairs(grid))
        keys += [f'Metric/recon_{n}' for n in recon]
        values += [res[n].mean() for n in recon]
    if regions and recon:
        jobs = [(a, b, lab) for (a, b), lab in zip(grid_pairs(grid), grid_labels(grid))]
        reg = region_metrics.region_metrics_table(jobs, [REGIONS[r] for r in regions])
        for n in recon:
            means = torch.nanmean(reg[n], dim=0)                      # [R]; NaN where no pair defines it
            keys += [f'Metric/recon_{n}_{r}' for r in regions]
            values += list(means)
    if PARSING in names:
        pred_lut, target_lut = parsing_luts()
        scores = region_metrics.parsing_scores(region_metrics.label_confusion_table(grid_parsing_pairs(grid), pred_lut, target_lut, PARSING_CLASSES))
        keys += ['Metric/parsing_acc', 'Metric/parsing_miou']
        values += [scores['acc'], scores['miou']]
    host = torch.stack([v.to(torch.float64) for v in values]).cpu().tolist()
    whole = len(recon)                                                # (the whole-panel figures are always defined and always written)
    return {k: float(v) for i, (k, v) in enumerate(zip(keys, host)) if i < whole or not np.isnan(v)}


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


def label_window(dataroot, person, panel_hw, path):
    """The label window of person `person`'s panel: ``<dataroot>/parsing/<person>.png`` through the loader's ``_pad_square(., 0)`` and
    ``gt_parsing_classes``, then `panel_window`'s columns -> uint8 [h, w].  ValueError naming `path` when that is not the panel's shape."""
    import PIL.Image
    from . import dataset as ds_mod
    name = os.path.join(dataroot, 'parsing', person + '.png')
    if not os.path.isfile(name):
        raise ValueError(f'"{path}": no parsing image "{name}"')
    with PIL.Image.open(name) as im:
        raw = np.array(im)
    raw = (raw if raw.ndim == 2 else raw[..., 0])[..., None]
    parsing, _ = ds_mod._pad_square(raw, 0)
    gt, _ = ds_mod.gt_parsing_classes(parsing)
    x0, cw = panel_window(gt.shape[1])
    lab = np.ascontiguousarray(gt[:, x0:x0 + cw, 0].astype(np.uint8))
    if lab.shape != tuple(panel_hw):
        raise ValueError(f'"{path}": the label window of "{name}" is {lab.shape[0]} x {lab.shape[1]}, the panel {panel_hw[0]} x {panel_hw[1]}')
    return lab


def _json_value(v):
    return None if np.isnan(v) else float(v)


def evaluate_results(results_dir, names=NAMES, pairs='self', device='cuda', batch=16, per_file=None, dataroot=None, regions=None):
    """Person panel against result panel over the triptychs of `results_dir` -> ``{name: mean, ..., 'count': n, 'pairs': pairs}``.  Batches of `batch`
    files go up as uint8 and take one launch each; `per_file`: a path that gets one JSON line per image.  ValueError when no file qualifies or a
    width is not divisible by 3.  `regions` (names out of `REGIONS`; needs `dataroot`, the try-on data directory with ``parsing/<person>.png``) adds,
    after those keys, ``<name>_<region>`` -- the mean over the pairs in which the figure is defined, None when there is none -- and
    ``count_<region>``, the pairs in which the region holds a pixel; the per-file lines gain the per-pair values (null where undefined)."""
    names = parse_metrics(names)
    if names is None:
        raise ValueError('no metric selected')
    if PARSING in names:
        raise ValueError('--metrics parsing: the triptychs hold no predicted parsing (the training driver scores the parsing head: train.py --metrics parsing)')
    regions = parse_regions(regions)
    if regions and dataroot is None:
        raise ValueError('--regions needs --dataroot (the directory whose parsing/<person>.png hold the labels)')
    files = result_files(results_dir, pairs)
    if not files:
        raise ValueError(f'no {"self-pair " if pairs == "self" else ""}triptych (<person>___<clothes>.png) in "{results_dir}"')
    dev = torch.device(device)
    cols = {n: [] for n in NAMES}
    rcols = {n: [] for n in NAMES + ('n',)}
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
        if regions:
            labels = [label_window(dataroot, os.path.basename(f)[:-4].split('___', 1)[0], tuple(a.shape[:2]), f) for f, (a, _) in zip(files[lo:], jobs)]
            reg = region_metrics.region_metrics_table([(a, b, torch.from_numpy(lab).to(dev)) for (a, b), lab in zip(jobs, labels)],
                                                      [REGIONS[r] for r in regions])
            for n in rcols:
                rcols[n].append(reg[n].to(torch.float64))
    table = torch.stack([torch.cat(cols[n]) for n in NAMES]).cpu()            # [3, count]: the one host read
    out = {n: float(table[NAMES.index(n)].mean()) for n in names}
    out.update(count=len(files), pairs=pairs)
    rtable = None
    if regions:
        rtable = torch.stack([torch.cat(rcols[n]) for n in NAMES + ('n',)]).cpu().numpy()      # [4, count, R]: ... and the regions' one
        for k, r in enumerate(regions):
            for n in names:
                v = rtable[NAMES.index(n), :, k]
                out[f'{n}_{r}'] = _json_value(v[~np.isnan(v)].mean()) if (~np.isnan(v)).any() else None
            out[f'count_{r}'] = int((rtable[3, :, k] > 0).sum())
    if per_file is not None:
        with open(per_file, 'w') as f:
            for j, path in enumerate(files):
                line = dict({'file': os.path.basename(path)}, **{n: float(table[NAMES.index(n), j]) for n in names})
                if regions:
                    line.update({f'{n}_{r}': _json_value(rtable[NAMES.index(n), j, k]) for k, r in enumerate(regions) for n in names})
                f.write(json.dumps(line) + '\n')
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
    p.add_argument('--dataroot', default=None, help='test data directory (tryon.py --dataroot): its parsing/<person>.png label the regions')
    p.add_argument('--regions', default=None, help=f'comma-separated out of {", ".join(REGIONS)}: the metrics over these label regions too; needs --dataroot')
    a = p.parse_args(argv)
    try:
        out = evaluate_results(a.results, names=a.metrics, pairs=a.pairs, device=a.device, batch=a.batch, per_file=a.per_file, dataroot=a.dataroot,
                               regions=a.regions)
    except ValueError as e:
        sys.exit(f'calc_metrics: {e}')
    print(json.dumps(out), flush=True)
    return out
