"""The per-region reconstruction metrics and the parsing scores without a GPU: pins of the restatement (tests/region_metrics_ref.py), the claims the
synthetic cases make about their own regions, the op's CPU route against the restatement, and the two drivers (``grid_reconstruction`` and the
training driver's ``stats.jsonl`` on a synthetic visualisation root; ``evaluate_results`` / calc_metrics.py on synthetic triptychs with
``parsing/*.png``).

`build_cases` is shared with tests/test_region_metrics_gpu.py.  Windows: 11 x 11 (one position), 42 x 42 (exactly one 32 x 32 tile of the kernel),
43 x 47 and 75 x 53 (ragged second tile row / column), C = 1 and 3, every pair kind (the flat ones included).  The eight regions of a case, `REGIONS8`:

    0 (1,)  1 (2, 3)  2 (1, 2, 3, 4): overlaps 0 and 1   3 every label 0..31   4 (7,): ONE pixel, the window's centre
    5 (9,): empty -- no pixel carries 9   6 (8,): row 0 and the last column only, i.e. within 5 of the border: n > 0, positions = 0
    7 (0, 31)

Labels are 4 x 4 blocks of 0..6, sprinkled with 31 and with labels >= 32 (in no region, not even 3); from 42 x 42 on a 9 x 9 patch of label 1 lies
across the tile seam at pixel 32.  What each case claims about n and positions is asserted on the restatement in
`test_the_cases_hold_what_they_claim`.  The two driver runs are the slow part (~30 s on the CPU, as in tests/test_image_metrics_cpu.py)."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_metrics_ref as R
import region_metrics_ref as RR
from test_snapshot_grid_cpu import WIDTH, write_vis_root

PIL = pytest.importorskip('PIL.Image')

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pasta-gan-plusplus_amd')

SHAPES = ((11, 11), (42, 42), (43, 47), (75, 53))
KINDS = ('noise', 'noise+-3', 'sine+-20', 'flat+-1', 'flat 200/255', 'identical')
REGIONS8 = ((1,), (2, 3), (1, 2, 3, 4), tuple(range(32)), (7,), (9,), (8,), (0, 31))
NONEMPTY = (0, 1, 2, 3, 7)                      # from 42 x 42 on these hold the centre of a valid window
FIGURES = ('l1', 'mse', 'psnr', 'ssim')


def noise(rng, shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def nudge(rng, a, k):
    return np.clip(a.astype(np.int64) + rng.integers(-k, k + 1, a.shape), 0, 255).astype(np.uint8)


def make_pair(rng, kind, h, w, c):
    """The pair kinds of tests/test_image_metrics_gpu.py."""
    if kind == 'noise':
        return noise(rng, (h, w, c)), noise(rng, (h, w, c))
    if kind == 'noise+-3':
        a = noise(rng, (h, w, c))
        return a, nudge(rng, a, 3)
    if kind.startswith('sine'):
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([127.5 + 100 * np.sin(x / (5.0 + k) + 0.3 * k) * np.cos(y / (7.0 - k)) for k in range(c)], axis=2).round().astype(np.uint8)
        return a, nudge(rng, a, int(kind.split('+-')[1]))
    if kind == 'flat+-1':
        a = np.full((h, w, c), 200, np.uint8)
        return a, (200 + rng.integers(-1, 2, a.shape)).astype(np.uint8)
    if kind == 'flat 200/255':
        return np.full((h, w, c), 200, np.uint8), np.full((h, w, c), 255, np.uint8)
    a = noise(rng, (h, w, c))
    return a, a.copy()


def make_labels(rng, h, w):
    lab = np.repeat(np.repeat(rng.integers(0, 7, ((h + 3) // 4, (w + 3) // 4)), 4, axis=0), 4, axis=1)[:h, :w].astype(np.uint8)
    sprinkle = rng.random((h, w)) < 0.04
    lab[sprinkle] = rng.choice(np.array([31, 32, 40, 255], np.uint8), int(sprinkle.sum()))
    if h >= 42 and w >= 42:
        lab[28:37, 28:37] = 1                    # across the seam between the first tile's pixels (0..31) and the next one's, both ways
        lab[20, 20] = 200                        # the centre of a valid window, in no region
    lab[1, 1] = 40
    lab[0, :] = 8
    lab[:, w - 1] = 8
    lab[h // 2, w // 2] = 7
    return lab


class Case:
    """One pair with its labels, and per region of `regions` the restatement's figures (`want[r]`) and the SSIM bar max(1e-6, 2 e32)."""

    def __init__(self, name, a, b, labels, regions=REGIONS8):
        self.name, self.a, self.b, self.labels, self.regions = name, a, b, labels, regions
        maps = RR.ssim_map(a, b), RR.ssim_map(a, b, np.float32)
        self.want = [RR.region_metrics(a, b, labels, reg, maps) for reg in regions]
        self.e32 = [abs(w['ssim32'] - w['ssim']) if w['positions'] else 0.0 for w in self.want]
        self.bar = [max(1e-6, 2 * e) for e in self.e32]


_CASES = []


def build_cases():
    """Every (shape, C, kind): built once per process, never modified."""
    if not _CASES:
        rng = np.random.default_rng(21)
        for h, w in SHAPES:
            for c in (1, 3):
                for kind in KINDS:
                    _CASES.append(Case(f'{kind} {h}x{w}x{c}', *make_pair(rng, kind, h, w, c), make_labels(rng, h, w)))
    return _CASES


def same_float(got, want, rel):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return got == pytest.approx(want, rel=rel, abs=0)


def check_table(res, cases_, ssim_bar=None, label=''):
    """`res` (the op's dict, [J, R]) against the cases' restatement: the four integers equal; l1 / mse / psnr at rel 1e-13 (NaN and inf asserted as
    such); ssim within `ssim_bar` (a number) or the case's own bar, NaN where positions = 0.  Every (case, region) is compared.  -> worst dev / bar."""
    host = {k: v.cpu().tolist() for k, v in res.items()}
    worst = 0.0
    for j, cs in enumerate(cases_):
        for r, want in enumerate(cs.want):
            for k in ('n', 'sad', 'ssd', 'positions'):
                assert host[k][j][r] == want[k], (cs.name, r, k, host[k][j][r], want[k])
            for k in ('l1', 'mse', 'psnr'):
                assert same_float(host[k][j][r], want[k], 1e-13), (cs.name, r, k, host[k][j][r], want[k])
            got = host['ssim'][j][r]
            if want['positions'] == 0:
                assert math.isnan(got), (cs.name, r, got)
                continue
            bar = ssim_bar if ssim_bar is not None else cs.bar[r]
            dev = abs(got - want['ssim'])
            worst = max(worst, dev / bar)
            if label:
                print(f'{label}{cs.name:26s} region {r} ssim {want["ssim"]:+.9f} dev {dev:.2e} e32 {cs.e32[r]:.2e} dev/bar {dev / bar:.3f}')
            assert dev <= bar, (cs.name, r, dev, bar)
    return worst


# ------------------------------------------------------------------------------------------------------------- the restatement

def test_restatement_by_hand():
    a = np.zeros((11, 11, 1), np.uint8)
    b = np.zeros((11, 11, 1), np.uint8)
    lab = np.zeros((11, 11), np.uint8)
    a[0, 0, 0], lab[0, 0] = 255, 3                      # |d| = 255, in region (3,)
    a[3, 4, 0], b[3, 4, 0], lab[3, 4] = 10, 13, 3       # 3
    a[5, 5, 0], b[5, 5, 0], lab[5, 5] = 7, 1, 4         # 6, the centre pixel, in region (4,)
    lab[9, 9] = 40                                      # in no region
    m = RR.region_metrics(a, b, lab, (3,))
    assert (m['n'], m['sad'], m['ssd'], m['positions']) == (2, 258, 255 * 255 + 9, 0)
    assert m['l1'] == 258 / (255 * 2) and m['mse'] == (65025 + 9) / 2 and math.isnan(m['ssim'])
    m = RR.region_metrics(a, b, lab, (4, 17))
    assert (m['n'], m['sad'], m['ssd'], m['positions']) == (1, 6, 36, 1) and abs(m['ssim'] - R.ssim_separable(a, b)) <= 1e-15
    m = RR.region_metrics(a, b, lab, (5,))
    assert m['n'] == m['positions'] == 0 and all(math.isnan(m[k]) for k in FIGURES)
    m = RR.region_metrics(a, b, lab, range(32))
    assert m['n'] == 120 and (m['sad'], m['ssd']) == R.sums(a, b)
    ident = RR.region_metrics(a, a.copy(), lab, (3,))
    assert ident['psnr'] == math.inf and ident['l1'] == 0.0


def test_restatement_of_a_whole_region_is_the_unmasked_metric():
    rng = np.random.default_rng(22)
    a, b = noise(rng, (30, 23, 3)), noise(rng, (30, 23, 3))
    m = RR.region_metrics(a, b, rng.integers(0, 32, (30, 23)).astype(np.uint8), range(32))
    want = R.metrics(a, b)
    assert (m['n'], m['positions'], m['sad'], m['ssd']) == (30 * 23, 20 * 13, want['sad'], want['ssd'])
    assert abs(m['ssim'] - want['ssim']) <= 1e-14 and m['psnr'] == pytest.approx(want['psnr'], rel=1e-15)
    assert abs(m['ssim32'] - R.ssim_f32(a, b)) <= 1e-14


def test_the_cases_hold_what_they_claim():
    for cs in build_cases():
        h, w, _ = cs.a.shape
        want = cs.want
        assert want[4]['n'] == 1 and want[4]['positions'] == 1, cs.name                     # one pixel: the centre
        assert want[5]['n'] == 0 and want[5]['positions'] == 0 and math.isnan(want[5]['l1']), cs.name
        assert want[6]['n'] == h + w - 1 and want[6]['positions'] == 0 and math.isfinite(want[6]['l1']) and math.isnan(want[6]['ssim']), cs.name
        assert want[3]['positions'] < (h - 10) * (w - 10) or min(h, w) == 11, cs.name        # labels >= 32 are not even in the region of every label
        assert want[3]['n'] == int((cs.labels < 32).sum()) < h * w, cs.name
        assert want[2]['n'] == want[0]['n'] + int(np.isin(cs.labels, (2, 3, 4)).sum()), cs.name
        if min(h, w) >= 42:
            assert all(want[r]['positions'] > 0 and math.isfinite(want[r]['ssim']) for r in NONEMPTY), cs.name
            assert (cs.labels[28:37, 28:37] == 1).all()
        else:
            assert want[3]['positions'] == 1 and want[0]['positions'] == 0                   # 11 x 11: the one position's centre carries label 7
    kinds = {cs.name.split(' ')[0] for cs in build_cases()}
    assert {'flat+-1', 'flat', 'identical'} <= kinds
    assert any(cs.want[3]['psnr'] == math.inf for cs in build_cases())


# ------------------------------------------------------------------------------------------------------------- the op's CPU route

def jobs_of(cases_, dev='cpu'):
    return [(torch.from_numpy(cs.a).to(dev), torch.from_numpy(cs.b).to(dev), torch.from_numpy(cs.labels).to(dev)) for cs in cases_]


def test_cpu_route_equals_the_restatement():
    from torch_utils.ops import region_metrics as M
    cases_ = build_cases()
    res = M.region_metrics_table(jobs_of(cases_), REGIONS8)
    for k in ('n', 'sad', 'ssd', 'positions'):
        assert res[k].dtype == torch.int64 and res[k].shape == (len(cases_), 8)
    for k in FIGURES:
        assert res[k].dtype == torch.float64 and res[k].shape == (len(cases_), 8)
    check_table(res, cases_, ssim_bar=1e-12)
    one = M.region_metrics_table(jobs_of(cases_[7:8]), [REGIONS8[2]])                              # R = 1
    check_table(one, [Case('R = 1', cases_[7].a, cases_[7].b, cases_[7].labels, [REGIONS8[2]])], ssim_bar=1e-12)


def test_cpu_route_on_views():
    from torch_utils.ops import region_metrics as M
    rng = np.random.default_rng(23)
    parent = torch.from_numpy(noise(rng, (64, 97, 3)))
    wide = torch.from_numpy(noise(rng, (50, 60, 4)))
    lab = torch.from_numpy(rng.integers(0, 7, (64, 97)).astype(np.uint8))
    lab3 = torch.from_numpy(rng.integers(0, 7, (70, 120, 3)).astype(np.uint8))
    jobs = [(parent[2:45, 3:48], parent[19:62, 50:95], lab[2:45, 3:48]), (wide[1:44, 2:50, :3], wide[3:46, 5:53, 1:], lab3[3:46, 5:53, 0]),
            (wide[1:44, 2:50, 3:], wide[3:46, 5:53, :1], lab3[3:46, 5:53, 2])]
    regions = [(1, 4), (2, 3), (5, 6)]
    res = M.region_metrics_table(jobs, regions)
    check_table(res, [Case(f'view {j}', a.numpy(), b.numpy(), l.numpy(), regions) for j, (a, b, l) in enumerate(jobs)], ssim_bar=1e-12)


def test_cpu_route_refuses_bad_arguments():
    from torch_utils.ops import region_metrics as M
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)
    ok = (z(20, 20, 3), z(20, 20, 3), z(20, 20))
    assert M.region_metrics_table([ok], [(0,)])['n'].tolist() == [[400]]
    for regions in ([], [(0,)] * 9, [(32,)], [(-1,)], 5, [3]):
        with pytest.raises(ValueError):
            M.region_metrics_table([ok], regions)
    for job in ((z(10, 20, 3), z(10, 20, 3), z(10, 20)), (z(20, 20, 2), z(20, 20, 2), z(20, 20)), (z(20, 20, 3), z(20, 20, 3), z(20, 21)),
                (z(20, 20, 3), z(20, 20, 3), z(20, 20, 1)), (z(20, 20, 3), z(20, 20, 3), z(20, 20).float()), (z(20, 20, 3), z(20, 21, 3), z(20, 20))):
        with pytest.raises(ValueError):
            M.region_metrics_table([job], [(0,)])
    with pytest.raises(ValueError):
        M.region_metrics_table([], [(0,)])
    ident, lut = np.arange(256), np.full(256, 255)
    lut[:4] = np.arange(4)
    assert M.label_confusion_table([(z(3, 5), z(3, 5))], lut, lut, 4)[0, 0, 0] == 15
    for args in ((ident, lut, 4), (lut, lut, 0), (lut, lut, 17), (lut[:255], lut, 4), (lut, np.where(lut == 3, 4, lut), 4)):
        with pytest.raises(ValueError):
            M.label_confusion_table([(z(3, 5), z(3, 5))], *args)
    for job in ((z(3, 5), z(3, 6)), (z(3, 5, 1), z(3, 5, 1)), (z(0, 5), z(0, 5)), (z(3, 5).float(), z(3, 5))):
        with pytest.raises(ValueError):
            M.label_confusion_table([job], lut, lut, 4)
    with pytest.raises(ValueError):
        M.label_confusion_table([], lut, lut, 4)


# ------------------------------------------------------------------------------------------------------------- confusion and scores

def grey_luts():
    """(pred_lut, target_lut) of the snapshot grid's K = 7 parsing, written out: grey bytes 0, 43, 85, 128, 170, 212, 255 -> 0..6."""
    pred, target = np.full(256, 255, np.uint8), np.full(256, 255, np.uint8)
    for k, g in enumerate((0, 43, 85, 128, 170, 212, 255)):
        pred[g] = k
    target[:7] = np.arange(7)
    return pred, target


def confusion_jobs(rng):
    """[(pred view, target view, pred_lut, target_lut, K)]: K = 7 on channel 0 of RGB cells (grey bytes and a few bytes that are no grey level;
    targets 0..6 and a few 9s: ignored on either side) -- 1 x 1, 3 x 70 and 45 x 333 (several workgroups, not a multiple of 8) --, and K = 16 on bytes
    0..20 (16..20 ignored), the target a strided view."""
    greys = np.array([0, 43, 85, 128, 170, 212, 255, 7, 100], np.uint8)
    p7, t7 = grey_luts()
    ident = np.where(np.arange(256) < 16, np.arange(256), 255).astype(np.uint8)
    out = []
    for h, w in ((1, 1), (3, 70), (45, 333)):
        cell = np.repeat(greys[np.repeat(rng.integers(0, 9, (h, (w + 5) // 6)), 6, axis=1)[:, :w]][..., None], 3, axis=2)
        cell[..., 1:] = noise(rng, (h, w, 2))
        target = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 9], np.uint8), (h, w))
        out.append((torch.from_numpy(cell)[:, :, 0], torch.from_numpy(target), p7, t7, 7))
    big = torch.from_numpy(rng.integers(0, 21, (40, 2 * 51)).astype(np.uint8))
    out.append((torch.from_numpy(rng.integers(0, 21, (40, 51)).astype(np.uint8)), big[:, 1::2], ident, ident, 16))
    return out


def test_confusion_cpu_route_equals_the_restatement():
    from torch_utils.ops import region_metrics as M
    jobs = confusion_jobs(np.random.default_rng(24))
    got = M.label_confusion_table([(p, t) for p, t, _, _, _ in jobs[:3]], jobs[0][2], jobs[0][3], 7)
    assert got.dtype == torch.int64 and got.shape == (3, 7, 7)
    for j, (p, t, pl, tl, K) in enumerate(jobs[:3]):
        want = RR.confusion(p.numpy(), t.numpy(), pl, tl, K)
        assert np.array_equal(got[j].numpy(), want) and want.sum() < p.numel() + (j == 0), j       # some pixels are ignored
    p, t, pl, tl, K = jobs[3]
    assert np.array_equal(M.label_confusion_table([(p, t)], pl, tl, K)[0].numpy(), RR.confusion(p.numpy(), t.numpy(), pl, tl, K))
    from training import metrics as MT
    assert all(np.array_equal(x, y) for x, y in zip(MT.parsing_luts(), grey_luts()))


def test_parsing_scores_by_hand():
    from torch_utils.ops import region_metrics as M
    table = [[3, 1, 0], [0, 2, 0], [0, 0, 0]]                        # class 2 neither present nor predicted
    s = M.parsing_scores(torch.tensor(table))
    assert s['acc'].dtype == s['iou'].dtype == s['miou'].dtype == torch.float64
    assert float(s['acc']) == 5 / 6 and s['iou'].tolist()[:2] == [3 / 4, 2 / 3] and math.isnan(s['iou'][2]) and float(s['miou']) == (3 / 4 + 2 / 3) / 2
    acc, iou, miou = RR.parsing_scores(table)
    assert acc == 5 / 6 and miou == (3 / 4 + 2 / 3) / 2 and math.isnan(iou[2])
    pooled = M.parsing_scores(torch.tensor([table, [[0, 0, 0], [0, 0, 0], [0, 0, 4]]]))            # [J, K, K] is pooled
    assert float(pooled['acc']) == 9 / 10 and pooled['iou'].tolist() == [3 / 4, 2 / 3, 1.0]
    zero = M.parsing_scores(torch.zeros(3, 3, dtype=torch.int64))
    assert math.isnan(zero['acc']) and math.isnan(zero['miou']) and all(math.isnan(v) for v in zero['iou'].tolist())
    assert all(math.isnan(v) for v in (RR.parsing_scores(np.zeros((3, 3)))[0], RR.parsing_scores(np.zeros((3, 3)))[2]))


# ------------------------------------------------------------------------------------------------------------- the training driver

@pytest.fixture(scope='module')
def vis_root(tmp_path_factory):
    return write_vis_root(str(tmp_path_factory.mktemp('vis_region_metrics')))


def gt_windows(vis_root):
    """The three persons' gt_parsing, columns 96 : 416 (the loader's own map: tests/test_train_loader.py covers it)."""
    from training.dataset import NO_ERASE, TrainSet
    ts = TrainSet(vis_root, shuffle=False, device='cpu')
    return [np.ascontiguousarray(ts.unrouted(i, NO_ERASE)['gt_parsing'][:, 96:416, 0]) for i in ts.vis_index[:3]]


def grid_reference(fin_grid, par_grid, gts, names, regions, parsing):
    """The restatement on the downloaded grids: diagonal cell against left-column cell, columns 96 : 416, labels = the person's gt_parsing."""
    from training import metrics as MT
    out = {}
    per = []
    for i, gt in enumerate(gts):
        rows = slice(512 * (i + 1), 512 * (i + 2))
        a, b = fin_grid[rows, 512 * (i + 1) + 96:512 * (i + 1) + 416], fin_grid[rows, 96:416]
        maps = RR.ssim_map(a, b), RR.ssim_map(a, b, np.float32)
        per.append({r: RR.region_metrics(a, b, gt, MT.REGIONS[r], maps) for r in regions})
    for n in names:
        for r in regions:
            vals = [p[r][n] for p in per if not math.isnan(p[r][n])]
            if vals:
                out[f'Metric/recon_{n}_{r}'] = float(np.mean(vals))
    if parsing:
        p7, t7 = grey_luts()
        pooled = sum(RR.confusion(par_grid[512 * (i + 1):512 * (i + 2), 512 * (i + 1) + 96:512 * (i + 1) + 416, 0], gt, p7, t7, 7) for i, gt in enumerate(gts))
        acc, _, miou = RR.parsing_scores(pooled)
        out.update({'Metric/parsing_acc': acc, 'Metric/parsing_miou': miou})
    return out, per


def test_option_parsing():
    from training import metrics as MT
    from training import training_loop as T
    assert MT.REGIONS == dict(upper=(1, 4), lower=(2, 3), garment=(1, 2, 3, 4), skin=(5, 6), other=(0,))
    assert MT.parse_regions(None) is None and MT.parse_regions('none') is None and MT.parse_regions('') is None
    assert MT.parse_regions('skin, upper,lower') == ('upper', 'lower', 'skin') and MT.parse_regions(('other',)) == ('other',)
    with pytest.raises(ValueError, match='unknown region'):
        MT.parse_regions('upper,sleeves')
    assert MT.parse_metrics('parsing,ssim') == ('ssim', 'parsing') and MT.parse_metrics('l1') == ('l1',)
    base = ['--data', 'd', '--outdir', 'o']
    assert T.parse_args(base).metric_regions == 'none' and T.parse_args(base + ['--metric-regions', 'upper,skin']).metric_regions == 'upper,skin'
    for argv in (['--metric-regions', 'upper'], ['--metric-regions', 'upper', '--metrics', 'parsing']):       # refused before anything is read or built
        with pytest.raises(SystemExit, match='select at least one'):
            T.main(base + argv)
    with pytest.raises(SystemExit, match='unknown region'):
        T.main(base + ['--metrics', 'l1', '--metric-regions', 'hat'])
    with pytest.raises(ValueError, match='select at least one'):
        T.training_loop('o', 'd', metrics='parsing', metric_regions='upper')


def test_grid_reconstruction_with_regions_and_parsing_on_a_cpu_grid(vis_root):
    from training import metrics as MT
    from training import snapshot_grid as S
    from training import training_loop as T
    from training.dataset import TrainSet
    grid = S.setup_snapshot_grid(TrainSet(vis_root, shuffle=False, device='cpu'), 'cpu')
    gts = gt_windows(vis_root)
    assert grid.persons['gt_parsing'].dtype == torch.uint8 and tuple(grid.persons['gt_parsing'].shape) == (3, 512, 512, 1)
    for lab, gt in zip(MT.grid_labels(grid), gts):
        assert np.array_equal(lab.numpy(), gt)
    torch.manual_seed(0)
    G = T.build_networks(1, 'cpu', WIDTH)[0].eval().requires_grad_(False)
    fin_grid, par_grid = grid.render(G, 3)
    assert list(MT.grid_reconstruction(grid, ('l1', 'psnr', 'ssim'))) == ['Metric/recon_l1', 'Metric/recon_psnr', 'Metric/recon_ssim']     # as today
    regions = ('upper', 'lower', 'skin')
    got = MT.grid_reconstruction(grid, ('l1', 'ssim', 'parsing'), regions)
    want, per = grid_reference(fin_grid, par_grid, gts, ('l1', 'ssim'), regions, True)
    assert list(got)[:2] == ['Metric/recon_l1', 'Metric/recon_ssim'] and set(got) - set(list(got)[:2]) == set(want)
    assert any(p[r]['n'] == 0 for p in per for r in regions) and 'Metric/recon_l1_upper' in want      # the dress wearer has no lower garment ...
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k
    assert 0 <= got['Metric/parsing_acc'] <= 1 and 0 <= got['Metric/parsing_miou'] <= 1
    assert set(MT.grid_reconstruction(grid, ('parsing',))) == {'Metric/parsing_acc', 'Metric/parsing_miou'}
    pred, lab = MT.grid_parsing_pairs(grid)[1]
    assert pred.shape == lab.shape == (512, 320) and pred.stride(1) == 3 and pred.data_ptr() - grid.grid_parsing.data_ptr() == (1024 * 2048 + 1024 + 96) * 3


def stats_lines(run):
    return [json.loads(line) for line in open(os.path.join(run, 'stats.jsonl'))]


def test_driver_writes_the_new_keys_only_when_asked(vis_root, tmp_path, capsys):
    from training import training_loop as T
    kw = dict(batch=1, batch_gpu=1, kimg=0.001, tick=0.001, snap=None, image_snap=1, workers=0, device='cpu', width=WIDTH, aug='noaug',
              dataset_kwargs=dict(shuffle=False))
    plain, full = str(tmp_path / 'plain'), str(tmp_path / 'full')
    T.training_loop(plain, vis_root, metrics=('l1', 'psnr', 'ssim'), **kw)
    line = stats_lines(plain)[0]
    assert [k for k in line if k.startswith('Metric/')] == ['Metric/recon_l1', 'Metric/recon_psnr', 'Metric/recon_ssim']
    T.training_loop(full, vis_root, metrics='l1,psnr,ssim,parsing', metric_regions='upper,lower,skin', **kw)
    line = stats_lines(full)[0]
    fin, par = (np.array(PIL.open(os.path.join(full, f'fakes000000_{n}.png'))) for n in ('finetune', 'parsing'))
    want, _ = grid_reference(fin, par, gt_windows(vis_root), ('l1', 'psnr', 'ssim'), ('upper', 'lower', 'skin'), True)
    metric_keys = [k for k in line if k.startswith('Metric/')]
    assert metric_keys[:3] == ['Metric/recon_l1', 'Metric/recon_psnr', 'Metric/recon_ssim'] and set(metric_keys[3:]) == set(want) and len(want) == 11
    for k, v in want.items():
        assert line[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k
    assert stats_lines(plain)[0]['Metric/recon_ssim'] == line['Metric/recon_ssim']               # the whole-panel figures do not move
    assert 'Metric/parsing_miou' in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------------- evaluate_results / calc_metrics.py

def write_region_results(root, rng):
    """Triptychs of 24 x 24 panels and ``dataroot/parsing/<person>.png`` of 24 x 16 raw parsing labels (the loader pads them to 24 x 24 with 0):
    p1 wears a top (5) and pants (9), p2 a top only -- its 'lower' region is empty --; both show neck (10) and an arm (14).  Returns
    (results dir, dataroot, {file: (person panel, result panel, gt label window)})."""
    res, data = os.path.join(root, 'res'), os.path.join(root, 'data')
    os.makedirs(res)
    os.makedirs(os.path.join(data, 'parsing'))
    gts = {}
    for person, lower in (('p1', True), ('p2', False)):
        raw = np.zeros((24, 16), np.uint8)
        raw[2:4, 6:10] = 10
        raw[4:12, 3:13] = 5
        raw[5:11, 1:3] = 14
        raw[0:2, 6:10] = 2                       # hair: class 0
        if lower:
            raw[12:22, 4:12] = 9
        PIL.fromarray(raw, 'L').save(os.path.join(data, 'parsing', person + '.png'))
        gt = np.zeros((24, 24), np.uint8)
        gt[:, 4:20] = np.select([raw == 5, raw == 9, raw == 10, raw == 14], [1, 2, 5, 6], 0)
        gts[person] = gt
    out = {}
    for name in ('p1___p1.png', 'p2___p2.png', 'p1___p2.png'):
        person = noise(rng, (24, 24, 3))
        trip = np.concatenate([noise(rng, (24, 24, 3)), person, nudge(rng, person, 9)], axis=1)
        PIL.fromarray(trip, 'RGB').save(os.path.join(res, name))
        out[name] = (trip[:, 24:48], trip[:, 48:], gts[name.split('___')[0]])
    return res, data, out


def region_reference(panels, files, names, regions):
    from training import metrics as MT
    per = [{r: RR.region_metrics(*panels[f], MT.REGIONS[r]) for r in regions} for f in files]
    out = {}
    for r in regions:
        for n in names:
            vals = [p[r][n] for p in per if not math.isnan(p[r][n])]
            out[f'{n}_{r}'] = float(np.mean(vals)) if vals else None
        out[f'count_{r}'] = sum(p[r]['n'] > 0 for p in per)
    return out, per


def test_evaluate_results_with_regions(tmp_path):
    from training import metrics as MT
    res, data, panels = write_region_results(str(tmp_path), np.random.default_rng(25))
    per_file = str(tmp_path / 'per.jsonl')
    assert list(MT.evaluate_results(res, device='cpu')) == ['l1', 'psnr', 'ssim', 'count', 'pairs']                      # as today
    got = MT.evaluate_results(res, device='cpu', batch=2, per_file=per_file, dataroot=data, regions='skin,upper,lower')
    files, regions = ['p1___p1.png', 'p2___p2.png'], ('upper', 'lower', 'skin')
    want, per = region_reference(panels, files, ('l1', 'psnr', 'ssim'), regions)
    assert list(got) == ['l1', 'psnr', 'ssim', 'count', 'pairs'] + [k for r in regions for k in (f'l1_{r}', f'psnr_{r}', f'ssim_{r}', f'count_{r}')]
    assert got['count'] == 2 and got['count_upper'] == 2 and got['count_lower'] == 1 and got['count_skin'] == 2
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12), k
    assert got['ssim'] == pytest.approx(np.mean([R.metrics(*panels[f][:2])['ssim'] for f in files]), abs=1e-12)
    lines = [json.loads(line) for line in open(per_file)]
    assert [line['file'] for line in lines] == files
    assert lines[1]['l1_lower'] is None and lines[1]['ssim_lower'] is None and 'null' in open(per_file).read()         # p2: no lower garment
    for line, p in zip(lines, per):
        for r in regions:
            for n in ('l1', 'psnr', 'ssim'):
                assert (line[f'{n}_{r}'] is None) == math.isnan(p[r][n])
                assert line[f'{n}_{r}'] is None or line[f'{n}_{r}'] == pytest.approx(p[r][n], rel=1e-12), (line['file'], n, r)
    everything = MT.evaluate_results(res, device='cpu', pairs='all', dataroot=data, regions=('lower',), names='l1')
    assert list(everything) == ['l1', 'count', 'pairs', 'l1_lower', 'count_lower'] and everything['count'] == 3 and everything['count_lower'] == 2


def test_evaluate_results_region_errors(tmp_path):
    from training import metrics as MT
    res, data, _ = write_region_results(str(tmp_path), np.random.default_rng(26))
    with pytest.raises(ValueError, match='needs --dataroot'):
        MT.evaluate_results(res, device='cpu', regions='upper')
    with pytest.raises(ValueError, match='no predicted parsing'):
        MT.evaluate_results(res, device='cpu', names='ssim,parsing')
    with pytest.raises(ValueError, match='unknown region'):
        MT.evaluate_results(res, device='cpu', dataroot=data, regions='hat')
    PIL.fromarray(np.zeros((20, 16), np.uint8), 'L').save(os.path.join(data, 'parsing', 'p2.png'))
    with pytest.raises(ValueError, match=r'p2___p2\.png.*20 x 20.*24 x 24'):
        MT.evaluate_results(res, device='cpu', dataroot=data, regions='upper')
    os.remove(os.path.join(data, 'parsing', 'p1.png'))
    with pytest.raises(ValueError, match=r'p1___p1\.png.*no parsing image'):
        MT.evaluate_results(res, device='cpu', dataroot=data, regions='upper')


def test_command_line_with_regions(tmp_path):
    res, data, panels = write_region_results(str(tmp_path), np.random.default_rng(27))
    cli = os.path.join(PKG, 'calc_metrics.py')
    run = subprocess.run([sys.executable, cli, '--results', res, '--device', 'cpu', '--dataroot', data, '--regions', 'upper,lower'], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    want, _ = region_reference(panels, ['p1___p1.png', 'p2___p2.png'], ('l1', 'psnr', 'ssim'), ('upper', 'lower'))
    assert list(out) == ['l1', 'psnr', 'ssim', 'count', 'pairs', 'l1_upper', 'psnr_upper', 'ssim_upper', 'count_upper', 'l1_lower', 'psnr_lower',
                         'ssim_lower', 'count_lower']
    assert out['count_lower'] == 1 and out['ssim_upper'] == pytest.approx(want['ssim_upper'], abs=1e-12)
    run = subprocess.run([sys.executable, cli, '--results', res, '--device', 'cpu', '--regions', 'upper'], capture_output=True, text=True)
    assert run.returncode != 0 and '--regions needs --dataroot' in run.stderr and not run.stdout.strip()
