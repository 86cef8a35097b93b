"""``pg_region_pair_metrics_u8`` and ``pg_label_confusion_u8`` (csrc/region_metrics.hip) on the GPU against the restatement
(tests/region_metrics_ref.py), and the layers above them.

The cases, their eight regions and what they claim are those of tests/test_region_metrics_cpu.py (`build_cases`: 11 x 11, 42 x 42 = one tile, 43 x 47
and 75 x 53 = ragged second tile row / column, C = 1 and 3, every pair kind with the flat ones; one-pixel, empty, border-only, overlapping and
every-label regions, labels >= 32, a patch across the tile seam).

Bars.  n, sad, ssd, positions and every confusion entry: equal.  l1 / mse / psnr: rel 1e-13 (exact sums, float64 afterwards); NaN and +inf asserted
as such.  SSIM per (case, region): |kernel - float64| <= max(1e-6, 2 e32), e32 = the deviation of the float32 restatement on inputs minus 127.5 over
the same centre mask -- the bar of tests/test_image_metrics_gpu.py, taken per region.  A region of few positions has no mean to average its roundings
away, which is why e32 is taken over the region's own mask."""

import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import image_metrics_ref as R
import region_metrics_ref as RR

pytestmark = pytest.mark.gpu

from test_region_metrics_cpu import (REGIONS8, Case, build_cases, check_table, confusion_jobs, grey_luts, grid_reference, gt_windows, jobs_of,      # noqa: E402
                                     make_labels, noise, nudge, region_reference, write_region_results)
from test_snapshot_grid_cpu import write_vis_root                                   # noqa: E402

PIL = pytest.importorskip('PIL.Image')

DEFAULT3 = ((1, 4), (2, 3), (5, 6))


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def counted(M):
    M.launch_counter = dict(regions=0, confusion=0)
    return M.launch_counter


def test_every_case_in_one_launch_of_mixed_shapes():
    """All shapes, contents and channel counts as ONE job table with R = 8."""
    from torch_utils.ops import image_metrics as IM
    from torch_utils.ops import region_metrics as M
    dev = _cuda()
    cases_ = build_cases()
    jobs = jobs_of(cases_, dev)
    counter = counted(M)
    try:
        res = M.region_metrics_table(jobs, REGIONS8)
        assert counter == dict(regions=1, confusion=0)
    finally:
        M.launch_counter = None
    assert res['n'].dtype == res['positions'].dtype == torch.int64 and res['ssim'].dtype == res['l1'].dtype == torch.float64 and res['ssim'].is_cuda
    assert res['n'].shape == res['psnr'].shape == (len(cases_), 8)
    print('worst dev/bar', check_table(res, cases_, label='gpu '))
    # the region of every label against the unmasked kernel, on labels that are all < 32: sums equal, SSIM within the case's bar
    low = [(a, b, lab % 32) for a, b, lab in jobs]
    whole = M.region_metrics_table(low, [tuple(range(32))])
    plain = IM.pair_metrics_table([(a, b) for a, b, _ in jobs])
    assert torch.equal(whole['sad'][:, 0], plain['sad']) and torch.equal(whole['ssd'][:, 0], plain['ssd'])
    assert whole['n'][:, 0].tolist() == [cs.a.shape[0] * cs.a.shape[1] for cs in cases_]
    assert whole['positions'][:, 0].tolist() == [(cs.a.shape[0] - 10) * (cs.a.shape[1] - 10) for cs in cases_]
    for cs, x, y in zip(cases_, whole['ssim'][:, 0].tolist(), plain['ssim'].tolist()):
        want = R.ssim_separable(cs.a, cs.b)
        bar = max(1e-6, 2 * abs(R.ssim_f32(cs.a, cs.b) - want))                                # the unmasked kernel's own bar for this pair
        assert abs(x - want) <= bar and abs(y - want) <= bar, (cs.name, x, y, want, bar)


def test_one_region_and_default_regions():
    """R = 1 and R = 3 take the same tiles: each region's figures do not depend on which other regions share the call."""
    from torch_utils.ops import region_metrics as M
    dev = _cuda()
    cases_ = build_cases()[12:30]
    jobs = jobs_of(cases_, dev)
    all8 = M.region_metrics_table(jobs, REGIONS8)
    for r in (0, 3, 6):
        one = M.region_metrics_table(jobs, [REGIONS8[r]])
        check_table(one, [Case(cs.name, cs.a, cs.b, cs.labels, [REGIONS8[r]]) for cs in cases_])
        for k in one:
            assert torch.equal(one[k][:, 0].view(torch.int64), all8[k][:, r].view(torch.int64)), (r, k)


@pytest.mark.parametrize('J', [1, 37])
def test_batches_are_bit_identical_run_to_run_and_pair_by_pair(J):
    from torch_utils.ops import region_metrics as M
    dev = _cuda()
    rng = np.random.default_rng(30 + J)
    a = noise(rng, (J, 43, 75, 3))
    b = np.stack([nudge(rng, a[j], 1 + j % 20) for j in range(J)])
    labs = np.stack([make_labels(rng, 43, 75) for _ in range(J)])
    ta, tb, tl = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(labs).to(dev)
    jobs = [(ta[j], tb[j], tl[j]) for j in range(J)]
    one, two = M.region_metrics_table(jobs, DEFAULT3), M.region_metrics_table(jobs, DEFAULT3)
    singles = [M.region_metrics_table(jobs[j:j + 1], DEFAULT3) for j in range(J)]
    for k in one:
        assert one[k].shape == (J, 3)
        assert torch.equal(one[k].view(torch.int64), two[k].view(torch.int64)), k
        assert torch.equal(one[k].view(torch.int64), torch.cat([s[k] for s in singles]).view(torch.int64)), k
    check_table({k: v[::9] for k, v in one.items()}, [Case(f'pair {j}', a[j], b[j], labs[j], DEFAULT3) for j in range(0, J, 9)])


def test_windows_and_label_views_at_odd_offsets():
    """Image windows of one parent at odd byte offsets (row pitch 291), pixel stride above C (3 of 4 channels, and 1 of 4); label views: a window of a
    [64, 97] parent at an odd base (row stride 97 > w, every row at another alignment: the dword path's ragged ends) and one channel of a
    [70, 120, 3] parent at an odd base (row stride 360, pixel stride 3: the byte path)."""
    from torch_utils.ops import region_metrics as M
    dev = _cuda()
    rng = np.random.default_rng(31)
    parent, other = torch.from_numpy(noise(rng, (64, 97, 3))).to(dev), torch.from_numpy(noise(rng, (64, 97, 3))).to(dev)
    grey = torch.from_numpy(noise(rng, (64, 97, 1))).to(dev)
    wide = torch.from_numpy(noise(rng, (50, 60, 4))).to(dev)
    lab = torch.from_numpy(np.pad(make_labels(rng, 60, 90), ((2, 2), (3, 4)), constant_values=1)).to(dev)             # [64, 97]
    lab3 = torch.from_numpy(np.stack([make_labels(rng, 70, 120) for _ in range(3)], axis=2)).to(dev)                  # [70, 120, 3]
    jobs = [(parent[2:2 + 43, 3:3 + 75], other[2:2 + 43, 3:3 + 75], lab[2:2 + 43, 3:3 + 75]),
            (parent[2:2 + 43, 3:3 + 45], parent[19:19 + 43, 50:50 + 45], lab3[3:3 + 43, 5:5 + 45, 0]),
            (parent[2:62, 3:20], parent[2:62, 3:20], lab[1:61, 8:25]),
            (grey[2:2 + 43, 3:3 + 75], grey[21:21 + 43, 22:22 + 75], lab3[4:4 + 43, 6:6 + 75, 2]),
            (wide[1:44, 2:50, :3], wide[3:46, 5:53, 1:], lab[7:50, 9:57]),
            (wide[1:44, 2:50, 3:], wide[3:46, 5:53, :1], lab3[9:52, 1:49, 1])]
    assert jobs[0][2].data_ptr() % 2 == 1 and jobs[0][2].stride(0) == 97 and jobs[1][2].data_ptr() % 2 == 1 and jobs[1][2].stride() == (360, 3)
    regions = DEFAULT3 + ((0, 31), (8,))
    res = M.region_metrics_table(jobs, regions)
    check_table(res, [Case(f'view {j}', a.cpu().numpy(), b.cpu().numpy(), l.cpu().numpy(), regions) for j, (a, b, l) in enumerate(jobs)])
    assert int(res['sad'][2].sum()) == 0 and float(res['psnr'][2, 0]) == math.inf                                       # identical windows


def test_bad_arguments_are_refused_and_nothing_is_launched():
    from torch_utils.ops import _native as nat
    from torch_utils.ops import region_metrics as M
    dev = _cuda()
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    ok = (z(20, 20, 3), z(20, 20, 3), z(20, 20))
    p7, t7 = grey_luts()
    counter = counted(M)
    try:
        for regions in ([], [(0,)] * 9, [(32,)], [(-1,)]):
            with pytest.raises(nat.NativeOpError):
                M.region_metrics_table([ok], regions)
        for job in ((z(10, 20, 3), z(10, 20, 3), z(10, 20)), (z(20, 10, 1), z(20, 10, 1), z(20, 10)), (z(20, 20, 2), z(20, 20, 2), z(20, 20)),
                    (z(20, 20, 3), z(20, 20, 3), z(20, 21)), (z(20, 20, 3), z(20, 20, 3), z(20, 20).float()), (z(20, 20, 3), z(21, 20, 3), z(20, 20)),
                    (z(20, 3, 20).permute(0, 2, 1), z(20, 20, 3), z(20, 20)), (z(20, 20, 3), z(20, 20, 3), z(20, 20).cpu())):
            with pytest.raises(nat.NativeOpError):
                M.region_metrics_table([job], [(0,)])
        for args in ((np.arange(256), t7, 7), (p7, t7, 0), (p7, t7, 17), (p7, t7, 6), (p7[:100], t7, 7)):
            with pytest.raises(nat.NativeOpError):
                M.label_confusion_table([(z(3, 5), z(3, 5))], *args)
        for job in ((z(3, 5), z(3, 6)), (z(3, 5, 1), z(3, 5, 1)), (z(0, 5), z(0, 5)), (z(3, 5).float(), z(3, 5))):
            with pytest.raises(nat.NativeOpError):
                M.label_confusion_table([job], p7, t7, 7)
        assert counter == dict(regions=0, confusion=0)
    finally:
        M.launch_counter = None
    # the C entry points themselves: negative status, and the outputs keep their bytes
    lib = M._init().lib
    img, lab = z(20, 20, 3), z(20, 20)
    counts = torch.full([4 * 8], -7, dtype=torch.int64, device=dev)
    ssim = torch.full([8], -7.0, dtype=torch.float64, device=dev)
    conf = torch.full([49], -7, dtype=torch.int64, device=dev)
    work = torch.empty([256], dtype=torch.int64, device=dev)
    bits = np.array([1, 2, 4, 8, 16, 32, 64, 128, 256], dtype=np.uint32)

    def call(n=1, R=1, table=True, regions=True, **fields):
        t = np.zeros(1, dtype=M._RPAIR_DT)
        t['a'], t['b'], t['labels'] = img.data_ptr(), img.data_ptr(), lab.data_ptr()
        t['a_row_stride'], t['b_row_stride'], t['l_row_stride'], t['a_pix_stride'], t['b_pix_stride'], t['l_pix_stride'] = 60, 60, 20, 3, 3, 1
        t['h'], t['w'], t['channels'] = 20, 20, 3
        for k, v in fields.items():
            t[k] = v
        host = t.ctypes.data_as(ctypes.c_void_p) if table else None
        tab = torch.from_numpy(t.view(np.uint8).reshape(-1)).to(dev)
        ws = lib.pg_region_pair_metrics_workspace(host, n, R)
        st = lib.pg_region_pair_metrics_u8(host, tab.data_ptr() if table else None, n, bits.ctypes.data_as(ctypes.c_void_p) if regions else None, R,
                                           work.data_ptr(), counts.data_ptr(), ssim.data_ptr(), None)
        return ws, st
    for kw in (dict(h=10), dict(w=10), dict(channels=2), dict(channels=4), dict(n=0), dict(n=-1), dict(table=False), dict(a=0), dict(labels=0),
               dict(a_pix_stride=2), dict(l_pix_stride=0), dict(b_row_stride=0), dict(l_row_stride=0), dict(R=0), dict(R=9)):
        ws, st = call(**kw)
        assert ws == st == -1, kw
    assert call(regions=False)[1] == -1
    assert call(n=70000)[1] == -3 and call(h=65536, w=65536)[1] == -3

    def confusion_call(n=1, K=7, table=True, pred_lut=p7, **fields):
        t = np.zeros(1, dtype=M._LPAIR_DT)
        t['pred'], t['target'], t['p_row_stride'], t['t_row_stride'], t['p_pix_stride'], t['t_pix_stride'], t['h'], t['w'] = (
            img.data_ptr(), lab.data_ptr(), 60, 20, 3, 1, 20, 20)
        for k, v in fields.items():
            t[k] = v
        tab = torch.from_numpy(t.view(np.uint8).reshape(-1)).to(dev)
        return lib.pg_label_confusion_u8(t.ctypes.data_as(ctypes.c_void_p) if table else None, tab.data_ptr(), n,
                                         pred_lut.ctypes.data_as(ctypes.c_void_p) if pred_lut is not None else None, t7.ctypes.data_as(ctypes.c_void_p), K,
                                         conf.data_ptr(), None)
    for kw in (dict(n=0), dict(n=-1), dict(K=0), dict(K=17), dict(K=6), dict(table=False), dict(pred_lut=None), dict(pred=0), dict(target=0), dict(h=0),
               dict(w=0), dict(p_pix_stride=0), dict(t_pix_stride=0), dict(p_row_stride=0), dict(t_row_stride=0)):
        assert confusion_call(**kw) == -1, kw
    assert confusion_call(n=70000) == -3 and confusion_call(h=65536, w=65536) == -3
    torch.cuda.synchronize()
    assert counts.tolist() == [-7] * 32 and ssim.tolist() == [-7.0] * 8 and conf.tolist() == [-7] * 49
    # ... and the accepted calls: one region of label 0 over an all-zero pair; the confusion ADDS to its table
    ws, st = call()
    assert ws == 24 and st == 0
    assert confusion_call() == 0
    torch.cuda.synchronize()
    assert counts.tolist()[:4] == [400, 0, 0, 100] and ssim.tolist()[0] == 300.0
    assert conf.tolist()[0] == 400 - 7 and conf.tolist()[1:] == [-7] * 48


def test_no_host_synchronisation():
    from torch_utils.ops import region_metrics as M
    dev = _cuda()
    rng = np.random.default_rng(33)
    a, b = torch.from_numpy(noise(rng, (3, 43, 45, 3))).to(dev), torch.from_numpy(noise(rng, (3, 43, 45, 3))).to(dev)
    lab = torch.from_numpy(np.stack([make_labels(rng, 43, 45) for _ in range(3)])).to(dev)
    jobs = [(a[j], b[j], lab[j]) for j in range(3)]
    p7, t7 = grey_luts()
    pairs = [(a[j, :, :, 0], lab[j]) for j in range(3)]
    warm = M.region_metrics_table(jobs, DEFAULT3)
    warm_c = M.label_confusion_table(pairs, p7, t7, 7)
    M.parsing_scores(warm_c)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = M.region_metrics_table(jobs, DEFAULT3)
        mean = torch.stack([torch.nanmean(res[k], dim=0) for k in ('l1', 'psnr', 'ssim')])
        conf = M.label_confusion_table(pairs, p7, t7, 7)
        scores = M.parsing_scores(conf)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(res['ssim'].view(torch.int64), warm['ssim'].view(torch.int64)) and mean.shape == (3, 3)
    assert torch.equal(conf, warm_c) and scores['iou'].shape == (7,) and scores['acc'].is_cuda


# ------------------------------------------------------------------------------------------------------------- the confusion count

def test_confusion_equals_the_restatement_in_one_launch():
    from torch_utils.ops import region_metrics as M
    dev = _cuda()
    jobs = confusion_jobs(np.random.default_rng(34))
    on = lambda t: (t._base if t._base is not None else t).to(dev).as_strided(t.shape, t.stride(), t.storage_offset())      # the same view, on the device
    counter = counted(M)
    try:
        got = M.label_confusion_table([(on(p), on(t)) for p, t, _, _, _ in jobs[:3]], jobs[0][2], jobs[0][3], 7)
        assert counter == dict(regions=0, confusion=1)
        p, t, pl, tl, K = jobs[3]
        got16 = M.label_confusion_table([(on(p), on(t))], pl, tl, K)
    finally:
        M.launch_counter = None
    assert got.dtype == torch.int64 and got.shape == (3, 7, 7) and got.is_cuda and on(jobs[1][0]).stride(1) == 3 and on(t).stride(1) == 2
    for j, (p, t, pl, tl, K) in enumerate(jobs[:3]):
        assert np.array_equal(got[j].cpu().numpy(), RR.confusion(p.numpy(), t.numpy(), pl, tl, K)), j
    p, t, pl, tl, K = jobs[3]
    want = RR.confusion(p.numpy(), t.numpy(), pl, tl, K)
    assert np.array_equal(got16[0].cpu().numpy(), want) and (want > 0).sum() > 150
    again = M.label_confusion_table([(on(p), on(t)) for p, t, _, _, _ in jobs[:3]], jobs[0][2], jobs[0][3], 7)
    assert torch.equal(got, again)
    s, (acc, iou, miou) = M.parsing_scores(got), RR.parsing_scores(got.sum(dim=0).cpu().numpy())
    assert float(s['acc']) == pytest.approx(acc, rel=1e-14) and float(s['miou']) == pytest.approx(miou, rel=1e-14)
    assert np.allclose(s['iou'].cpu().numpy(), iou, rtol=1e-14, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------- the layers above

@pytest.fixture(scope='module')
def vis_root(tmp_path_factory):
    return write_vis_root(str(tmp_path_factory.mktemp('vis_region_metrics_gpu')))


def test_grid_reconstruction_with_regions_and_parsing_on_a_gpu_grid(vis_root):
    """One region launch and one confusion launch on top of today's pair launch; the figures against the restatement on the downloaded grids."""
    from training import metrics as MT
    from training import snapshot_grid as S
    from training import training_loop as T
    from training.dataset import TrainSet
    from torch_utils.ops import image_metrics as IM
    from torch_utils.ops import region_metrics as M
    _cuda()
    grid = S.setup_snapshot_grid(TrainSet(vis_root, shuffle=False, device='cpu'), 'cuda')
    torch.manual_seed(0)
    G = T.build_networks(4, 'cuda', dict(channel_base=4096, channel_max=512))[0].eval().requires_grad_(False)
    fin_grid, par_grid = grid.render(G, 4)
    gts = gt_windows(vis_root)
    regions = ('upper', 'lower', 'skin')
    counter = counted(M)
    IM.launch_counter = dict(pairs=0)
    try:
        assert list(MT.grid_reconstruction(grid, ('l1', 'psnr', 'ssim'))) == ['Metric/recon_l1', 'Metric/recon_psnr', 'Metric/recon_ssim']
        assert counter == dict(regions=0, confusion=0) and IM.launch_counter == dict(pairs=1)
        got = MT.grid_reconstruction(grid, ('l1', 'psnr', 'ssim', 'parsing'), regions)
        assert counter == dict(regions=1, confusion=1) and IM.launch_counter == dict(pairs=2)
    finally:
        M.launch_counter = IM.launch_counter = None
    want, per = grid_reference(fin_grid, par_grid, gts, ('l1', 'psnr', 'ssim'), regions, True)
    assert set(list(got)[3:]) == set(want) and len(want) == 11
    jobs = [(a, b, lab) for (a, b), lab in zip(MT.grid_pairs(grid), MT.grid_labels(grid))]
    cs = [Case(f'cell {i}', a.cpu().numpy(), b.cpu().numpy(), lab.cpu().numpy(), [MT.REGIONS[r] for r in regions]) for i, (a, b, lab) in enumerate(jobs)]
    for c, p in zip(cs, per):
        assert [w['sad'] for w in c.want] == [p[r]['sad'] for r in regions]                    # the views are the cells the restatement cuts
    check_table(M.region_metrics_table(jobs, [MT.REGIONS[r] for r in regions]), cs, label='grid ')
    for k, v in want.items():
        if k.startswith('Metric/recon_ssim_'):
            r = regions.index(k.rsplit('_', 1)[1])
            assert abs(got[k] - v) <= max(c.bar[r] for c in cs), k
        else:
            assert got[k] == pytest.approx(v, rel=1e-13), k                                    # exact sums / counts -> the definitions' float64


def test_driver_writes_the_region_and_parsing_keys_on_image_ticks(vis_root, tmp_path, capsys):
    from training import training_loop as T
    _cuda()
    run = str(tmp_path / 'run')
    T.training_loop(run, vis_root, batch=2, batch_gpu=2, kimg=0.006, tick=0.002, snap=None, image_snap=2, seed=3, workers=0, device='cuda',
                    width=dict(channel_base=4096, channel_max=512), dataset_kwargs=dict(shuffle=False), metrics='ssim,parsing', metric_regions='upper,skin')
    lines = [json.loads(line) for line in open(os.path.join(run, 'stats.jsonl'))]
    assert [line['Progress/tick'] for line in lines] == [0, 1, 2]
    keys = {'Metric/recon_ssim', 'Metric/recon_ssim_upper', 'Metric/recon_ssim_skin', 'Metric/parsing_acc', 'Metric/parsing_miou'}
    for line in lines:
        assert {k for k in line if k.startswith('Metric/')} == (keys if line['Progress/tick'] in (0, 2) else set()), line
    fin, par = (np.array(PIL.open(os.path.join(run, f'fakes000000_{n}.png'))) for n in ('finetune', 'parsing'))
    want, per = grid_reference(fin, par, gt_windows(vis_root), ('ssim',), ('upper', 'skin'), True)     # (the files hold the last image tick's grids)
    for k, v in want.items():
        if k.startswith('Metric/recon_ssim_'):
            r = k.rsplit('_', 1)[1]
            bar = max(max(1e-6, 2 * abs(p[r]['ssim32'] - p[r]['ssim'])) for p in per if p[r]['positions'])
            assert abs(lines[2][k] - v) <= bar, (k, lines[2][k], v, bar)
        else:
            assert lines[2][k] == pytest.approx(v, rel=1e-13), k


def test_evaluate_results_with_regions_on_the_gpu_equals_the_cpu_route(tmp_path):
    from training import metrics as MT
    _cuda()
    res, data, panels = write_region_results(str(tmp_path), np.random.default_rng(35))
    files = ['p1___p1.png', 'p2___p2.png']
    regions = ('upper', 'lower', 'skin')
    per = {d: str(tmp_path / f'per_{d}.jsonl') for d in ('cpu', 'cuda')}
    out = {d: MT.evaluate_results(res, device=d, batch=2, per_file=per[d], dataroot=data, regions=regions) for d in ('cpu', 'cuda')}
    want, ref = region_reference(panels, files, ('l1', 'psnr', 'ssim'), regions)
    assert list(out['cuda']) == list(out['cpu']) and out['cuda']['count_lower'] == out['cpu']['count_lower'] == 1
    cs = [Case(f, *panels[f], [MT.REGIONS[r] for r in regions]) for f in files]
    lines = {d: [json.loads(line) for line in open(per[d])] for d in per}
    for j, f in enumerate(files):
        for k, r in enumerate(regions):
            for n in ('l1', 'psnr', 'ssim'):
                c, g, w = lines['cpu'][j][f'{n}_{r}'], lines['cuda'][j][f'{n}_{r}'], ref[j][r][n]
                if math.isnan(w):
                    assert c is None and g is None, (f, n, r)
                elif n == 'ssim':
                    assert abs(c - w) <= 1e-12 and abs(g - w) <= cs[j].bar[k], (f, r)
                else:
                    assert c == pytest.approx(w, rel=1e-13) and g == pytest.approx(w, rel=1e-13), (f, n, r)
    for key, w in want.items():
        if key.startswith('ssim_'):
            assert abs(out['cuda'][key] - w) <= max(c.bar[regions.index(key[5:])] for c in cs), key
        else:
            assert out['cuda'][key] == pytest.approx(w, rel=1e-13), key
