"""``pg_image_pair_metrics_u8`` (csrc/image_metrics.hip) on the GPU against the float64 restatement (tests/image_metrics_ref.py), and the layers above it.

The kernel's tile is TILE x TILE = 32 x 32 SSIM positions, i.e. 42 x 42 pixels: per direction the extents 41, 42, 43 (TILE + 10 - 1, + 10, + 10 + 1:
one tile short by one, one full tile, one tile plus a one-position second tile) and 75 (two tiles + 10 + 1: a third tile of one position) are
covered, besides the single window 11 x 11 and 12 x 27.

Bars.  sad / ssd are integers: equal.  SSIM: |kernel - float64| <= max(1e-6, 2 e32), e32 = the deviation of the float32 restatement on inputs minus
127.5 (computed here, per case); 1e-6 is the floor for well-conditioned pairs (a handful of float32 roundings on O(1) quantities, then a mean).  The
flat cases are there on purpose: e32 is ~1e-5 there and a float32 evaluation on raw levels several times worse, which the bar refuses (checked on the
restatement's raw-level variant).  The references are computed once per module."""

import ctypes
import json
import os

import numpy as np
import pytest
import torch

import image_metrics_ref as R

pytestmark = pytest.mark.gpu

from test_image_metrics_cpu import grid_reference, noise, nudge, write_triptychs      # noqa: E402
from test_snapshot_grid_cpu import write_vis_root                                   # noqa: E402

TILE = 32
EDGE = (TILE + 9, TILE + 10, TILE + 11, 2 * TILE + 11)
SHAPES = [(11, 11), (12, 27)] + [(e, 12) for e in EDGE] + [(12, e) for e in EDGE] + [(2 * TILE + 11, TILE + 11)]
KINDS = ('noise', 'noise+-3', 'sine+-3', 'sine+-20', 'flat+-1', 'flat 200/255', 'identical')


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def make_pair(rng, kind, h, w, c):
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


class Case:
    def __init__(self, name, a, b):
        self.name, self.a, self.b = name, a, b
        self.want = R.metrics(a, b)
        self.e32 = abs(R.ssim_f32(a, b) - self.want['ssim'])
        self.raw = abs(R.ssim_f32(a, b, 0.0) - self.want['ssim'])
        self.bar = max(1e-6, 2 * self.e32)


@pytest.fixture(scope='module')
def cases():
    rng = np.random.default_rng(11)
    return [Case(f'{kind} {h}x{w}x{c}', *make_pair(rng, kind, h, w, c)) for (h, w) in SHAPES for c in (1, 3) for kind in KINDS]


def check(res, cases_, label=''):
    sad, ssd, ssim = res['sad'].cpu().tolist(), res['ssd'].cpu().tolist(), res['ssim'].cpu().tolist()
    worst = 0.0
    for j, cs in enumerate(cases_):
        dev = abs(ssim[j] - cs.want['ssim'])
        worst = max(worst, dev / cs.bar)
        print(f'{label}{cs.name:28s} ssim {cs.want["ssim"]:+.9f} dev {dev:.2e} e32 {cs.e32:.2e} raw {cs.raw:.2e} dev/bar {dev / cs.bar:.3f}')
        assert sad[j] == cs.want['sad'] and ssd[j] == cs.want['ssd'], cs.name
        assert dev <= cs.bar, (cs.name, dev, cs.bar)
    return worst


def test_every_case_in_one_launch_of_mixed_shapes(cases):
    """All shapes, contents and channel counts as ONE job table: exact sums, SSIM within the bar; the derived figures are the definitions' float64."""
    from torch_utils.ops import image_metrics as M
    dev = _cuda()
    M.launch_counter = dict(pairs=0)
    try:
        res = M.pair_metrics_table([(torch.from_numpy(cs.a).to(dev), torch.from_numpy(cs.b).to(dev)) for cs in cases])
        assert M.launch_counter == dict(pairs=1)
    finally:
        M.launch_counter = None
    assert res['sad'].dtype == res['ssd'].dtype == torch.int64 and res['ssim'].dtype == res['psnr'].dtype == torch.float64 and res['l1'].is_cuda
    print('worst dev/bar', check(res, cases))
    l1, mse, psnr = res['l1'].cpu().tolist(), res['mse'].cpu().tolist(), res['psnr'].cpu().tolist()
    for j, cs in enumerate(cases):
        assert l1[j] == pytest.approx(cs.want['l1'], rel=1e-14) and mse[j] == pytest.approx(cs.want['mse'], rel=1e-14)
        assert psnr[j] == pytest.approx(cs.want['psnr'], rel=1e-12) if cs.want['ssd'] else psnr[j] == float('inf')
    # the bar tells the two float32 evaluations apart: on the flat, jittered images a raw-level evaluation is refused
    flat = [cs for cs in cases if cs.name.startswith('flat+-1') and cs.a.shape[0] * cs.a.shape[1] >= 12 * 41]
    print('flat+-1 raw / e32:', ' '.join(f'{cs.raw / cs.e32:.1f}' for cs in flat))
    assert flat and all(cs.raw > cs.bar for cs in flat)


@pytest.mark.parametrize('J', [1, 37])
def test_batches_are_bit_identical_run_to_run_and_pair_by_pair(J):
    from torch_utils.ops import image_metrics as M
    dev = _cuda()
    rng = np.random.default_rng(J)
    a = noise(rng, (J, 43, 75, 3))
    b = np.stack([nudge(rng, a[j], 1 + j % 20) for j in range(J)])
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    one, two = M.pair_metrics(ta, tb), M.pair_metrics(ta, tb)
    singles = [M.pair_metrics(ta[j:j + 1], tb[j:j + 1]) for j in range(J)]
    for k in one:
        assert one[k].shape == (J,)
        assert torch.equal(one[k].view(torch.int64), two[k].view(torch.int64)), k
        assert torch.equal(one[k].view(torch.int64), torch.cat([s[k] for s in singles]).view(torch.int64)), k
    check({k: v[::9] for k, v in one.items()}, [Case(f'pair {j}', a[j], b[j]) for j in range(0, J, 9)])


def test_windows_of_one_parent_at_odd_offsets():
    """x0 = 3, y0 = 2 in a 64 x 97 x 3 parent (row pitch 291 bytes: every row starts at another byte alignment); both windows of a pair in the same
    parent, as in the snapshot grid; a 1-channel parent; 3 of the 4 channels of a wider pixel (pixel stride > C: the byte path)."""
    from torch_utils.ops import image_metrics as M
    dev = _cuda()
    rng = np.random.default_rng(12)
    parent, other = torch.from_numpy(noise(rng, (64, 97, 3))).to(dev), torch.from_numpy(noise(rng, (64, 97, 3))).to(dev)
    grey = torch.from_numpy(noise(rng, (64, 97, 1))).to(dev)
    wide = torch.from_numpy(noise(rng, (50, 60, 4))).to(dev)
    jobs = [(parent[2:2 + 43, 3:3 + 75], other[2:2 + 43, 3:3 + 75]), (parent[2:2 + 43, 3:3 + 45], parent[19:19 + 43, 50:50 + 45]),
            (parent[2:62, 3:20], parent[2:62, 3:20]), (grey[2:2 + 43, 3:3 + 75], grey[21:21 + 43, 22:22 + 75]),
            (wide[1:44, 2:50, :3], wide[3:46, 5:53, 1:]), (wide[1:44, 2:50, 3:], wide[3:46, 5:53, :1])]
    assert jobs[0][0].data_ptr() % 2 == 1 or jobs[0][0].stride(0) % 2 == 1
    res = M.pair_metrics_table(jobs)
    check(res, [Case(f'view {j}', a.cpu().numpy(), b.cpu().numpy()) for j, (a, b) in enumerate(jobs)])
    assert float(res['ssim'][2]) == 1.0 and int(res['sad'][2]) == 0


def test_bad_arguments_are_refused_and_nothing_is_launched():
    from torch_utils.ops import _native as nat
    from torch_utils.ops import image_metrics as M
    dev = _cuda()
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    M.launch_counter = dict(pairs=0)
    try:
        for a, b in ((z(1, 10, 20, 3), z(1, 10, 20, 3)), (z(1, 20, 10, 1), z(1, 20, 10, 1)), (z(1, 20, 20, 2), z(1, 20, 20, 2)),
                     (z(0, 20, 20, 3), z(0, 20, 20, 3)), (z(1, 20, 20, 3), z(1, 21, 20, 3)), (z(1, 20, 20, 3), z(1, 20, 20, 3).float())):
            with pytest.raises(nat.NativeOpError):
                M.pair_metrics(a, b)
        with pytest.raises(nat.NativeOpError):
            M.pair_metrics_table([(z(20, 3, 20).permute(0, 2, 1), z(20, 20, 3))])              # channel stride 20
    except BaseException:
        M.launch_counter = None
        raise
    assert M.launch_counter == dict(pairs=0)
    M.launch_counter = None
    # the C entry point itself: negative status, and the outputs keep their bytes
    lib = M._init().lib
    img = z(20, 20, 3)
    out = torch.full([3], -7, dtype=torch.int64, device=dev)
    ssim = torch.full([1], -7.0, dtype=torch.float32, device=dev)
    work = torch.empty([64], dtype=torch.int64, device=dev)

    def call(n=1, table=True, **fields):
        t = np.zeros(1, dtype=M._PAIR_DT)
        t['a'], t['b'], t['a_row_stride'], t['b_row_stride'], t['a_pix_stride'], t['b_pix_stride'] = img.data_ptr(), img.data_ptr(), 60, 60, 3, 3
        t['h'], t['w'], t['channels'] = 20, 20, 3
        for k, v in fields.items():
            t[k] = v
        host = t.ctypes.data_as(ctypes.c_void_p) if table else None
        tab = torch.from_numpy(t.view(np.uint8).reshape(-1)).to(dev)
        ws = lib.pg_image_pair_metrics_workspace(host, n)
        st = lib.pg_image_pair_metrics_u8(host, tab.data_ptr() if table else None, n, work.data_ptr(), out[0:].data_ptr(), out[1:].data_ptr(),
                                          ssim.data_ptr(), None)
        return ws, st
    for kw in (dict(h=10), dict(w=10), dict(channels=2), dict(channels=4), dict(n=0), dict(n=-1), dict(table=False), dict(a=0), dict(a_pix_stride=2),
               dict(b_row_stride=0)):
        ws, st = call(**kw)
        assert ws == st == -1, kw
    assert call(n=70000)[1] == -3 and call(h=65536, w=65536)[1] == -3
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7, -7] and ssim.tolist() == [-7.0]
    ws, st = call()
    assert ws == 24 and st == 0
    torch.cuda.synchronize()
    assert out.tolist()[:2] == [0, 0] and ssim.tolist() == [1.0]


def test_no_host_synchronisation():
    from torch_utils.ops import image_metrics as M
    dev = _cuda()
    rng = np.random.default_rng(13)
    a, b = torch.from_numpy(noise(rng, (3, 43, 45, 3))).to(dev), torch.from_numpy(noise(rng, (3, 43, 45, 3))).to(dev)
    warm = M.pair_metrics(a, b)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = M.pair_metrics(a, b)
        mean = torch.stack([res[k].mean() for k in ('l1', 'psnr', 'ssim')])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(res['ssim'], warm['ssim']) and mean.shape == (3,)


# ------------------------------------------------------------------------------------------------------------- the layers above

@pytest.fixture(scope='module')
def vis_root(tmp_path_factory):
    return write_vis_root(str(tmp_path_factory.mktemp('vis_metrics_gpu')))


def test_grid_reconstruction_on_a_gpu_grid(vis_root):
    from training import metrics as MT
    from training import snapshot_grid as S
    from training import training_loop as T
    from training.dataset import TrainSet
    from torch_utils.ops import image_metrics as M
    _cuda()
    grid = S.setup_snapshot_grid(TrainSet(vis_root, shuffle=False, device='cpu'), 'cuda')
    torch.manual_seed(0)
    G = T.build_networks(4, 'cuda', dict(channel_base=4096, channel_max=512))[0].eval().requires_grad_(False)
    fin_grid, _ = grid.render(G, 4)
    got = MT.grid_reconstruction(grid, ('l1', 'psnr', 'ssim'))
    want, per = grid_reference(fin_grid, 3, ('l1', 'psnr', 'ssim'))
    pairs = MT.grid_pairs(grid)
    assert len(pairs) == 3 and pairs[0][0].shape == (512, 320, 3)
    cs = [Case(f'cell {i}', a.cpu().numpy(), b.cpu().numpy()) for i, (a, b) in enumerate(pairs)]
    for c, p in zip(cs, per):
        assert c.want['sad'] == p['sad'] and c.want['ssim'] == p['ssim']                     # the views are the cells the restatement cuts
    check(M.pair_metrics_table(pairs), cs, 'grid ')
    assert got['Metric/recon_l1'] == pytest.approx(want['Metric/recon_l1'], rel=1e-13)       # sums exact -> the definitions' float64
    assert got['Metric/recon_psnr'] == pytest.approx(want['Metric/recon_psnr'], rel=1e-13)
    assert abs(got['Metric/recon_ssim'] - want['Metric/recon_ssim']) <= float(np.mean([c.bar for c in cs]))


def test_driver_writes_the_metrics_on_image_ticks_only(vis_root, tmp_path, capsys):
    from training import training_loop as T
    _cuda()
    run = str(tmp_path / 'run')
    T.training_loop(run, vis_root, batch=2, batch_gpu=2, kimg=0.006, tick=0.002, snap=None, image_snap=2, seed=3, workers=0, device='cuda',
                    width=dict(channel_base=4096, channel_max=512), dataset_kwargs=dict(shuffle=False), metrics=('l1', 'psnr', 'ssim'))
    lines = [json.loads(line) for line in open(os.path.join(run, 'stats.jsonl'))]
    assert [line['Progress/tick'] for line in lines] == [0, 1, 2]
    keys = {'Metric/recon_l1', 'Metric/recon_psnr', 'Metric/recon_ssim'}
    for line in lines:
        have = {k for k in line if k.startswith('Metric/')}
        assert have == (keys if line['Progress/tick'] in (0, 2) else set()), line
    for line in (lines[0], lines[2]):
        assert np.isfinite([line[k] for k in keys]).all() and -1 <= line['Metric/recon_ssim'] <= 1 and 0 < line['Metric/recon_l1'] <= 1
    assert capsys.readouterr().out.count('Metric/recon_ssim') == 2
    assert 'fakes000000_finetune.png' in os.listdir(run)                  # (both image ticks fall into kimg 0: one file name)


def test_evaluate_results_on_the_gpu_equals_the_cpu_route(tmp_path):
    from training import metrics as MT
    _cuda()
    rng = np.random.default_rng(14)
    panels = write_triptychs(str(tmp_path / 'res'), rng)
    res = str(tmp_path / 'res')
    files = {}
    for pairs in ('self', 'all'):
        for device in ('cpu', 'cuda'):
            files[device] = str(tmp_path / f'per_{device}.jsonl')
            out = MT.evaluate_results(res, pairs=pairs, device=device, batch=2, per_file=files[device])
            if device == 'cpu':
                want = out
        assert out['count'] == want['count'] and out['pairs'] == pairs
        assert out['l1'] == pytest.approx(want['l1'], rel=1e-13) and out['psnr'] == pytest.approx(want['psnr'], rel=1e-13)        # from exact sums
        cpu_lines, gpu_lines = ([json.loads(line) for line in open(files[d])] for d in ('cpu', 'cuda'))
        assert [line['file'] for line in cpu_lines] == [line['file'] for line in gpu_lines]
        for c, g in zip(cpu_lines, gpu_lines):
            cs = Case(c['file'], *panels[c['file']])
            assert g['l1'] == pytest.approx(c['l1'], rel=1e-13) and g['psnr'] == pytest.approx(c['psnr'], rel=1e-13)
            assert abs(c['ssim'] - cs.want['ssim']) <= 1e-12 and abs(g['ssim'] - cs.want['ssim']) <= cs.bar, c['file']
