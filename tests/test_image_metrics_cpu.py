"""The reconstruction metrics without a GPU: pins of the restatement (tests/image_metrics_ref.py), the op's CPU route against it, `grid_reconstruction`
on a CPU `SnapshotGrid`, `evaluate_results` / calc_metrics.py on synthetic triptychs, and the training driver's ``metrics`` hook.

The two driver runs are the slow part (one training image and, with metrics, nine generator passes at the narrowest width, on the CPU: ~30 s)."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_metrics_ref as R
from test_snapshot_grid_cpu import WIDTH, write_vis_root

PIL = pytest.importorskip('PIL.Image')

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pasta-gan-plusplus_amd')


def noise(rng, shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def nudge(rng, a, k):
    return np.clip(a.astype(np.int64) + rng.integers(-k, k + 1, a.shape), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- the restatement

def test_the_two_forms_of_the_restatement_agree():
    rng = np.random.default_rng(0)
    for shape in ((11, 11, 1), (12, 27, 3), (30, 23, 3)):
        a = noise(rng, shape)
        for b in (noise(rng, shape), nudge(rng, a, 3)):
            assert abs(R.ssim_separable(a, b) - R.ssim_window(a, b)) <= 1e-12
            assert abs(R.ssim_separable(a, b) - R.ssim_separable(b, a)) <= 1e-12                  # symmetric in (a, b)
    assert abs(R.taps().sum() - 1) < 1e-15 and R.taps().shape == (11,)


def test_identical_and_constant_images():
    rng = np.random.default_rng(1)
    a = noise(rng, (17, 19, 3))
    m = R.metrics(a, a.copy())
    assert m['ssim'] == 1.0 and m['psnr'] == math.inf and m['sad'] == 0 and m['ssd'] == 0 and m['l1'] == 0.0
    p, q = 200, 255
    got = R.ssim_separable(np.full((13, 15, 3), p, np.uint8), np.full((13, 15, 3), q, np.uint8))
    assert abs(got - (2 * p * q + R.C1) / (p * p + q * q + R.C1)) <= 1e-12
    assert abs(got - 0.971199117) < 1e-9


def test_integer_sums_by_hand():
    a = np.zeros((11, 11, 1), np.uint8)
    b = np.zeros((11, 11, 1), np.uint8)
    a[0, 0, 0], b[0, 0, 0] = 255, 0                     # |d| = 255
    a[3, 4, 0], b[3, 4, 0] = 10, 13                     # 3
    a[10, 10, 0], b[10, 10, 0] = 7, 1                   # 6
    assert R.sums(a, b) == (255 + 3 + 6, 255 * 255 + 9 + 36)
    m = R.metrics(a, b)
    assert m['l1'] == 264 / (255 * 121) and m['mse'] == 65070 / 121 and abs(m['psnr'] - 10 * math.log10(65025 * 121 / 65070)) < 1e-12


def test_the_float32_yardstick_orders_the_two_origins():
    """Flat 200 with +-1 jitter: float32 on raw levels loses several times more than float32 about 127.5 (why the kernel takes its moments about an
    origin)."""
    rng = np.random.default_rng(2)
    f = np.full((40, 40, 3), 200, np.uint8)
    j = (200 + rng.integers(-1, 2, f.shape)).astype(np.uint8)
    exact = R.ssim_separable(f, j)
    centred, raw = abs(R.ssim_f32(f, j) - exact), abs(R.ssim_f32(f, j, 0.0) - exact)
    print(f'flat jitter: centred {centred:.2e}, raw {raw:.2e}')
    assert centred < 2e-5 and raw > 2 * centred


# ------------------------------------------------------------------------------------------------------------- the op's CPU route

def check_against_ref(res, pairs, ssim_tol):
    for j, (a, b) in enumerate(pairs):
        want = R.metrics(a, b)
        assert int(res['sad'][j]) == want['sad'] and int(res['ssd'][j]) == want['ssd'], j
        assert abs(float(res['ssim'][j]) - want['ssim']) <= ssim_tol, j
        assert float(res['l1'][j]) == pytest.approx(want['l1'], rel=1e-14) and float(res['mse'][j]) == pytest.approx(want['mse'], rel=1e-14)
        assert float(res['psnr'][j]) == pytest.approx(want['psnr'], rel=1e-13) if want['ssd'] else float(res['psnr'][j]) == math.inf


def test_cpu_route_equals_the_restatement():
    from torch_utils.ops import image_metrics as M
    rng = np.random.default_rng(3)
    for c in (1, 3):
        a = noise(rng, (4, 12, 27, c))
        b = np.stack([noise(rng, (12, 27, c)), nudge(rng, a[1], 3), a[2].copy(), nudge(rng, a[3], 20)])
        res = M.pair_metrics(torch.from_numpy(a), torch.from_numpy(b))
        for k in ('sad', 'ssd'):
            assert res[k].dtype == torch.int64 and res[k].shape == (4,)
        for k in ('l1', 'mse', 'psnr', 'ssim'):
            assert res[k].dtype == torch.float64 and res[k].shape == (4,)
        check_against_ref(res, list(zip(a, b)), 1e-12)
        assert float(res['ssim'][2]) == 1.0


def test_cpu_route_on_views_of_one_parent():
    from torch_utils.ops import image_metrics as M
    rng = np.random.default_rng(4)
    parent = torch.from_numpy(noise(rng, (64, 97, 3)))
    wide = torch.from_numpy(noise(rng, (30, 40, 4)))
    jobs = [(parent[2:42, 3:48], parent[5:45, 20:65]), (parent[2:20, 3:30], parent[2:20, 3:30]), (wide[:, :, :3], wide[:, :, 1:]),
            (wide[1:20, 2:30, 3:], wide[3:22, 1:29, :1])]
    res = M.pair_metrics_table(jobs)
    check_against_ref(res, [(a.numpy(), b.numpy()) for a, b in jobs], 1e-12)


def test_cpu_route_refuses_bad_shapes():
    from torch_utils.ops import image_metrics as M
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)
    for a, b in ((z(1, 10, 20, 3), z(1, 10, 20, 3)), (z(1, 20, 10, 3), z(1, 20, 10, 3)), (z(1, 20, 20, 2), z(1, 20, 20, 2)), (z(0, 20, 20, 3), z(0, 20, 20, 3)),
                 (z(1, 20, 20, 3), z(1, 20, 21, 3)), (z(20, 20, 3), z(20, 20, 3))):
        with pytest.raises(ValueError):
            M.pair_metrics(a, b)
    with pytest.raises(ValueError):
        M.pair_metrics(torch.zeros(1, 20, 20, 3), torch.zeros(1, 20, 20, 3))
    with pytest.raises(ValueError):
        M.pair_metrics_table([])


# ------------------------------------------------------------------------------------------------------------- the snapshot grid

@pytest.fixture(scope='module')
def vis_root(tmp_path_factory):
    return write_vis_root(str(tmp_path_factory.mktemp('vis_metrics')))


def grid_reference(fin_grid, g, names):
    """The restatement on a downloaded grid: diagonal cell against left-column cell, columns 96 : 416."""
    per = []
    for i in range(g):
        rows = slice(512 * (i + 1), 512 * (i + 2))
        per.append(R.metrics(fin_grid[rows, 512 * (i + 1) + 96:512 * (i + 1) + 416], fin_grid[rows, 96:416]))
    return {f'Metric/recon_{n}': float(np.mean([p[n] for p in per])) for n in names}, per


def test_grid_reconstruction_on_a_cpu_grid(vis_root):
    from training import metrics as MT
    from training import snapshot_grid as S
    from training import training_loop as T
    from training.dataset import TrainSet
    grid = S.setup_snapshot_grid(TrainSet(vis_root, shuffle=False, device='cpu'), 'cpu')
    torch.manual_seed(0)
    G = T.build_networks(1, 'cpu', WIDTH)[0].eval().requires_grad_(False)
    fin_grid, _ = grid.render(G, 3)
    got = MT.grid_reconstruction(grid, ('l1', 'psnr', 'ssim'))
    want, per = grid_reference(fin_grid, 3, ('l1', 'psnr', 'ssim'))
    assert set(got) == set(want) == {'Metric/recon_l1', 'Metric/recon_psnr', 'Metric/recon_ssim'}
    for k in want:
        assert isinstance(got[k], float) and got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k
    assert all(p['sad'] > 0 for p in per)                                 # an untrained generator does not reproduce the photograph
    assert set(MT.grid_reconstruction(grid, ('ssim',))) == {'Metric/recon_ssim'}
    a, b = MT.grid_pairs(grid)[1]
    assert a.shape == b.shape == (512, 320, 3) and a.data_ptr() - grid.grid_img.data_ptr() == (1024 * 2048 + 1024 + 96) * 3


# ------------------------------------------------------------------------------------------------------------- evaluate_results / calc_metrics.py

def write_triptychs(root, rng):
    """Four files: two self-pairs, one cross pair, one file that is no triptych name.  Returns {name: (person panel, result panel)}."""
    os.makedirs(root, exist_ok=True)
    out = {}
    for name, h, pw in (('p1___p1.png', 24, 20), ('p2___p2.png', 24, 20), ('p1___p2.png', 24, 20), ('notes.png', 24, 20)):
        person = noise(rng, (h, pw, 3))
        trip = np.concatenate([noise(rng, (h, pw, 3)), person, nudge(rng, person, 9)], axis=1)
        PIL.fromarray(trip, 'RGB').save(os.path.join(root, name))
        out[name] = (trip[:, pw:2 * pw], trip[:, 2 * pw:])
    return out


def test_evaluate_results_on_synthetic_triptychs(tmp_path):
    from training import metrics as MT
    panels = write_triptychs(str(tmp_path / 'res'), np.random.default_rng(6))
    per_file = str(tmp_path / 'per.jsonl')
    for pairs, names in (('self', ['p1___p1.png', 'p2___p2.png']), ('all', ['p1___p1.png', 'p1___p2.png', 'p2___p2.png'])):
        got = MT.evaluate_results(str(tmp_path / 'res'), pairs=pairs, device='cpu', batch=2, per_file=per_file)
        want = [R.metrics(*panels[n]) for n in names]
        assert got['count'] == len(names) and got['pairs'] == pairs
        for k in ('l1', 'psnr', 'ssim'):
            assert got[k] == pytest.approx(np.mean([w[k] for w in want]), rel=1e-12), (pairs, k)
        lines = [json.loads(line) for line in open(per_file)]
        assert [line['file'] for line in lines] == names
        for line, w in zip(lines, want):
            assert line['ssim'] == pytest.approx(w['ssim'], abs=1e-12) and line['l1'] == pytest.approx(w['l1'], rel=1e-12)
    assert set(MT.evaluate_results(str(tmp_path / 'res'), names=('psnr',), device='cpu')) == {'psnr', 'count', 'pairs'}


def test_evaluate_results_errors(tmp_path):
    from training import metrics as MT
    rng = np.random.default_rng(7)
    os.makedirs(tmp_path / 'cross')
    PIL.fromarray(noise(rng, (24, 60, 3)), 'RGB').save(str(tmp_path / 'cross' / 'a___b.png'))
    with pytest.raises(ValueError, match='no self-pair triptych'):
        MT.evaluate_results(str(tmp_path / 'cross'), device='cpu')
    assert MT.evaluate_results(str(tmp_path / 'cross'), pairs='all', device='cpu')['count'] == 1
    os.makedirs(tmp_path / 'odd')
    PIL.fromarray(noise(rng, (24, 61, 3)), 'RGB').save(str(tmp_path / 'odd' / 'a___a.png'))
    with pytest.raises(ValueError, match='not divisible by 3'):
        MT.evaluate_results(str(tmp_path / 'odd'), device='cpu')
    with pytest.raises(ValueError, match='detector'):
        MT.evaluate_results(str(tmp_path / 'cross'), names='fid50k_full', pairs='all', device='cpu')


def test_command_line(tmp_path):
    panels = write_triptychs(str(tmp_path / 'res'), np.random.default_rng(8))
    cli = os.path.join(PKG, 'calc_metrics.py')
    per_file = str(tmp_path / 'per.jsonl')
    run = subprocess.run([sys.executable, cli, '--results', str(tmp_path / 'res'), '--device', 'cpu', '--per-file', per_file], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    want = [R.metrics(*panels[n]) for n in ('p1___p1.png', 'p2___p2.png')]
    assert list(out) == ['l1', 'psnr', 'ssim', 'count', 'pairs'] and out['count'] == 2 and out['pairs'] == 'self'
    assert out['ssim'] == pytest.approx(np.mean([w['ssim'] for w in want]), abs=1e-12)
    assert len(open(per_file).readlines()) == 2
    os.makedirs(tmp_path / 'empty')
    run = subprocess.run([sys.executable, cli, '--results', str(tmp_path / 'empty'), '--device', 'cpu'], capture_output=True, text=True)
    assert run.returncode != 0 and 'no self-pair triptych' in run.stderr and not run.stdout.strip()


# ------------------------------------------------------------------------------------------------------------- the training driver

def test_metrics_option_parsing():
    from training import metrics as MT
    from training import training_loop as T
    base = ['--data', 'd', '--outdir', 'o']
    assert T.parse_args(base).metrics == 'none'
    assert MT.parse_metrics('none') is None and MT.parse_metrics(None) is None and MT.parse_metrics('') is None
    assert MT.parse_metrics('ssim, l1') == ('l1', 'ssim') and MT.parse_metrics(('psnr',)) == ('psnr',)
    for bad in ('fid50k_full', 'kid50k_full', 'pr50k3_full', 'ppl2_wend', 'is50k'):
        with pytest.raises(ValueError, match='need a pretrained detector network'):
            MT.parse_metrics(bad)
    with pytest.raises(ValueError, match='unknown metric'):
        MT.parse_metrics('ssim,sharpness')
    with pytest.raises(SystemExit, match='need a pretrained detector network'):          # refused before anything is read or built
        T.main(base + ['--metrics', 'fid50k_full'])


def stats_lines(run):
    return [json.loads(line) for line in open(os.path.join(run, 'stats.jsonl'))]


def test_driver_without_metrics_writes_no_metric_key(vis_root, tmp_path, capsys):
    from training import training_loop as T
    run = str(tmp_path / 'run')
    T.training_loop(run, vis_root, batch=1, batch_gpu=1, kimg=0.001, tick=0.001, snap=None, image_snap=0, workers=0, device='cpu', width=WIDTH, aug='noaug',
                    dataset_kwargs=dict(shuffle=False))
    lines = stats_lines(run)
    assert lines and not [k for line in lines for k in line if k.startswith('Metric/')]
    assert 'Metric/' not in capsys.readouterr().out


def test_driver_with_metrics_writes_finite_values(vis_root, tmp_path, capsys):
    from training import training_loop as T
    run = str(tmp_path / 'run')
    T.training_loop(run, vis_root, batch=1, batch_gpu=1, kimg=0.001, tick=0.001, snap=None, image_snap=1, workers=0, device='cpu', width=WIDTH, aug='noaug',
                    dataset_kwargs=dict(shuffle=False), metrics=('l1', 'psnr', 'ssim'))
    lines = stats_lines(run)
    assert len(lines) == 1
    line = lines[0]
    for k in ('Metric/recon_l1', 'Metric/recon_psnr', 'Metric/recon_ssim'):
        assert k in line and math.isfinite(line[k]), line
    assert -1 <= line['Metric/recon_ssim'] <= 1 and 0 < line['Metric/recon_l1'] <= 1 and line['Metric/recon_psnr'] > 0
    out = capsys.readouterr().out
    assert out.index('Metric/recon_l1') > out.index('tick 0')
    fin = np.array(PIL.open(os.path.join(run, 'fakes000000_finetune.png')))
    want, _ = grid_reference(fin, 3, ('l1', 'psnr', 'ssim'))
    for k in want:
        assert line[k] == pytest.approx(want[k], rel=1e-12), k


def test_driver_with_metrics_but_no_grid_says_so(tmp_path, capsys):
    from training import training_loop as T
    from test_train_loader import write_train_root
    root = write_train_root(str(tmp_path / 'train'))
    run = str(tmp_path / 'run')
    T.training_loop(run, root, batch=1, batch_gpu=1, kimg=0.001, tick=0.001, snap=None, image_snap=1, workers=0, device='cpu', width=WIDTH, aug='noaug',
                    dataset_kwargs=dict(shuffle=False), metrics='ssim')
    out = capsys.readouterr().out
    assert out.count('--metrics is off') == 1
    assert not [k for line in stats_lines(run) for k in line if k.startswith('Metric/')]
