"""`bench.py --dump-outputs DIR` (CPU only): the last timed step's outputs as DIR/<name>.npy in float32 / float64, at most
DUMP_BYTES_MAX bytes of files, larger outputs as a fixed sample that is the same from run to run; `--steps` below 1 is refused."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    import bench
    bench.torch = torch             # bench.py imports torch in main(), after its launcher branch
    return bench


def test_small_outputs_are_written_whole(tmp_path):
    bench = _bench()
    x = torch.randn(2, 3, 4, 5, generator=torch.Generator().manual_seed(0))
    info = bench.dump_outputs(dict(img=x, d=x.double(), h=x.to(torch.bfloat16), none=None), str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['d.npy', 'h.npy', 'img.npy']
    assert np.array_equal(np.load(tmp_path / 'img.npy'), x.numpy())
    assert np.load(tmp_path / 'd.npy').dtype == np.float64 and np.load(tmp_path / 'h.npy').dtype == np.float32
    assert not any(v['sampled'] for v in info.values()) and info['img']['shape'] == [2, 3, 4, 5]


def test_headline_sized_outputs_are_sampled_within_the_budget_and_reproducibly(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(1)
    outs = dict(img=torch.randn(8, 3, 512, 512, generator=g), finetune_img=torch.randn(8, 3, 512, 512, generator=g),
                pred_parsing=torch.randn(8, 7, 512, 512, generator=g))
    info = bench.dump_outputs(outs, str(tmp_path / 'a'))
    bench.dump_outputs(outs, str(tmp_path / 'b'))
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= bench.DUMP_BYTES_MAX
    for name, t in outs.items():
        a = np.load(tmp_path / 'a' / f'{name}.npy')
        assert info[name]['sampled'] and info[name]['elements_written'] == a.size
        assert np.array_equal(a, np.load(tmp_path / 'b' / f'{name}.npy'))
        idx = np.sort(np.random.RandomState(0).permutation(t.numel())[:a.size])
        assert np.array_equal(a, t.numpy().reshape(-1)[idx])


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and '--steps' in r.stderr
