"""Measure the training driver's image snapshots (training/snapshot_grid.py) on a GPU.

Writes --persons synthetic people (tools/tryon_bench.py's) as a training directory with a visualisation list, and reports as one JSON line:
  - `setup_snapshot_grid` wall time (host work included: loading, key-point geometry, job tables) and the canvases / jobs it made;
  - the device time of the ONE fused pg_patch_denorm_u8 launch over all of them;
  - the same canvases through the unfused route (pg_warp_perspective_u8 of every patch and mask, pg_patch_compose_ordered_u8_k), chunked so that the
    warped intermediates stay below --unfused-mb, with a byte-for-byte comparison;
  - `render` split into input staging, generator and cell packing (events), plus the copy of the two grids to the host;
  - the PNG encode time of one grid.

    python tools/snapshot_grid_bench.py --persons 14 --batch-gpu 4
"""

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def write_root(root, k):
    import PIL.Image
    from tryon_bench import write_pairs
    sub = os.path.join(root, 'Zalando_512_320_v1')
    write_pairs(sub, k)
    names = sorted(os.listdir(os.path.join(sub, 'image')))
    with open(os.path.join(sub, 'train_pairs_front_list_220508.txt'), 'w') as f:
        f.write(''.join(f'{n} {n}\n' for n in names))
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    PIL.Image.fromarray(np.zeros((512, 512), np.uint8), 'L').save(os.path.join(root, 'train_random_mask_acgpn', 'mask_0.png'))
    os.makedirs(os.path.join(root, 'train_img_front_vis_512_220414'))
    for n in names:
        open(os.path.join(root, 'train_img_front_vis_512_220414', n), 'w').close()


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def unfused(jobs, H, W, ksize, chunk):
    from torch_utils.ops import _native as nat
    from training import patch_routing as P
    dev = torch.device('cuda')
    out = torch.empty([len(jobs), H, W, 3], dtype=torch.uint8, device=dev)
    for lo in range(0, len(jobs), chunk):
        part = jobs[lo:lo + chunk]
        warped = P.warp_perspective_batch([(t, m, (W, H)) for parts in part for patch, mask, m in parts for t in (patch, mask)])
        ct = np.zeros(len(part), dtype=P._COMPOSE_DT)
        k = 0
        for j, parts in enumerate(part):
            ct[j]['canvas'], ct[j]['nparts'] = out.data_ptr() + (lo + j) * H * W * 3, len(parts)
            for q in range(len(parts)):
                ct[j]['patch'][q], ct[j]['mask'][q] = warped[k].data_ptr(), warped[k + 1].data_ptr()
                k += 2
        tab = P._upload_table(ct, dev)
        nat.check(P._init().lib.pg_patch_compose_ordered_u8_k(tab.data_ptr(), len(part), H, W, 3, ksize, nat.stream_of(out)), 'pg_patch_compose_ordered_u8_k')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--persons', type=int, default=14)
    ap.add_argument('--batch-gpu', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--unfused-mb', type=int, default=2048)
    ap.add_argument('--channel-base', type=int, default=32768, help='generator width (32768: the full model)')
    a = ap.parse_args()
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from training import snapshot_grid as S
    from training import training_loop as T
    from training.dataset import TrainSet
    res = dict(persons=a.persons, batch_gpu=a.batch_gpu)
    with tempfile.TemporaryDirectory() as root:
        write_root(root, a.persons)
        ds = TrainSet(root, shuffle=False)
        captured = {}
        orig = S.denorm_canvases

        def capture(jobs, H, W, ksize=S.KSIZE, taps=None):
            captured.update(jobs=jobs, H=H, W=W, ksize=ksize)
            return orig(jobs, H, W, ksize, taps)
        S.denorm_canvases = capture
        S.setup_snapshot_grid(ds, 'cuda')                     # warm-up: plugin loading
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid = S.setup_snapshot_grid(ds, 'cuda')
        torch.cuda.synchronize()
        res['setup_s'] = round(time.perf_counter() - t0, 3)
        S.denorm_canvases = orig
    jobs, H, W, ks = captured['jobs'], captured['H'], captured['W'], captured['ksize']
    nparts = sum(len(p) for p in jobs)
    res.update(gnum=grid.gnum, canvases=len(jobs), parts=nparts)
    res['fused_ms'], fused = device_ms(lambda: orig(jobs, H, W, ks), a.reps)
    chunk = max(1, a.unfused_mb * 2 ** 20 // (20 * H * W * 3))
    res['unfused_ms'], plain = device_ms(lambda: unfused(jobs, H, W, ks, chunk), a.reps)
    res.update(unfused_chunk=chunk, unfused_intermediate_mb=round(nparts * 2 * H * W * 3 / 2 ** 20, 1), fused_equals_unfused=bool(torch.equal(fused, plain)))
    res['fused_ms'], res['unfused_ms'] = round(res['fused_ms'], 3), round(res['unfused_ms'], 3)

    torch.manual_seed(0)
    G = T.build_networks(a.batch_gpu, 'cuda', dict(channel_base=a.channel_base, channel_max=512))[0].eval().requires_grad_(False)
    marks = []

    def timer(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))
    grid.render(G, a.batch_gpu)                               # warm-up
    marks.clear()
    start = torch.cuda.Event(enable_timing=True)
    start.record()
    t0 = time.perf_counter()
    grids = grid.render(G, a.batch_gpu, timer=timer)
    res['render_s'] = round(time.perf_counter() - t0, 3)
    split, prev = dict(inputs=0.0, generator=0.0, cells=0.0), start
    for name, e in marks:
        split[name] += prev.elapsed_time(e)
        prev = e
    res.update({f'render_{k}_ms': round(v, 2) for k, v in split.items()})
    with tempfile.TemporaryDirectory() as out:
        t0 = time.perf_counter()
        S.save_png(os.path.join(out, 'grid.png'), grids[0])
        res['png_encode_s'] = round(time.perf_counter() - t0, 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
