"""Measure the training loader's GPU half (training/train_fetch.py) on one GPU, in one run.

Writes K synthetic people in the reference's training layout to a temporary directory (``tools/tryon_bench.py``'s writer, plus the list file and two
random masks), and reports as one JSON line:
  - device ms and achieved GB/s of pg_train_fetch alone (bytes = every source byte read once + every output byte written once);
  - device ms of `fetch_reference` (the same statements in torch) on the same GPU tensors;
  - device ms of ``normalize_batch(part='train')`` and of the row-extent launch;
  - host ms per sample of ``TrainSet.unrouted`` (one process).

    python tools/train_fetch_bench.py --batch 16 --people 16
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def write_train_root(root, k, seed=0):
    import PIL.Image
    from tryon_bench import write_pairs
    sub = os.path.join(root, 'Zalando_512_320_v1')
    write_pairs(sub, k, seed)
    with open(os.path.join(sub, 'test_pairs.txt')) as f, open(os.path.join(sub, 'train_pairs_front_list_220508.txt'), 'w') as g:
        g.writelines(line.split()[1] + '\n' for line in f)
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    for i in range(2):
        m = np.zeros((512, 512), np.uint8)
        m[150 + 100 * i:330 + 100 * i, 180:320] = 255
        PIL.Image.fromarray(m, 'L').save(os.path.join(root, 'train_random_mask_acgpn', f'mask_{i}.png'))


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--people', type=int, default=16)
    p.add_argument('--reps', type=int, default=20)
    args = p.parse_args(argv)
    from training import dataset as ds_mod
    from training import train_fetch as F
    with tempfile.TemporaryDirectory() as root:
        write_train_root(root, args.people)
        ds = ds_mod.TrainSet(root, shuffle=False)
        t0 = time.perf_counter()
        items = [ds.unrouted(i % len(ds)) for i in range(args.batch)]
        host_ms = 1e3 * (time.perf_counter() - t0) / args.batch
    batch = F.upload(ds_mod.collate_train(items, pin=True), 'cuda')
    routed, ext = F.route(batch)
    n, H, W, h, w = args.batch, 512, 512, 128, 128
    moved = n * (H * W * (3 + 3 + 1 + 1 + 1 + 3 + 3) + h * w * 45 + H) + 4 * n * (H * W * (3 + 6 + 5 + 3 + 3 + 1 + 1 + 1) + h * w * 45)
    fetch_ms = device_ms(lambda: F.fetch(batch, routed, ext), args.reps)
    result = dict(tool='train_fetch_bench', device=torch.cuda.get_device_name(0), batch=n,
                  pg_train_fetch_ms=round(fetch_ms, 4), pg_train_fetch_bytes=moved, pg_train_fetch_gbps=round(moved / fetch_ms / 1e6, 1),
                  fetch_reference_torch_ms=round(device_ms(lambda: F.fetch_reference(batch, routed, ext), max(2, args.reps // 4)), 4),
                  normalize_batch_train_ms=round(device_ms(lambda: F.patch_routing.normalize_batch(
                      [(batch['upper_img'][i], batch['lower_img'][i], batch['upper_mask'][i], batch['lower_mask'][i], batch['sleeve'][i], batch['person_kp'][i],
                        batch['person_kp'][i]) for i in range(n)], 2, part='train'), max(2, args.reps // 4)), 4),
                  row_extent_ms=round(device_ms(lambda: F.lower_mask_extents(routed), args.reps), 4),
                  host_unrouted_ms_per_sample=round(host_ms, 2))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
