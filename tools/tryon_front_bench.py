"""Measure the two fronts of the try-on driver against each other, in one run on one GPU: the loader's host code (``TryOnTestSet.unrouted`` in the
DataLoader's workers) and the native front (``TryOnTestSet.raw`` in the workers, ``training.tryon_front.front_batch`` on the device).

Writes K synthetic pairs (tools/tryon_bench.py's), builds the full-width generator of tools/tryon_bench.py, and reports as one JSON line:
  - host seconds per sample of ``unrouted`` and of ``raw`` in one process, and the pinned bytes per pair each hands over;
  - device ms, bytes moved (from the shapes) and GB/s of each of the three front launches alone, and of ``front_batch`` as a whole;
  - end-to-end images/s and the per-batch loader wait of ``run_tryon`` for both fronts, alternating them (after a warm-up pass of each).

    python tools/tryon_front_bench.py --batch 16 --pairs 64 --workers 8 --part upper
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

from tryon_bench import _device_ms, write_pairs  # noqa: E402


def _pinned_bytes(batch, n):
    return sum(t.numel() * t.element_size() for t in batch.values() if isinstance(t, torch.Tensor)) // n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--part', default='upper', choices=['upper', 'lower', 'full', 'outfit'])
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=2, help='timed end-to-end passes per front (alternating)')
    ap.add_argument('--small', action='store_true', help='a narrow generator (a rehearsal of the tool, not a measurement)')
    ap.add_argument('--dataroot')
    args = ap.parse_args()

    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from training import networks as PN
    from training import tryon, tryon_front
    from training.dataset import TryOnTestSet, collate_raw, collate_unrouted
    from training.synthetic import fill_module_
    dev = torch.device('cuda', 0)

    tmp = None
    root = args.dataroot
    if root is None:
        tmp = tempfile.TemporaryDirectory()
        root = tmp.name
        write_pairs(root, args.pairs, outfit=args.part == 'outfit')
    ds = TryOnTestSet(root, use_sleeve_mask=True, part=args.part)
    base, w_dim = (4096, 64) if args.small else (32768, 512)
    G = fill_module_(PN.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=w_dim, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                          synthesis_kwargs=dict(channel_base=base, channel_max=512, conv_clamp=256)), 'bench.')
    G = G.eval().requires_grad_(False).to(dev)
    out = dict(part=args.part, batch=args.batch, pairs=len(ds), workers=args.workers)

    # ---- host: seconds per sample in one process, bytes handed over per pair
    m = min(len(ds), 8)
    host = {}
    for name, fn, collate in (('unrouted', ds.unrouted, collate_unrouted), ('raw', ds.raw, collate_raw)):
        t0 = time.perf_counter()
        items = [fn(i) for i in range(m)]
        host[name] = dict(s_per_sample=round((time.perf_counter() - t0) / m, 5), pinned_bytes_per_pair=_pinned_bytes(collate(items), m))
    out['host'] = host

    # ---- the launches alone, on one full batch
    n = args.batch
    raw = tryon.upload(collate_raw([ds.raw(i % len(ds)) for i in range(n)], pin=True), dev)
    plan = tryon_front.plan_batch(raw, args.part)
    moved = tryon_front.launch_bytes(n, 512, raw['person_img'].shape[2], args.part, True)
    for name in tryon_front.LAUNCHES:                        # (in order once: bit_rows and compose read what the launch before them wrote)
        tryon_front.launch(plan, name)
    kern = {}
    for name in tryon_front.LAUNCHES:
        ms = _device_ms(lambda: tryon_front.launch(plan, name), 50)
        kern[name] = dict(ms=round(ms, 4), MB=round(moved[name] / 1e6, 2), GBps=round(moved[name] / ms / 1e6, 1))
    kern['front_batch'] = dict(ms=round(_device_ms(lambda: tryon_front.front_batch(raw, args.part), 50), 4))
    out['front_launches'] = kern

    # ---- end to end: both fronts, alternating, after a warm-up pass of each
    e2e = {f: dict(images_per_s=[], loader_wait_ms_per_batch=[], upload_and_front_ms_per_batch=[]) for f in tryon.FRONTS}
    with tempfile.TemporaryDirectory() as od:
        for f in tryon.FRONTS:
            tryon.run_tryon(ds, G, od, batch_size=args.batch, device=dev, workers=args.workers, front=f)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for f in tryon.FRONTS:
                stats = {}
                t0 = time.perf_counter()
                files = tryon.run_tryon(ds, G, od, batch_size=args.batch, device=dev, workers=args.workers, stats=stats, front=f)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                e2e[f]['images_per_s'].append(round(len(files) / wall, 2))
                e2e[f]['loader_wait_ms_per_batch'].append(round(float(np.mean(stats['load_s'])) * 1e3, 2))
                if f == 'native':
                    e2e[f]['upload_and_front_ms_per_batch'].append(round(float(np.mean([e[0].elapsed_time(e[1]) for e in stats['events']])), 3))
                e2e[f]['gpu_ms_per_batch'] = round(float(np.mean([e[0].elapsed_time(e[-1]) for e in stats['events']])), 3)
    out['end_to_end'] = e2e
    print(json.dumps(out))
    if tmp is not None:
        tmp.cleanup()


if __name__ == '__main__':
    main()
