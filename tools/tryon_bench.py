"""Measure the try-on driver (training/tryon.py) end to end on a GPU.

Writes K synthetic pairs in the reference's file formats to a temporary directory (or reads --dataroot), builds a full-width GeneratorFull_v20
(deterministic weights, or --network), and reports as one JSON line:
  - end-to-end images/s of ``run_tryon`` (after one warm-up pass), with the worker count;
  - host ms per sample of the loader's unrouted half (``TryOnTestSet.unrouted``, one process);
  - GPU ms per batch from events around routing, inputs (row extents + pg_tryon_inputs), generator and triptych (--part outfit: the four panels,
    pg_tryon_panels_u8, under the same keys);
  - launches per batch of the three tryon kernels, the device time and achieved GB/s of pg_tryon_inputs and pg_tryon_triptych_u8 alone;
  - an A/B on the same batch against the existing path: the loader's 16-tuple (pinned, float64 skin / label maps) through ``to_generator_inputs`` and
    test.py's host triptych (finetune_img, image and clothes to the host as float32, NumPy), against pg_tryon_inputs + pg_tryon_triptych_u8 + one copy
    of the bytes.  Both sides exclude the generator.

    python tools/tryon_bench.py --batch 16 --pairs 64 --part upper
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

ORDER = ['cnose', 'cneck', 'rshoulder', 'relbow', 'rwrist', 'lshoulder', 'lelbow', 'lwrist', 'rhip', 'rknee', 'rankle', 'lhip', 'lknee', 'lankle',
         'reye', 'leye', 'rear', 'lear']
JOINTS = dict(cnose=(160, 60), cneck=(160, 110), rshoulder=(104, 120), relbow=(84, 200), rwrist=(74, 270), lshoulder=(216, 120), lelbow=(239, 200),
              lwrist=(249, 270), rhip=(124, 290), rknee=(119, 390), rankle=(116, 480), lhip=(196, 290), lknee=(201, 390), lankle=(204, 480),
              reye=(150, 50), leye=(170, 50), rear=(140, 55), lear=(180, 55))


def write_pairs(root, k, seed=0, outfit=False):
    """k synthetic people (noise photo, blocky LIP parsing, garment parsing, jittered OpenPose-18), paired i -> i+1; outfit: lines of three names, the
    upper clothes i+1 and the lower clothes i+2 on person i."""
    import PIL.Image
    rng = np.random.default_rng(seed)
    for d in ('image', 'parsing', 'garment_parsing', 'keypoints'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    names = []
    for i in range(k):
        name, dress = f'p{i:04d}', i % 5 == 4
        PIL.Image.fromarray(rng.integers(30, 226, (512, 320, 3), dtype=np.uint8), 'RGB').save(os.path.join(root, 'image', name + '.jpg'), quality=95)
        lab = np.zeros((512, 320), np.uint8)
        lab[30:90, 130:190], lab[15:30, 130:190], lab[90:112, 145:175] = 13, 2, 10
        lab[112:300, 100:220] = 6 if dress else 5
        lab[112:280, 70:100], lab[112:280, 220:250] = 14, 15
        lab[290:470, 110:210] = 6 if dress else (9 if i % 2 else 12)
        lab[470:500, 105:150], lab[470:500, 170:215] = 18, 19
        PIL.Image.fromarray(lab, 'L').save(os.path.join(root, 'parsing', name + '.png'))
        gp = np.zeros((512, 320, 3), np.uint8)
        gp[112:200, 70:100, 0], gp[112:200, 220:250, 0] = 10, 11
        PIL.Image.fromarray(gp, 'RGB').save(os.path.join(root, 'garment_parsing', name + '.png'))
        kp = []
        for j in ORDER:
            x, y = JOINTS[j]
            kp += [float(x + rng.normal(0, 4)), float(y + rng.normal(0, 4)), 0.9]
        with open(os.path.join(root, 'keypoints', name + '_keypoints.json'), 'w') as f:
            json.dump(dict(version=1.3, people=[dict(pose_keypoints_2d=kp)]), f)
        names.append(name + '.jpg')
    with open(os.path.join(root, 'test_pairs.txt'), 'w') as f:
        for i in range(k):
            f.write(f'{names[(i + 1) % k]} {names[(i + 2) % k]} {names[i]}\n' if outfit else f'{names[(i + 1) % k]} {names[i]}\n')


def _device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--part', default='upper', choices=['upper', 'lower', 'full', 'outfit'])
    ap.add_argument('--workers', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--dataroot')
    ap.add_argument('--network')
    args = ap.parse_args()

    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from training import networks as PN
    from training import tryon
    from training.dataset import TryOnTestSet, collate_unrouted, to_generator_inputs
    from training.synthetic import fill_module_
    dev = torch.device('cuda', 0)

    tmp = None
    root = args.dataroot
    if root is None:
        tmp = tempfile.TemporaryDirectory()
        root = tmp.name
        write_pairs(root, args.pairs, outfit=args.part == 'outfit')
    ds = TryOnTestSet(root, use_sleeve_mask=True, part=args.part)
    if args.network:
        G = tryon.build_generator(args.network, dev)
    else:
        G = fill_module_(PN.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                              synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256)), 'bench.')   # bench.py config 3's
        G = G.eval().requires_grad_(False).to(dev)
    out = dict(part=args.part, batch=args.batch, pairs=len(ds), workers=args.workers)

    # ---- host: the loader's unrouted half, one process
    m = min(len(ds), 8)
    t0 = time.perf_counter()
    items = [ds.unrouted(i) for i in range(m)]
    out['loader_host_ms_per_sample'] = round((time.perf_counter() - t0) * 1e3 / m, 2)

    # ---- end to end (one warm-up pass), with per-stage events
    with tempfile.TemporaryDirectory() as od:
        tryon.run_tryon(ds, G, od, batch_size=args.batch, device=dev, workers=args.workers)
        torch.cuda.synchronize()
        stats = {}
        tryon.launch_counter = dict(row_extent=0, inputs=0, triptych=0, panels=0)
        t0 = time.perf_counter()
        files = tryon.run_tryon(ds, G, od, batch_size=args.batch, device=dev, workers=args.workers, stats=stats)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        counts, tryon.launch_counter = tryon.launch_counter, None
    nb = len(stats['events'])
    full = [e for e, s in zip(stats['events'], range(nb)) if s < len(ds) // args.batch]                 # full batches only
    stage = lambda i, j: float(np.mean([e[i].elapsed_time(e[j]) for e in full]))
    out['images_per_s'] = round(len(files) / wall, 2)
    out['loader_wait_ms_per_batch'] = round(float(np.mean(stats['load_s'])) * 1e3, 2)
    out['gpu_ms_per_batch'] = dict(routing=round(stage(0, 1), 3), inputs=round(stage(1, 2), 3), generator=round(stage(2, 3), 3),
                                   triptych=round(stage(3, 4), 3), total=round(stage(0, 4), 3))
    out['launches_per_batch'] = {k: v / nb for k, v in counts.items()}

    # ---- the kernels alone, and the A/B on one full batch
    n = args.batch
    items = [ds.unrouted(i % len(ds)) for i in range(n)]
    batch = tryon.upload(collate_unrouted(items, pin=True), dev)
    routed, ext = tryon.route(batch, args.part)
    den_up, den_lo, _ = tryon._canvases(batch, routed, args.part)
    inp_ms = _device_ms(lambda: tryon.generator_inputs(batch, routed[0], routed[1], den_up, den_lo, ext, args.part), 50)
    inp = tryon.batch_inputs(batch, routed, ext, args.part)
    moved = sum(t.numel() * t.element_size() for t in inp.values())
    moved += sum(t.numel() for t in (batch['image'], batch['pose'], batch['retain_mask'], den_up, den_lo, routed[0], routed[1]))
    out['inputs_kernel'] = dict(ms=round(inp_ms, 4), MB=round(moved / 1e6, 1), GBps=round(moved / inp_ms / 1e6, 1))
    with torch.no_grad():
        _, fin, _ = G(**inp, noise_mode='const')
    k = 3 if args.part == 'outfit' else 2                                                               # source panels
    tri_ms = _device_ms(lambda: tryon.pack(fin, batch, args.part), 50)
    tmoved = fin.numel() * 4 // 512 * 320 + k * n * 512 * 320 * 3 + n * 512 * (k + 1) * 320 * 3
    out['triptych_kernel'] = dict(ms=round(tri_ms, 4), MB=round(tmoved / 1e6, 1), GBps=round(tmoved / tri_ms / 1e6, 1))

    tup = [t.cpu().contiguous().pin_memory() for t in tryon.loader_tuple(batch, routed, ext, args.part)]        # what test.py's DataLoader hands over

    def old():
        x = to_generator_inputs(tup, dev)
        img = x['retain'][:, :3]                                                                             # (stand-ins of test.py's
        f, im, cl = fin.cpu().numpy(), img.cpu().numpy(), img.cpu().numpy()                                  # three device -> host copies)
        for ii in range(n):
            g = np.clip((f[ii].transpose(1, 2, 0) + 1.0) * 127.5, 0, 255).astype(np.uint8)
            a = ((im[ii].transpose(1, 2, 0) + 1.0) * 127.5).astype(np.uint8)
            b = ((cl[ii].transpose(1, 2, 0) + 1.0) * 127.5).astype(np.uint8)
            np.concatenate([b[:, 96:416], a[:, 96:416], g[:, 96:416]], axis=1)

    host = torch.empty([n, 512, (k + 1) * 320, 3], dtype=torch.uint8, pin_memory=True)

    def new():
        tryon.generator_inputs(batch, routed[0], routed[1], den_up, den_lo, ext, args.part)
        host.copy_(tryon.pack(fin, batch, args.part), non_blocking=True)
        torch.cuda.synchronize()

    def wall_ms(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps
    out['ab_ms_per_batch'] = dict(existing=round(wall_ms(old), 2), native=round(wall_ms(new), 2))
    print(json.dumps(out))
    if tmp is not None:
        tmp.cleanup()


if __name__ == '__main__':
    main()
