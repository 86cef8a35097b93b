"""Dev tool (GPU box): throughput of training.patch_routing on synthetic 512x512 samples, inputs resident on the GPU -- `normalize_batch` (a batch
of 16, the route config3_routed takes) and the per-sample `normalize`, for the mode given by --part (upper | lower | full | outfit | train | all; outfit
routes the lower garment through a second set of key points).
Reports per batch the device time of the routing with the host work hidden (bench.py's config3_routed figure), the host wall time, the native
launches and the algorithmic bytes."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
from torch_utils import custom_ops
custom_ops.verbosity = 'none'
from training import patch_routing as P
from test_patch_routing import keypoints

ap = argparse.ArgumentParser()
ap.add_argument('--part', default='upper', choices=sorted(P.MODES) + ['all'])
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--reps', type=int, default=20)
args = ap.parse_args()

rng = np.random.default_rng(0)
up, lo = (torch.from_numpy(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)).cuda() for _ in range(2))
um = torch.zeros(512, 512, 3, dtype=torch.uint8, device='cuda'); um[90:310, 150:370] = 255
lm = torch.zeros(512, 512, 3, dtype=torch.uint8, device='cuda'); lm[270:505, 190:330] = 255
samples = [(up * (um > 0), lo * (lm > 0), um, lm, None, keypoints(rng, 8.0), keypoints(rng, 8.0)) for _ in range(args.batch)]
samples8 = [s + (keypoints(rng, 8.0),) for s in samples]            # outfit: the lower clothes' key points as the eighth entry

c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
c0.record(); torch.cuda._sleep(10 ** 7); c1.record(); torch.cuda.synchronize()
spin_per_ms = 1e7 / max(c0.elapsed_time(c1), 1e-3)                 # the spin kernel's clock (shader or constant-rate counter)

for part in (sorted(P.MODES) if args.part == 'all' else [args.part]):
    samples = samples8 if part == 'outfit' else [s[:7] for s in samples8]
    if part == 'train':                                            # the training mode applies a sleeve mask unconditionally: an empty one
        samples = [s[:4] + (torch.zeros(512, 512, 1, dtype=torch.uint8, device='cuda'),) + s[5:] for s in samples]
    for _ in range(3):
        P.normalize_batch(samples, 2, part=part)
    torch.cuda.synchronize()
    # host wall time of a batch: geometry, job tables and bookkeeping included (the GPU idles behind the host here)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        P.normalize_batch(samples, 2, part=part)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) / args.reps * 1e3
    # GPU time of a batch as config3_routed sees it: the host enqueues the batch while the GPU is still busy (here: a spin kernel standing in for the
    # previous generator pass), so the events bracket the device work of the routing only
    P.traffic_counter = dict(bytes=0, launches=0)
    gpu_ms = []
    for _ in range(args.reps):
        torch.cuda._sleep(int(2 * wall_ms * spin_per_ms))      # twice the host time: the queue is never drained before e0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        P.normalize_batch(samples, 2, part=part)
        e1.record()
        torch.cuda.synchronize()
        gpu_ms.append(e0.elapsed_time(e1))
    batch_ms = float(np.median(gpu_ms))
    launches, nbytes = P.traffic_counter['launches'] // args.reps, P.traffic_counter['bytes'] // args.reps
    P.traffic_counter = None
    t0 = time.perf_counter()
    for s in samples:
        P.normalize(*s[:7], 2, part=part, lower_keypoints=s[7] if len(s) > 7 else None)
    torch.cuda.synchronize()
    sample_ms = (time.perf_counter() - t0) / len(samples) * 1e3
    print(json.dumps(dict(part=part, batch=args.batch, gpu_ms_per_batch=round(batch_ms, 3), host_wall_ms_per_batch=round(wall_ms, 2), launches_per_batch=launches, algorithmic_mb_per_batch=round(nbytes / 1e6, 1),
                          per_sample_normalize_ms=round(sample_ms, 3))), flush=True)
