#!/usr/bin/env python3
"""Time AugmentPipe's late stages (imgfilter, noise, cutout) on the GPU, N = 4, 3 x 512^2, with device events after warm-up, in one run:

* ``apply_late`` on the native route (one ``pg_augment_late`` launch) against the same stages as the torch composition
  (``augment_ops.late_reference``: reflect-pad copy, two grouped 43-tap depthwise convolutions, the noise multiply-add, the mask
  launches) on the same device tensors, for `filter`, `noise`, `cutout` and all three, forward and forward + backward, the two arms
  alternating; the outputs of the two arms are compared first;
* the native forward's bytes per second (the image read once and written once, plus the noise image where it is read);
* a whole ``bgcfnc`` pipe against a ``bgc`` pipe, forward and forward + backward.

The native route must not be slower than the composition of the same stages in this run, for any of the four: the script exits with
status 1 where it is.

Usage:  python tools/augment_late_bench.py [--reps 50] [--rounds 3]   (prints one JSON line)
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pasta-gan-plusplus_amd')]

import torch  # noqa: E402

SHAPE = [4, 3, 512, 512]
STAGES = {'filter': dict(imgfilter=1), 'noise': dict(noise=1), 'cutout': dict(cutout=1), 'all': dict(imgfilter=1, noise=1, cutout=1)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(arms, reps, rounds):
    """Best of `rounds` windows of `reps` calls per arm, the arms alternating; every arm is warmed up first."""
    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn, reps))
    return {k: min(v) for k, v in times.items()}, {k: [round(t, 4) for t in v] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('augment_late_bench.py measures on a GPU; none found')
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import augment_ops
    from training.augment import AugmentPipe, AUGPIPE_SPECS
    dev = torch.device('cuda')
    torch.manual_seed(0)
    x = torch.rand(SHAPE, device=dev) * 2 - 1
    dy = torch.randn_like(x)
    n, c, h, w = SHAPE
    out = dict(workload='AugmentPipe late stages, p = 1, N = 4, 3 x 512^2, device events after warm-up; best of alternating windows (ms)',
               reps=args.reps, rounds=args.rounds, stages={})
    slower = []
    for name, kw in STAGES.items():
        pipe = AugmentPipe(**kw).requires_grad_(False).to(dev)
        late = pipe.sample_late(n, c, h, w, dev)
        native = lambda t: augment_ops.late(t, *late)
        torch_ = lambda t: augment_ops.late_reference(t, *late)
        try:
            err = float((native(x) - torch_(x)).abs().max())
        except RuntimeError as e:           # the composition itself failed on this device (its grouped convolution): say so, time the native route alone
            best, every = alternate({'native': lambda: native(x)}, args.reps, args.rounds)
            out['stages'][name] = dict(torch_composition_error=str(e).splitlines()[0][:200], native_forward_ms=every['native'])
            continue

        def fwd(f):
            def run():
                with torch.no_grad():
                    f(x)
            return run

        def fwd_bwd(f):
            def run():
                xi = x.detach().requires_grad_(True)
                torch.autograd.grad(f(xi), xi, dy)
            return run
        best_f, all_f = alternate({'native': fwd(native), 'torch': fwd(torch_)}, args.reps, args.rounds)
        best_b, all_b = alternate({'native': fwd_bwd(native), 'torch': fwd_bwd(torch_)}, args.reps, args.rounds)
        bytes_moved = x.numel() * 4 * (3 if late[1] is not None else 2)
        out['stages'][name] = dict(max_abs_native_minus_torch=err,
                                   forward_ms=all_f, forward_backward_ms=all_b,
                                   forward_torch_over_native=round(best_f['torch'] / best_f['native'], 3),
                                   forward_backward_torch_over_native=round(best_b['torch'] / best_b['native'], 3),
                                   native_forward_GBps=round(bytes_moved / (best_f['native'] * 1e-3) / 1e9, 1))
        if best_f['native'] > best_f['torch'] or best_b['native'] > best_b['torch']:
            slower.append(name)

    pipes = {k: AugmentPipe(**AUGPIPE_SPECS[k]).requires_grad_(False).to(dev).set_native_late(True) for k in ('bgc', 'bgcfnc')}

    def pipe_fwd(p):
        def run():
            with torch.no_grad():
                p(x)
        return run

    def pipe_fwd_bwd(p):
        def run():
            xi = x.detach().requires_grad_(True)
            torch.autograd.grad(p(xi), xi, dy)
        return run
    best_f, all_f = alternate({k: pipe_fwd(p) for k, p in pipes.items()}, args.reps, args.rounds)
    best_b, all_b = alternate({k: pipe_fwd_bwd(p) for k, p in pipes.items()}, args.reps, args.rounds)
    out['pipe'] = dict(forward_ms=all_f, forward_backward_ms=all_b, forward_bgcfnc_over_bgc=round(best_f['bgcfnc'] / best_f['bgc'], 3),
                       forward_backward_bgcfnc_over_bgc=round(best_b['bgcfnc'] / best_b['bgc'], 3))
    out['native_slower_than_torch'] = slower
    print(json.dumps(out), flush=True)
    if slower:
        sys.exit(1)


if __name__ == '__main__':
    main()
