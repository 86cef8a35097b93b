"""Measure the reconstruction metrics (torch_utils/ops/image_metrics.py, csrc/image_metrics.hip) on a GPU.

Two workloads on random uint8 images: the 16 panel pairs of a calc_metrics.py batch (512 x 320 x 3 each: middle against right panel of 512 x 960
triptychs) and the 14 diagonal-against-left-column pairs of a full snapshot grid (windows of one 7680 x 7680 x 3 image).  Reports as one JSON line, per
workload:
  - `native_ms`: device time of one pg_image_pair_metrics_u8 call (both launches) on a table that is already on the device (events over --reps calls);
  - `op_ms`: wall time of one `pair_metrics_table` call, host work included (table, pinned upload, the few torch ops behind it), without a host read;
  - `torch_ms`: device time of the same figures through a torch composition: float32 copies, `conv2d` with the separable window on the five moment maps;
  - `mb`: the bytes of the two windows of every pair (what has to be read at least), and `native_gbs` / `torch_gbs` = mb / time;
  - `ssim_dev`: the largest |native - torch composition| SSIM of a pair (the composition is float32 on raw levels: a plausibility check only);
and `tick_ms`: what ``--metrics l1,psnr,ssim`` adds to an image-snapshot tick: wall time of `training.metrics.grid_reconstruction` on the rendered grid,
its one host read included.

    python tools/image_metrics_bench.py --reps 20
"""

import argparse
import ctypes
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))


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


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def native_call(jobs):
    """A closure that enqueues pg_image_pair_metrics_u8 on a table uploaded once; returns (sad, ssd, ssim)."""
    from torch_utils.ops import image_metrics as M
    from training.patch_routing import _upload_table
    lib = M._init().lib
    dev = jobs[0][0].device
    n = len(jobs)
    t = np.zeros(n, dtype=M._PAIR_DT)
    t['a'], t['b'] = [a.data_ptr() for a, _ in jobs], [b.data_ptr() for _, b in jobs]
    t['a_row_stride'], t['b_row_stride'] = [a.stride(0) for a, _ in jobs], [b.stride(0) for _, b in jobs]
    t['a_pix_stride'], t['b_pix_stride'] = [a.stride(1) for a, _ in jobs], [b.stride(1) for _, b in jobs]
    t['h'], t['w'], t['channels'] = [a.shape[0] for a, _ in jobs], [a.shape[1] for a, _ in jobs], [a.shape[2] for a, _ in jobs]
    host = t.ctypes.data_as(ctypes.c_void_p)
    tab = _upload_table(t, dev)
    work = torch.empty([int(lib.pg_image_pair_metrics_workspace(host, n)) // 8], dtype=torch.int64, device=dev)
    sums = torch.empty([2, n], dtype=torch.int64, device=dev)
    ssim = torch.empty([n], dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        st = lib.pg_image_pair_metrics_u8(host, tab.data_ptr(), n, work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), ssim.data_ptr(), stream)
        assert st == 0, st
        return sums[0], sums[1], ssim
    call.keep = (t, tab)
    return call


def torch_composition(jobs):
    """The same figures with torch ops on the GPU: float32, raw levels, conv2d with the separable window."""
    from torch_utils.ops import image_metrics as M
    g = M.gaussian_taps().to(jobs[0][0].device, torch.float32)
    gx, gy = g.reshape(1, 1, 1, -1), g.reshape(1, 1, -1, 1)
    a = torch.stack([p[0] for p in jobs]).permute(0, 3, 1, 2).to(torch.float32)
    b = torch.stack([p[1] for p in jobs]).permute(0, 3, 1, 2).to(torch.float32)
    n, c, h, w = a.shape
    d = a - b
    sad, ssd = d.abs().sum(dim=(1, 2, 3), dtype=torch.float64), (d * d).sum(dim=(1, 2, 3), dtype=torch.float64)
    maps = torch.cat([a, b, a * a, b * b, a * b]).reshape(5 * n * c, 1, h, w)
    f = torch.nn.functional.conv2d(torch.nn.functional.conv2d(maps, gx), gy).reshape(5, n, c, h - 10, w - 10)
    ma, mb = f[0], f[1]
    va, vb, cab = f[2] - ma * ma, f[3] - mb * mb, f[4] - ma * mb
    ssim = (((2 * ma * mb + M.C1) * (2 * cab + M.C2)) / ((ma * ma + mb * mb + M.C1) * (va + vb + M.C2))).mean(dim=(1, 2, 3), dtype=torch.float64)
    return sad, ssd, ssim


def measure(jobs, reps):
    from torch_utils.ops import image_metrics as M
    call = native_call(jobs)
    native_ms, native = device_ms(call, reps)
    op_ms, _ = wall_ms(lambda: M.pair_metrics_table(jobs), reps)
    torch_ms, comp = device_ms(lambda: torch_composition(jobs), max(1, reps // 4))
    mb = sum(2 * a.shape[0] * a.shape[1] * a.shape[2] for a, _ in jobs) / 1e6
    assert torch.equal(native[0].double(), comp[0]) and torch.equal(native[1].double(), comp[1])
    return dict(pairs=len(jobs), mb=round(mb, 2), native_ms=round(native_ms, 4), op_ms=round(op_ms, 4), torch_ms=round(torch_ms, 4),
                native_gbs=round(mb / native_ms, 1), torch_gbs=round(mb / torch_ms, 1),
                ssim_dev=float((native[2].double() - comp[2]).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--gnum', type=int, default=14)
    a = ap.parse_args()
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from training import metrics as MT
    dev = torch.device('cuda')
    torch.manual_seed(0)
    res = {}
    trip = torch.randint(0, 256, (16, 512, 960, 3), dtype=torch.uint8, device=dev)
    near = (trip[:, :, 320:640].to(torch.int16) + torch.randint(-9, 10, (16, 512, 320, 3), device=dev, dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
    trip[:, :, 640:] = near
    res['panels'] = measure([(trip[j][:, 320:640], trip[j][:, 640:]) for j in range(16)], a.reps)
    g = a.gnum
    grid = types.SimpleNamespace(gnum=g, H=512, W=512, grid_img=torch.randint(0, 256, ((g + 1) * 512, (g + 1) * 512, 3), dtype=torch.uint8, device=dev))
    res['grid'] = measure(MT.grid_pairs(grid), a.reps)
    MT.grid_reconstruction(grid)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        MT.grid_reconstruction(grid)                          # (ends in its host read)
    res['tick_ms'] = round((time.perf_counter() - t0) * 1e3 / a.reps, 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
