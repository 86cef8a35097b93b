"""Measure the per-region reconstruction metrics and the label confusion count (torch_utils/ops/region_metrics.py, csrc/region_metrics.hip) on a GPU.

One workload: the 16 panel pairs of a calc_metrics.py batch (512 x 320 x 3 each: middle against right panel of 512 x 960 triptychs, random uint8) with
blocky random 7-class label maps and the three default regions (upper, lower, skin).  Reports one JSON line:
  - `region_ms`: device time of one pg_region_pair_metrics_u8 call (both launches) on a table that is already on the device (events over --reps calls);
  - `region_op_ms`: wall time of one `region_metrics_table` call, host work included, without a host read;
  - `torch_ms`: (a) device time of the same figures through a torch composition: float32 `conv2d` maps on raw levels, then masked sums per region;
  - `pair_ms`: (b) device time of pg_image_pair_metrics_u8 on the same pairs -- `region_over_pair` = region_ms / pair_ms is what the label read and
    the R accumulators cost over the unmasked pass;
  - `confusion_ms`: (c) device time of one pg_label_confusion_u8 call on 16 (grey RGB cell, label map) windows of 512 x 320, K = 7, against
    `bincount_ms`: `torch.bincount(target * K + pred)` per window on index maps that are already int64 (the look-ups not counted);
  - `ssim_dev`: the largest |native - torch composition| region SSIM (the composition is float32 on raw levels: a plausibility check only).

    python tools/region_metrics_bench.py --reps 20
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from image_metrics_bench import device_ms, native_call, wall_ms  # noqa: E402


def region_call(jobs, bits):
    """A closure that enqueues pg_region_pair_metrics_u8 on a table uploaded once; returns (counts [4, J, R], ssim_sum [J, R])."""
    from torch_utils.ops import region_metrics as M
    from training.patch_routing import _upload_table
    lib = M._init().lib
    dev = jobs[0][0].device
    n, R = len(jobs), len(bits)
    t = np.zeros(n, dtype=M._RPAIR_DT)
    for k, i in (('a', 0), ('b', 1), ('labels', 2)):
        t[k] = [job[i].data_ptr() for job in jobs]
    for k, i in (('a', 0), ('b', 1), ('l', 2)):
        t[k + '_row_stride'], t[k + '_pix_stride'] = [job[i].stride(0) for job in jobs], [job[i].stride(1) for job in jobs]
    t['h'], t['w'], t['channels'] = [j[0].shape[0] for j in jobs], [j[0].shape[1] for j in jobs], [j[0].shape[2] for j in jobs]
    host = t.ctypes.data_as(ctypes.c_void_p)
    tab = _upload_table(t, dev)
    work = torch.empty([int(lib.pg_region_pair_metrics_workspace(host, n, R)) // 8], dtype=torch.int64, device=dev)
    counts = torch.empty([4, n, R], dtype=torch.int64, device=dev)
    ssim_sum = torch.empty([n, R], dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        st = lib.pg_region_pair_metrics_u8(host, tab.data_ptr(), n, bits.ctypes.data_as(ctypes.c_void_p), R, work.data_ptr(), counts.data_ptr(),
                                           ssim_sum.data_ptr(), stream)
        assert st == 0, st
        return counts, ssim_sum
    call.keep = (t, tab, bits)
    return call


def confusion_call(pairs, pred_lut, target_lut, K):
    from torch_utils.ops import region_metrics as M
    from training.patch_routing import _upload_table
    lib = M._init().lib
    dev = pairs[0][0].device
    n = len(pairs)
    t = np.zeros(n, dtype=M._LPAIR_DT)
    t['pred'], t['target'] = [p.data_ptr() for p, _ in pairs], [q.data_ptr() for _, q in pairs]
    t['p_row_stride'], t['t_row_stride'] = [p.stride(0) for p, _ in pairs], [q.stride(0) for _, q in pairs]
    t['p_pix_stride'], t['t_pix_stride'] = [p.stride(1) for p, _ in pairs], [q.stride(1) for _, q in pairs]
    t['h'], t['w'] = [p.shape[0] for p, _ in pairs], [p.shape[1] for p, _ in pairs]
    host = t.ctypes.data_as(ctypes.c_void_p)
    tab = _upload_table(t, dev)
    out = torch.zeros([n, K, K], dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        out.zero_()                                               # (the kernel adds: the fill is part of a call, as in the op)
        st = lib.pg_label_confusion_u8(host, tab.data_ptr(), n, pred_lut.ctypes.data_as(ctypes.c_void_p), target_lut.ctypes.data_as(ctypes.c_void_p), K,
                                       out.data_ptr(), stream)
        assert st == 0, st
        return out
    call.keep = (t, tab, pred_lut, target_lut)
    return call


def torch_composition(jobs, regions):
    """The region figures with torch ops on the GPU: float32, raw levels, conv2d with the separable window, masked sums -> (counts [4, J, R], ssim)."""
    from torch_utils.ops import image_metrics as IM
    dev = jobs[0][0].device
    g = IM.gaussian_taps().to(dev, torch.float32)
    gx, gy = g.reshape(1, 1, 1, -1), g.reshape(1, 1, -1, 1)
    a = torch.stack([p[0] for p in jobs]).permute(0, 3, 1, 2).to(torch.float32)
    b = torch.stack([p[1] for p in jobs]).permute(0, 3, 1, 2).to(torch.float32)
    lab = torch.stack([p[2] for p in jobs]).to(torch.int64)
    n, c, h, w = a.shape
    member = torch.zeros([len(regions), 256], dtype=torch.bool, device=dev)
    for r, values in enumerate(regions):
        member[r, list(values)] = True
    m = member[:, lab].permute(1, 0, 2, 3)                                                   # [J, R, h, w]
    d = (a - b)
    ad, sq = d.abs().sum(dim=1), (d * d).sum(dim=1)                                          # [J, h, w]
    mf = m.to(torch.float64)
    counts = torch.stack([mf.sum(dim=(2, 3)), (mf * ad[:, None]).sum(dim=(2, 3)), (mf * sq[:, None]).sum(dim=(2, 3)), mf[:, :, 5:h - 5, 5:w - 5].sum(dim=(2, 3))])
    maps = torch.cat([a, b, a * a, b * b, a * b]).reshape(5 * n * c, 1, h, w)
    f = torch.nn.functional.conv2d(torch.nn.functional.conv2d(maps, gx), gy).reshape(5, n, c, h - 10, w - 10)
    ma, mb = f[0], f[1]
    va, vb, cab = f[2] - ma * ma, f[3] - mb * mb, f[4] - ma * mb
    smap = (((2 * ma * mb + IM.C1) * (2 * cab + IM.C2)) / ((ma * ma + mb * mb + IM.C1) * (va + vb + IM.C2))).sum(dim=1, dtype=torch.float64)      # [J, h', w']
    ssim = (mf[:, :, 5:h - 5, 5:w - 5] * smap[:, None]).sum(dim=(2, 3)) / (counts[3] * c)
    return counts, ssim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import region_metrics as M
    from training import metrics as MT
    dev = torch.device('cuda')
    torch.manual_seed(0)
    J, H, W, K = 16, 512, 320, 7
    trip = torch.randint(0, 256, (J, H, 3 * W, 3), dtype=torch.uint8, device=dev)
    near = (trip[:, :, W:2 * W].to(torch.int16) + torch.randint(-9, 10, (J, H, W, 3), device=dev, dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
    trip[:, :, 2 * W:] = near
    labels = torch.randint(0, K, (J, H // 16, W // 16), dtype=torch.uint8, device=dev).repeat_interleave(16, dim=1).repeat_interleave(16, dim=2).contiguous()
    jobs = [(trip[j][:, W:2 * W], trip[j][:, 2 * W:], labels[j]) for j in range(J)]
    names = ('upper', 'lower', 'skin')
    regions = [MT.REGIONS[r] for r in names]
    res = dict(pairs=J, shape=[H, W, 3], regions=list(names))

    call = region_call(jobs, M.region_bits(regions))
    region_ms, (counts, ssim_sum) = device_ms(call, a.reps)
    op_ms, _ = wall_ms(lambda: M.region_metrics_table(jobs, regions), a.reps)
    torch_ms, (tcounts, tssim) = device_ms(lambda: torch_composition(jobs, regions), max(1, a.reps // 4))
    pair_ms, _ = device_ms(native_call([(x, y) for x, y, _ in jobs]), a.reps)
    assert torch.equal(counts.double(), tcounts), 'integer sums differ from the torch composition'
    ssim = ssim_sum / (counts[3].double() * 3)
    res.update(region_ms=round(region_ms, 4), region_op_ms=round(op_ms, 4), torch_ms=round(torch_ms, 4), pair_ms=round(pair_ms, 4),
               region_over_pair=round(region_ms / pair_ms, 3), torch_over_region=round(torch_ms / region_ms, 1),
               ssim_dev=float((ssim - tssim).abs().max()))

    grey = torch.from_numpy(MT.parsing_luts(K)[0]).to(dev)
    table = torch.tensor([int(np.flatnonzero(MT.parsing_luts(K)[0] == k)[0]) for k in range(K)], dtype=torch.uint8, device=dev)
    pred_idx = torch.randint(0, K, (J, H // 16, W // 16), device=dev).repeat_interleave(16, dim=1).repeat_interleave(16, dim=2)
    cells = table[pred_idx][..., None].expand(J, H, W, 3).contiguous()                        # grey RGB cells, as the snapshot grid stores them
    pairs = [(cells[j][:, :, 0], labels[j]) for j in range(J)]
    pred_lut, target_lut = MT.parsing_luts(K)
    confusion_ms, conf = device_ms(confusion_call(pairs, pred_lut, target_lut, K), a.reps)
    tgt64, pred64 = labels.to(torch.int64), grey.to(torch.int64)[cells[..., 0].to(torch.int64)]
    bincount_ms, want = device_ms(lambda: torch.stack([torch.bincount((tgt64[j] * K + pred64[j]).reshape(-1), minlength=K * K) for j in range(J)]), a.reps)
    assert torch.equal(conf.reshape(J, K * K), want), 'confusion differs from torch.bincount'
    res.update(confusion_ms=round(confusion_ms, 4), bincount_ms=round(bincount_ms, 4), bincount_over_confusion=round(bincount_ms / confusion_ms, 1))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
