"""Measure the try-on generator's 16-bit mode (SynthesisNetworkFull_v18.set_half) on a GPU, in one process.

Reports as one JSON line:
  - config-2-shaped synthesis forward (512^2, full width, N = --batch) in images/s for precision fp32 and bf16 (events around --steps forwards after --warmup);
  - the two kernels of csrc/spade16.hip at the generator's shapes: microseconds per call, the bytes the call moves and the bandwidth that makes;
  - the max-abs deviation of the bf16 outputs from the float32 ones of the same network (img, finetune_img, pred_parsing) and the share of pixels whose
    `pred_parsing` argmax differs.

    python tools/tryon_half_bench.py --batch 8 --steps 10 --warmup 3
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        out = fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps, out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batch', type=int, default=8)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    args = p.parse_args(argv)
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import conv2d_mfma16
    from training import networks as PN
    from training.synthetic import fill_module_, synthesis_inputs
    dev = torch.device('cuda', 0)
    n = args.batch
    net = fill_module_(PN.SynthesisNetworkFull_v18(w_dim=512, img_resolution=512, img_channels=3, conv_clamp=256), 'cfg2.').to(dev).eval().requires_grad_(False)
    inp = synthesis_inputs(n, num_ws=net.num_ws)
    inp = {k: ({r: t.to(dev) for r, t in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in inp.items()}
    result = dict(batch=n, steps=args.steps, device=torch.cuda.get_device_name(0))
    outs = {}
    with torch.no_grad():
        for name, dtype in (('fp32', None), ('bf16', torch.bfloat16)):
            net.set_half(dtype)
            ms, outs[name] = timed(lambda: net(**inp, noise_mode='const'), args.steps, args.warmup)
            result[name] = dict(ms_per_step=round(ms, 3), images_per_s=round(1000.0 * n / ms, 1))
        net.set_half(None)
        result['deviation_bf16_vs_fp32'] = {nm: float((a - b).abs().max()) for nm, a, b in zip(('img', 'finetune_img', 'pred_parsing'), outs['bf16'], outs['fp32'])}
        result['range_fp32'] = {nm: float(b.abs().max()) for nm, b in zip(('img', 'finetune_img', 'pred_parsing'), outs['fp32'])}
        result['parsing_argmax_differs'] = float((outs['bf16'][2].argmax(1) != outs['fp32'][2].argmax(1)).float().mean())
        kernels = {}
        for c, res in ((128, 256), (64, 512)):          # spade_b256_*, spade_b512 at full width
            x = torch.randn([n, c, res, res], device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            gb = torch.randn([n, 2 * c, res, res], device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            ms, (mean, rstd) = timed(lambda: conv2d_mfma16.instance_norm_stats16(x), args.steps, args.warmup)
            nbytes = 2 * x.numel()
            kernels[f'stats N{n} C{c} {res}x{res}'] = dict(us=round(ms * 1e3, 1), mbytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / ms / 1e9, 2))
            ms, _ = timed(lambda: conv2d_mfma16.spade_combine16(x, mean, rstd, gb, act='relu', gain=2 ** 0.5), args.steps, args.warmup)
            nbytes = 2 * 4 * x.numel()
            kernels[f'combine N{n} C{c} {res}x{res}'] = dict(us=round(ms * 1e3, 1), mbytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / ms / 1e9, 2))
        result['kernels'] = kernels
    print(json.dumps(result))


if __name__ == '__main__':
    main()
