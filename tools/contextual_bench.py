"""Measure the contextual term (training/contextual_loss.py) on a GPU: N = 4 images of 512 x 512, two generated batches against one real batch as
in Gmain (S = 8), synthetic weights (training.synthetic.vgg19_conv_state_dict).  One run reports, as a table and as one JSON line:

  - ``pg_cx_forward`` and ``pg_cx_backward`` alone (device events) at the three level shapes of a 512 x 512 image -- r52 [512, 32 x 32], r42 [512, 64 x 64],
    avg_pool2(r32) [256, 64 x 64] -- with the rate over the multiply-adds of their GEMM sweeps (two forward, two backward), and the two prepare kernels;
  - the whole term forward + backward (trunk included);
  - the torch composition of the same formula (``contextual_ops.contextual_loss_composition``) on the GPU, forward + backward at each level, at the
    largest S <= 8 at which it runs without an out-of-memory error (reported as ``composition_S``);
  - one Gmain phase of the full-width networks at N = 4 with contextual_weight 1 against 0, alternating.

    python tools/contextual_bench.py [--reps 10] [--no-gmain] [--no-composition]
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))

N, G, RES = 4, 2, 512
LEVELS = (('r52', 512, 32), ('r42', 512, 64), ('pool2(r32)', 256, 64))      # (name, C, H = W)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-gmain', action='store_true')
    ap.add_argument('--no-composition', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('contextual_bench.py measures on a GPU; none found')
    dev = torch.device('cuda')
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import contextual_ops as ops
    from training.contextual_loss import ContextualLoss, VGG19ConvFeatures
    from training.synthetic import det_tensor, vgg19_conv_state_dict
    S = G * N
    out = dict(shape=[N, 3, RES, RES], groups=G, device=torch.cuda.get_device_name(0), levels={})

    # ---- the kernels alone, per level
    for name, c, r in LEVELS:
        y = 30 * torch.relu(torch.randn([N, c, r, r], device=dev))
        x = 0.3 * y.repeat([G, 1, 1, 1]) + 0.7 * 30 * torch.relu(torch.randn([S, c, r, r], device=dev))
        xn, yn, rx = ops.prepare(x, y)
        loss, stats = ops.forward_sweeps(xn, yn, c, 0.1)
        gout = torch.ones([S], device=dev)
        dxn = ops.backward_sweep(xn, yn, stats, gout, c, 0.1)
        flop = 2.0 * 2 * S * (r * r) ** 2 * c                        # two GEMM sweeps of S * P * P * C multiply-adds, forward and backward alike
        lv = dict(C=c, P=r * r,
                  prepare_ms=device_ms(lambda: ops.prepare(x, y), a.reps),
                  forward_ms=device_ms(lambda: ops.forward_sweeps(xn, yn, c, 0.1), a.reps),
                  backward_ms=device_ms(lambda: ops.backward_sweep(xn, yn, stats, gout, c, 0.1), a.reps),
                  prepare_backward_ms=device_ms(lambda: ops.prepare_backward(dxn, xn, rx, x.shape), a.reps))
        lv['forward_tflops'] = round(flop / (lv['forward_ms'] * 1e-3) / 1e12, 2)
        lv['backward_tflops'] = round(flop / (lv['backward_ms'] * 1e-3) / 1e12, 2)

        def native():
            xs = x.detach().requires_grad_(True)
            ops.contextual_loss(xs, y, groups=G).sum().backward()
        lv['op_ms'] = device_ms(native, a.reps)
        if not a.no_composition:
            for s_try in (8, 4, 2, 1):                               # the composition holds ~ 5 P x P float matrices per sample, and autograd's copies
                try:
                    xs0, ys0 = x[:s_try], y.repeat([G, 1, 1, 1])[:s_try]

                    def composed():
                        xs = xs0.detach().requires_grad_(True)
                        ops.contextual_loss_composition(xs, ys0).sum().backward()
                    lv['composition_ms'] = device_ms(composed, max(2, a.reps // 3))
                    lv['composition_S'] = s_try
                    break
                except torch.OutOfMemoryError:
                    torch.cuda.empty_cache()
        out['levels'][name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in lv.items()}
        del x, y, xn, yn, rx, stats, dxn

    # ---- the whole term
    M = ContextualLoss(VGG19ConvFeatures(vgg19_conv_state_dict())).to(dev)
    x = det_tensor('cxbench.x', [S, 3, RES, RES], 'uniform').to(dev)
    y = det_tensor('cxbench.y', [N, 3, RES, RES], 'uniform').to(dev)

    def term():
        xs = x.detach().requires_grad_(True)
        M([xs[:N], xs[N:]], y).sum().backward()
    out['term_ms'] = round(device_ms(term, a.reps), 3)

    # ---- one Gmain phase, contextual_weight 1 against 0
    if not a.no_gmain:
        from training import training_loop as T
        from training.loss import StyleGAN2Loss
        torch.manual_seed(0)
        Gn, D, DP = T.build_networks(N, dev)
        D.requires_grad_(False)
        DP.requires_grad_(False)
        u = lambda *s: torch.rand(*s, device=dev) * 2 - 1              # noqa: E731
        batch = dict(real_img=u(N, 3, RES, RES), gen_z=torch.zeros([N, 0], device=dev), style_input=u(N, 45, 128, 128), retain=u(N, 6, RES, RES),
                     pose=u(N, 5, RES, RES), denorm_upper_input=u(N, 3, RES, RES), denorm_lower_input=u(N, 3, RES, RES),
                     denorm_upper_mask=(u(N, 1, RES, RES) > 0).float(), denorm_lower_mask=(u(N, 1, RES, RES) > 0).float(),
                     gt_parsing=torch.randint(0, 7, [N, 1, RES, RES], device=dev).float())
        losses = {w: StyleGAN2Loss(device=dev, **T.g_parts(Gn), D=D, D_parsing=DP, l1_weight=10, mask_weight=30, contextual_weight=w,
                                   contextual=M if w else None) for w in (0, 1)}

        def phase(w):
            Gn.zero_grad(set_to_none=True)
            losses[w].accumulate_gradients(phase='Gmain', sync=True, gain=1, **batch)
        times = {0: [], 1: []}
        for w in (0, 1):
            phase(w)
        for _ in range(3):
            for w in (0, 1):
                times[w].append(device_ms(lambda: phase(w), 3))
        out['gmain_ms_cx0'] = [round(v, 2) for v in times[0]]
        out['gmain_ms_cx1'] = [round(v, 2) for v in times[1]]

    for name, lv in out['levels'].items():
        print(f"{name:11s} C {lv['C']:3d} P {lv['P']:4d} S {S}: pg_cx_forward {lv['forward_ms']:7.3f} ms ({lv['forward_tflops']} TFLOP/s), pg_cx_backward "
              f"{lv['backward_ms']:7.3f} ms ({lv['backward_tflops']} TFLOP/s), prepare {lv['prepare_ms']:.3f} + {lv['prepare_backward_ms']:.3f} ms; op forward + "
              f"backward {lv['op_ms']:.3f} ms" + (f"; torch composition at S = {lv['composition_S']}: {lv['composition_ms']:.3f} ms" if 'composition_ms' in lv else ''))
    print(f"contextual term, forward + backward, N = {N}, G = {G}, {RES} x {RES}: {out['term_ms']} ms")
    if not a.no_gmain:
        print(f"Gmain phase, N = {N}: contextual_weight 0: {out['gmain_ms_cx0']} ms, contextual_weight 1: {out['gmain_ms_cx1']} ms")
    print(json.dumps(out))


if __name__ == '__main__':
    main()
