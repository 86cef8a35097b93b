"""Measure the VGG19 perceptual term (training/vgg_loss.py) on a GPU: N = 4 images of 512 x 512, two generated batches against one real batch as in
Gmain, synthetic weights (training.synthetic.vgg19_state_dict).  One run reports, as a table and as one JSON line:

  - the term's forward + backward (device events), with the trunk's forward convolutions in the direct form (the default) and under the package's
    own policy ('auto': Winograd), and its split: the four pools and the five L1 means timed alone on tensors of the trunk's own shapes (what the term
    runs: pools forward on 12 images, backward on 8; L1 on 2 groups), the convolutions as the remainder;
  - each of the four native kernels beside aten's F.max_pool2d / (x - y).abs().mean() forward and backward on the same tensors, at the largest
    shape of the trunk (8 x 64 x 512 x 512): time and GB/s over the bytes the operator has to move (each input read once, each output written once);
  - one Gmain phase of the full-width networks at N = 4 with vgg_weight 20 against 0, alternating.

    python tools/vgg_loss_bench.py [--reps 20] [--no-gmain]
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))

N, G, RES = 4, 2, 512
POOLED = ((64, 512), (128, 256), (256, 128), (512, 64))                # (C, H = W) of the four pools' inputs
TAPPED = ((64, 512), (128, 256), (256, 128), (512, 64), (512, 32))     # ... of the five taps


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


def gbs(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-gmain', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('vgg_loss_bench.py measures on a GPU; none found')
    dev = torch.device('cuda')
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import vgg_ops
    from training.synthetic import det_tensor, vgg19_state_dict
    from training.vgg_loss import VGG19Features, VGGLoss
    F = torch.nn.functional
    out = dict(shape=[N, 3, RES, RES], groups=G, device=torch.cuda.get_device_name(0))
    sd = vgg19_state_dict()

    # ---- the term, forward + backward
    x = det_tensor('vggbench.x', [G * N, 3, RES, RES], 'uniform').to(dev)
    y = det_tensor('vggbench.y', [N, 3, RES, RES], 'uniform').to(dev)
    for algo in ('direct', 'auto'):
        V = VGGLoss(VGG19Features(sd, forward_algo=algo)).to(dev)

        def term():
            xs = x.detach().requires_grad_(True)
            V([xs[:N], xs[N:]], y).sum().backward()
        out[f'term_ms_{algo}'] = round(device_ms(term, a.reps), 3)

    # ---- its pools and L1 means alone, on the trunk's shapes
    pool_f = pool_b = l1_f = l1_b = 0.0
    for c, r in POOLED:
        t = torch.rand([G * N, c, r, r], device=dev).requires_grad_(True)
        ty = torch.rand([N, c, r, r], device=dev)
        dy = torch.rand([G * N, c, r // 2, r // 2], device=dev)
        pool_f += device_ms(lambda: (vgg_ops.maxpool2x2(t.detach()), vgg_ops.maxpool2x2(ty)), a.reps)
        p = vgg_ops.maxpool2x2(t)
        pool_b += device_ms(lambda: torch.autograd.grad(p, t, dy, retain_graph=True), a.reps)
    for c, r in TAPPED:
        t = torch.rand([G * N, c, r, r], device=dev).requires_grad_(True)
        ty = torch.rand([N, c, r, r], device=dev)
        gw = torch.ones([G], device=dev)
        l1_f += device_ms(lambda: vgg_ops.l1_mean(t.detach(), ty, groups=G), a.reps)
        m = vgg_ops.l1_mean(t, ty, groups=G)
        l1_b += device_ms(lambda: torch.autograd.grad(m, t, gw, retain_graph=True), a.reps)
    out.update(pools_ms=round(pool_f + pool_b, 3), l1_ms=round(l1_f + l1_b, 3),
               convs_ms_direct=round(out['term_ms_direct'] - pool_f - pool_b - l1_f - l1_b, 3),
               convs_ms_auto=round(out['term_ms_auto'] - pool_f - pool_b - l1_f - l1_b, 3))

    # ---- the four kernels beside aten, 8 x 64 x 512 x 512
    c, r = POOLED[0]
    t = torch.rand([G * N, c, r, r], device=dev).requires_grad_(True)
    ty = torch.rand([N, c, r, r], device=dev)
    dy = torch.rand([G * N, c, r // 2, r // 2], device=dev)
    gw = torch.ones([G], device=dev)
    xb, yb = t.numel() * 4, ty.numel() * 4
    kernels = {}

    def aten_l1(tt):
        return torch.stack([(tt[g * N:(g + 1) * N] - ty).abs().mean() for g in range(G)])
    for name, nbytes, native, aten in (
            ('maxpool2x2', xb + xb // 4, lambda: vgg_ops.maxpool2x2(t.detach()), lambda: F.max_pool2d(t.detach(), 2, 2)),
            ('l1_pair_sum', xb + yb, lambda: vgg_ops.l1_mean(t.detach(), ty, groups=G), lambda: aten_l1(t.detach()))):
        kernels[name] = dict(native_ms=device_ms(native, a.reps), aten_ms=device_ms(aten, a.reps), bytes=nbytes)
    pn, pa = vgg_ops.maxpool2x2(t), F.max_pool2d(t, 2, 2)
    ln, la = vgg_ops.l1_mean(t, ty, groups=G), aten_l1(t)
    for name, nbytes, native, aten in (
            ('maxpool2x2_backward', 2 * xb + xb // 4, lambda: torch.autograd.grad(pn, t, dy, retain_graph=True), lambda: torch.autograd.grad(pa, t, dy, retain_graph=True)),
            ('l1_pair_grad', 2 * xb + yb, lambda: torch.autograd.grad(ln, t, gw, retain_graph=True), lambda: torch.autograd.grad(la, t, gw, retain_graph=True))):
        kernels[name] = dict(native_ms=device_ms(native, a.reps), aten_ms=device_ms(aten, a.reps), bytes=nbytes)
    for k in kernels.values():
        k.update(native_gbs=gbs(k['bytes'], k['native_ms']), aten_gbs=gbs(k['bytes'], k['aten_ms']), native_ms=round(k['native_ms'], 4), aten_ms=round(k['aten_ms'], 4))
    out['kernels'] = kernels
    del t, ty, dy, pn, pa, ln, la

    # ---- one Gmain phase, vgg_weight 20 against 0
    if not a.no_gmain:
        from training import training_loop as T
        from training.loss import StyleGAN2Loss
        torch.manual_seed(0)
        Gn, D, DP = T.build_networks(N, dev)
        D.requires_grad_(False)
        DP.requires_grad_(False)
        u = lambda *s: torch.rand(*s, device=dev) * 2 - 1
        batch = dict(real_img=u(N, 3, RES, RES), gen_z=torch.zeros([N, 0], device=dev), style_input=u(N, 45, 128, 128), retain=u(N, 6, RES, RES),
                     pose=u(N, 5, RES, RES), denorm_upper_input=u(N, 3, RES, RES), denorm_lower_input=u(N, 3, RES, RES),
                     denorm_upper_mask=(u(N, 1, RES, RES) > 0).float(), denorm_lower_mask=(u(N, 1, RES, RES) > 0).float(),
                     gt_parsing=torch.randint(0, 7, [N, 1, RES, RES], device=dev).float())
        V = VGGLoss(VGG19Features(sd)).to(dev)
        losses = {w: StyleGAN2Loss(device=dev, **T.g_parts(Gn), D=D, D_parsing=DP, l1_weight=10, mask_weight=30, vgg_weight=w, vgg=V if w else None) for w in (0, 20)}

        def phase(w):
            Gn.zero_grad(set_to_none=True)
            losses[w].accumulate_gradients(phase='Gmain', sync=True, gain=1, **batch)
        times = {0: [], 20: []}
        for w in (0, 20):
            phase(w)                                         # warm-up of both
        for _ in range(3):
            for w in (0, 20):
                times[w].append(device_ms(lambda: phase(w), 3))
        out['gmain_ms_vgg0'] = [round(v, 2) for v in times[0]]
        out['gmain_ms_vgg20'] = [round(v, 2) for v in times[20]]

    print(f"VGG term, forward + backward, N = {N}, G = {G}, {RES} x {RES}: {out['term_ms_direct']} ms (forward convolutions direct), {out['term_ms_auto']} ms (auto)")
    print(f"  of which pools {out['pools_ms']} ms, L1 {out['l1_ms']} ms, convolutions (remainder) {out['convs_ms_direct']} / {out['convs_ms_auto']} ms")
    for name, k in kernels.items():
        print(f"  {name:22s} native {k['native_ms']:8.4f} ms {k['native_gbs']:8.1f} GB/s | aten {k['aten_ms']:8.4f} ms {k['aten_gbs']:8.1f} GB/s")
    if not a.no_gmain:
        print(f"Gmain phase, N = {N}: vgg_weight 0: {out['gmain_ms_vgg0']} ms, vgg_weight 20: {out['gmain_ms_vgg20']} ms")
    print(json.dumps(out))


if __name__ == '__main__':
    main()
