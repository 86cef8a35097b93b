#!/usr/bin/env python3
"""Time ADA's AugmentPipe (training/augment.py, 'bgc') on the GPU with device events after warm-up, N = 4, 3 x 512^2:
augment forward; forward + backward; forward + R1 double backward (autograd.grad(create_graph=True) through a small D, then the penalty's
backward); and one config-4 training iteration with augment_pipe at p = 0.6 against one without, alternating on the same box.

Usage:  python tools/augment_probe.py [--reps 20] [--iters 6]   (prints one JSON line)
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pasta-gan-plusplus_amd')]

import torch  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=6, help='config-4 iterations per arm and round')
    ap.add_argument('--skip-train', action='store_true')
    args = ap.parse_args()
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from training.augment import AugmentPipe, AUGPIPE_SPECS
    dev = torch.device('cuda')
    pipe = AugmentPipe(**AUGPIPE_SPECS['bgc']).requires_grad_(False).to(dev)
    pipe.p.fill_(0.6)
    x = (torch.rand([4, 3, 512, 512], device=dev) * 2 - 1)
    dy = torch.randn_like(x)
    torch.manual_seed(0)
    D = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1, stride=4), torch.nn.Softplus(), torch.nn.Conv2d(8, 1, 3, padding=1, stride=4)).to(dev)
    out = dict(workload='AugmentPipe bgc, p = 0.6, N = 4, 3 x 512^2, device events after warm-up', reps=args.reps)

    def fwd():
        with torch.no_grad():
            pipe(x)

    def fwd_bwd():
        xi = x.detach().requires_grad_(True)
        torch.autograd.grad(pipe(xi), xi, dy)

    def r1():
        xi = x.detach().requires_grad_(True)
        g, = torch.autograd.grad(D(pipe(xi)).sum(), xi, create_graph=True)
        g.square().sum().backward()

    def d_only():
        xi = x.detach().requires_grad_(True)
        g, = torch.autograd.grad(D(xi).sum(), xi, create_graph=True)
        g.square().sum().backward()
    out['forward_ms'] = round(timed(fwd, args.reps), 4)
    out['forward_backward_ms'] = round(timed(fwd_bwd, args.reps), 4)
    out['forward_r1_double_backward_ms'] = round(timed(r1, args.reps), 4)
    out['same_without_augment_ms'] = round(timed(d_only, args.reps), 4)

    if not args.skip_train:
        from training import networks
        from training.loss import StyleGAN2Loss
        from training.training_step import TrainingStep
        torch.manual_seed(0)
        G = networks.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                       synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256)).to(dev).train()
        dkw = dict(c_dim=512, img_resolution=512, channel_base=32768, channel_max=512, conv_clamp=256, epilogue_kwargs=dict(mbstd_group_size=4), num_fp16_res=3)
        Dn = networks.Discriminator(img_channels=6, **dkw).to(dev).train()
        DP = networks.Discriminator(img_channels=10, **dkw).to(dev).train()
        parts = dict(G_mapping=G.mapping, G_synthesis=G.synthesis, G_const_encoding=G.const_encoding, G_style_encoding=G.style_encoding)
        mk_loss = lambda: StyleGAN2Loss(device=dev, **parts, D=Dn, D_parsing=DP, style_mixing_prob=0.9, r1_gamma=10, l1_weight=50, mask_weight=1.0)
        plain = TrainingStep(parts, Dn, DP, mk_loss(), batch_size=4)
        aug = TrainingStep(parts, Dn, DP, mk_loss(), batch_size=4, augment_pipe=pipe, augment_p=0.6)
        g = torch.Generator(device='cpu').manual_seed(100)
        u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)
        n = 4
        batch = dict(real_img=u(n, 3, 512, 512), gen_z=torch.zeros([n, 0], device=dev), style_input=u(n, 45, 128, 128), retain=u(n, 6, 512, 512),
                     pose=u(n, 5, 512, 512), denorm_upper_input=u(n, 3, 512, 512), denorm_lower_input=u(n, 3, 512, 512),
                     denorm_upper_mask=(u(n, 1, 512, 512) > 0).float(), denorm_lower_mask=(u(n, 1, 512, 512) > 0).float(),
                     gt_parsing=torch.randint(0, 7, [n, 1, 512, 512], generator=g).float().to(dev))
        times = {'plain': [], 'augmented': []}
        for step in (plain, aug):                       # warm-up: every phase (batch_idx 0 runs them all)
            for _ in range(2):
                step.run([batch])
        torch.cuda.synchronize()
        for _ in range(3):                              # alternate the two arms, each from batch_idx 0: the same phase mix in both
            for name, step in (('plain', plain), ('augmented', aug)):
                step.batch_idx = 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.iters):
                    step.run([batch])
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.iters)
        out['config4_iteration_ms'] = {k: [round(v, 2) for v in vs] for k, vs in times.items()}
        mp, ma = min(times['plain']), min(times['augmented'])
        out['config4_ratio_augmented_over_plain_best'] = round(ma / mp, 4)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
