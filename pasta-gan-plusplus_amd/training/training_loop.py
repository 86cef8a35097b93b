"""The training driver: a dataset directory in, trained networks out (reference train.py + training/training_loop_fullbody.py, the parts this
package supports).  `TrainFeed` (training/train_fetch.py) turns `TrainSet` items into rounds, `TrainingStep` runs the eight phases on them; this
module builds the networks, runs the two until `kimg`, prints the reference's status line per tick (:669-679), appends the means of the loss reports to
``stats.jsonl`` and writes snapshots: the networks, and -- for a dataset with at least three visualisation persons -- the reference's image grids
(``init_denorm_{upper,lower}.png`` at start, ``fakesNNNNNN_{finetune,parsing}.png`` per image-snapshot tick; training/snapshot_grid.py).

Snapshots are plain ``torch.save`` dicts of ``state_dict``s under the reference's parameter names -- ``G``, ``D``, ``D_parsing``, ``G_ema``,
``augment_p``, ``cur_nimg`` -- which ``--resume`` reads back; ``--resume`` also reads a reference snapshot (.pkl) through ``checkpoint.load_into``
(nothing in it is executed).  The VGG19 perceptual term (``vgg_weight`` > 0) needs ``vgg_ckpt``, a torchvision-format ``vgg19`` state dict
(training/vgg_loss.py); its tensors are buffers of the loss, in no snapshot.  The contextual term (``contextual_weight`` > 0) likewise needs
``contextual_ckpt``, a state dict under the reference's ``vgg19_conv.pth`` key names (training/contextual_loss.py).  Writing the reference's own
pickle format is out of scope (its pickles embed module source), as are the reference's detector-based metrics (FID, KID, PR, PPL, IS), zip datasets and
tensorboard.  ``metrics`` (``--metrics l1,psnr,ssim``) is opt-in: on image-snapshot ticks the reconstruction error of the grid's diagonal cells goes
into ``stats.jsonl`` as ``Metric/recon_*`` (training/metrics.py); ``--metric-regions`` restricts it to label regions as well, and the name
``parsing`` scores the parsing head (``Metric/parsing_*``)."""

import argparse
import json
import os
import time

import torch

from . import augment
from . import checkpoint
from . import dataset as ds_mod
from . import networks
from . import snapshot_grid
from . import train_fetch
from .loss import StyleGAN2Loss
from .training_step import TrainingStep

FULL_WIDTH = dict(channel_base=32768, channel_max=512)


def build_networks(batch_gpu, device, width=None):
    """G, D, D_parsing with the reference's train.py options for the full-body model (:191-202); `width` overrides channel_base / channel_max."""
    width = dict(FULL_WIDTH, **(width or {}))
    G = networks.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                   synthesis_kwargs=dict(conv_clamp=256, **width))
    dkw = dict(c_dim=512, img_resolution=512, conv_clamp=256, num_fp16_res=3 if torch.device(device).type == 'cuda' else 0,
               epilogue_kwargs=dict(mbstd_group_size=min(batch_gpu, 4)), **width)
    D, D_parsing = networks.Discriminator(img_channels=6, **dkw), networks.Discriminator(img_channels=10, **dkw)
    return [m.to(device).train() for m in (G, D, D_parsing)]


def g_parts(G):
    return dict(G_mapping=G.mapping, G_synthesis=G.synthesis, G_const_encoding=G.const_encoding, G_style_encoding=G.style_encoding)


def save_snapshot(path, G, D, D_parsing, G_ema, augment_p, cur_nimg):
    plain = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
    torch.save(dict(G=plain(G), D=plain(D), D_parsing=plain(D_parsing), G_ema=plain(G_ema), augment_p=float(augment_p), cur_nimg=int(cur_nimg)), path)


def resume_from(path, G, D, D_parsing, G_ema):
    """Load a snapshot of this driver (a ``torch.save`` dict of state_dicts) or of the reference (.pkl, read without executing anything in it).
    Returns (augment_p, cur_nimg) of the former, (None, 0) for the latter."""
    nets = dict(G=G, D=D, D_parsing=D_parsing, G_ema=G_ema)
    if str(path).endswith('.pkl'):
        for key, module in nets.items():
            checkpoint.load_into(module, path, key=key)
        return None, 0
    snap = torch.load(path, map_location='cpu', weights_only=True)
    for key, module in nets.items():
        checkpoint.load_into(module, snap[key])
    return snap.get('augment_p'), int(snap.get('cur_nimg', 0))


def format_time(seconds):
    s = int(round(seconds))
    if s < 60:
        return f'{s}s'
    if s < 3600:
        return f'{s // 60}m {s % 60:02d}s'
    return f'{s // 3600}h {s // 60 % 60:02d}m {s % 60:02d}s'


def image_interval(snap, image_snap):
    """Ticks between image snapshots: `snap` drives both kinds of snapshot, as in the reference, unless `image_snap` is given; 0 / None: none."""
    return (snap if image_snap is None else image_snap) or 0


def check_augment_options(aug, p, augpipe):
    """The option rules of the reference's train.py (:259-296); ValueError with the text the command line prints."""
    if aug not in ('ada', 'noaug', 'fixed'):
        raise ValueError("--aug must be 'ada', 'noaug' or 'fixed'")
    if aug == 'fixed' and p is None:
        raise ValueError('--aug=fixed requires specifying --p')
    if p is not None:
        if aug != 'fixed':
            raise ValueError('--p can only be specified with --aug=fixed')
        if not 0 <= p <= 1:
            raise ValueError('--p must be between 0 and 1')
    if augpipe not in augment.AUGPIPE_SPECS:
        raise ValueError(f'--augpipe must be one of {", ".join(augment.AUGPIPE_SPECS)}')
    if augpipe != 'bgc' and aug == 'noaug':
        raise ValueError('--augpipe cannot be specified with --aug=noaug')


def training_loop(run_dir, data, batch=32, batch_gpu=4, gamma=10, l1_weight=50, mask_weight=1.0, vgg_weight=0, contextual_weight=0, aug='ada', target=0.6,
                  seed=0, workers=3, kimg=25000, tick=4, snap=50, resume=None, device='cuda', width=None, dataset_kwargs=None, on_start=None, image_snap=None,
                  vgg_ckpt=None, metrics=None, augpipe='bgc', p=None, metric_regions=None, contextual_ckpt=None):
    """Train on the dataset directory `data` for `kimg` thousand images (one process, one GPU: `batch` = `batch_gpu` x accumulation rounds).
    Returns the `TrainingStep`.  `width` narrows the networks (tests); `on_start(G, D, D_parsing, G_ema)` is called after `resume` was applied.
    `snap` drives both kinds of snapshot, as in the reference; `image_snap` overrides the interval of the image grids (0: none).
    `vgg_weight` > 0 turns the VGG19 perceptual term on and needs `vgg_ckpt` (no default path): NotImplementedError without one, FileNotFoundError for
    a path that does not exist, both before any network is built; `contextual_weight` > 0 and `contextual_ckpt` likewise.  `metrics`: None, or names out of 'l1', 'psnr', 'ssim' -- each image-snapshot tick
    then adds ``Metric/recon_<name>`` (training/metrics.py) to its ``stats.jsonl`` line and prints them after the status line -- and 'parsing':
    ``Metric/parsing_acc`` / ``Metric/parsing_miou`` of the grid's predicted parsing.  `metric_regions`: None, or names out of ``metrics.REGIONS`` --
    ``Metric/recon_<name>_<region>`` for each selected l1 / psnr / ssim (ValueError, before anything is built, when none of the three is selected).
    `aug`: 'ada' (adaptive, towards `target`), 'fixed' (the constant probability `p`, which also wins over a resumed snapshot's) or 'noaug'; `augpipe` names
    the pipeline out of ``augment.AUGPIPE_SPECS`` (reference train.py:259-305).  On a GPU the pipe's late stages run natively (``set_native_late``)."""
    if vgg_weight and vgg_ckpt is None:
        raise NotImplementedError('vgg_weight > 0 needs --vgg_ckpt: a torchvision-format vgg19 state dict (vgg19-dcbb9e9d.pth is not shipped)')
    if vgg_weight and not os.path.isfile(vgg_ckpt):
        raise FileNotFoundError(f'--vgg_ckpt "{vgg_ckpt}" does not exist')
    if contextual_weight and contextual_ckpt is None:
        raise NotImplementedError('contextual_weight > 0 needs --contextual_ckpt: a state dict under the key names of vgg19_conv.pth (which is not shipped)')
    if contextual_weight and not os.path.isfile(contextual_ckpt):
        raise FileNotFoundError(f'--contextual_ckpt "{contextual_ckpt}" does not exist')
    metrics_mod = None
    if metrics:
        from . import metrics as metrics_mod
        metrics = metrics_mod.parse_metrics(metrics)
    if metric_regions:
        from . import metrics as metrics_mod
        metric_regions = metrics_mod.parse_regions(metric_regions)
        metrics_mod.check_region_options(metrics, metric_regions)
    if batch % batch_gpu:
        raise ValueError('--batch must be a multiple of --batch-gpu')
    check_augment_options(aug, p, augpipe)
    dev = torch.device(device)
    os.makedirs(run_dir, exist_ok=True)
    torch.manual_seed(seed)
    G, D, D_parsing = build_networks(batch_gpu, dev, width)
    parts = g_parts(G)
    import copy
    G_ema = copy.deepcopy(G).eval().requires_grad_(False)
    augment_p, start_nimg = None, 0
    if resume is not None:
        print(f'Resuming from "{resume}"')
        augment_p, start_nimg = resume_from(resume, G, D, D_parsing, G_ema)
    if on_start is not None:
        on_start(G, D, D_parsing, G_ema)

    sums = {}                                                 # report name -> list of per-call means (device scalars; read once per tick)

    def report(name, value):
        if name.startswith('Loss/') and name != 'Loss/signs/real' and isinstance(value, torch.Tensor):      # (a phase reports 0 for a term it skips)
            sums.setdefault(name, []).append(value.detach().float().mean())
    vgg = None
    if vgg_weight:
        from . import vgg_loss
        vgg = vgg_loss.VGGLoss(vgg_loss.VGG19Features(vgg_loss.load_vgg19(vgg_ckpt))).to(dev)
    contextual = None
    if contextual_weight:
        from . import contextual_loss as cx
        contextual = cx.ContextualLoss(cx.VGG19ConvFeatures(cx.load_vgg19_conv(contextual_ckpt))).to(dev)
    loss = StyleGAN2Loss(device=dev, **parts, D=D, D_parsing=D_parsing, style_mixing_prob=0.9, r1_gamma=gamma, l1_weight=l1_weight, vgg_weight=vgg_weight,
                         vgg=vgg, contextual_weight=contextual_weight, contextual=contextual, mask_weight=mask_weight, report=report)
    pipe = augment.AugmentPipe(**augment.AUGPIPE_SPECS[augpipe]).to(dev).set_native_late(dev.type == 'cuda') if aug != 'noaug' else None
    if aug == 'fixed':
        augment_p = p
    step = TrainingStep(parts, D, D_parsing, loss, batch_size=batch, G_ema_parts=g_parts(G_ema), augment_pipe=pipe,
                        augment_p=augment_p if augment_p is not None else 0, ada_target=target if aug == 'ada' else None)
    step.cur_nimg = start_nimg
    dataset = ds_mod.TrainSet(data, seed=seed, **(dataset_kwargs or {}))
    feed = train_fetch.TrainFeed(dataset, batch_gpu, rounds=batch // batch_gpu, seed=seed, workers=workers, device=dev, z_dim=G.z_dim)

    image_snap = image_interval(snap, image_snap)
    grid = None
    if image_snap:
        if len(dataset.vis_index) < 3:
            print(f'Only {len(dataset.vis_index)} visualisation persons (train_img_front_vis_512_220414/): image snapshots are off.')
        else:
            print('Exporting sample images...')
            grid = snapshot_grid.setup_snapshot_grid(dataset, dev)
            for name, array in zip(('init_denorm_upper.png', 'init_denorm_lower.png'), grid.canvas_grids()):
                snapshot_grid.save_png(os.path.join(run_dir, name), array)
    if metrics and grid is None:
        print('No image grid: --metrics is off.')

    print(f'Training for {kimg} kimg...\n')
    start_time = tick_start_time = time.time()
    cur_tick, tick_start_nimg, maintenance_time = 0, step.cur_nimg, 0.0
    while True:
        step.run(next(feed))
        done = step.cur_nimg >= kimg * 1000
        if not done and cur_tick != 0 and step.cur_nimg < tick_start_nimg + tick * 1000:
            continue
        tick_end_time = time.time()
        p_now = float(pipe.p.cpu()) if pipe is not None else 0.0
        means = {k: float(torch.stack(v).mean().cpu()) for k, v in sums.items()}
        sums.clear()
        gpumem = torch.cuda.max_memory_allocated(dev) / 2 ** 30 if dev.type == 'cuda' else 0.0
        print(' '.join([f'tick {cur_tick:<5d}', f'kimg {step.cur_nimg / 1e3:<8.1f}', f'time {format_time(tick_end_time - start_time):<12s}',
                        f'sec/tick {tick_end_time - tick_start_time:<7.1f}',
                        f'sec/kimg {(tick_end_time - tick_start_time) / max(step.cur_nimg - tick_start_nimg, 1) * 1e3:<7.2f}',
                        f'maintenance {maintenance_time:<6.1f}', f'gpumem {gpumem:<6.2f}', f'augment {p_now:.3f}']), flush=True)
        image_tick = grid is not None and (done or cur_tick % image_snap == 0)
        rendered = None
        if metrics and image_tick:                                # the grid is rendered before the stats line is written: its figures go into it
            rendered = grid.render(G_ema, batch_gpu)
            recon = metrics_mod.grid_reconstruction(grid, metrics, metric_regions)
            means.update(recon)
            print(' '.join(f'{k} {v:.6g}' for k, v in recon.items()), flush=True)
        with open(os.path.join(run_dir, 'stats.jsonl'), 'a') as f:
            f.write(json.dumps(dict(means, **{'Progress/tick': cur_tick, 'Progress/kimg': step.cur_nimg / 1e3, 'Progress/augment': p_now,
                                              'timestamp': time.time()})) + '\n')
        if image_tick:
            for name, array in zip(('finetune', 'parsing'), rendered if rendered is not None else grid.render(G_ema, batch_gpu)):
                snapshot_grid.save_png(os.path.join(run_dir, f'fakes{step.cur_nimg // 1000:06d}_{name}.png'), array)
        if snap is not None and (done or cur_tick % snap == 0):
            save_snapshot(os.path.join(run_dir, f'network-snapshot-{step.cur_nimg // 1000:06d}.pt'), G, D, D_parsing, G_ema, p_now, step.cur_nimg)
        cur_tick += 1
        tick_start_nimg, tick_start_time = step.cur_nimg, time.time()
        maintenance_time = tick_start_time - tick_end_time
        if done:
            break
    print('\nExiting...')
    return step


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train PASTA-GAN++ on a dataset directory (the reference\'s train.py, the options this package supports).')
    p.add_argument('--data', required=True, help='training data directory (the sub-datasets and train_random_mask_acgpn/)')
    p.add_argument('--outdir', required=True, help='where stats.jsonl and the snapshots go')
    p.add_argument('--batch', type=int, default=32, help='images per iteration')
    p.add_argument('--batch-gpu', type=int, default=4, help='images per accumulation round')
    p.add_argument('--gamma', type=float, default=10, help='R1 weight')
    p.add_argument('--l1_weight', type=float, default=50)
    p.add_argument('--mask_weight', type=float, default=1.0)
    p.add_argument('--vgg_weight', type=float, default=0, help='weight of the VGG19 perceptual term (the reference\'s train.sh: 20); > 0 needs --vgg_ckpt')
    p.add_argument('--vgg_ckpt', default=None, help='torchvision-format vgg19 state dict (vgg19-dcbb9e9d.pth); no default path')
    p.add_argument('--contextual_weight', type=float, default=0, help='weight of the contextual term (the reference\'s train.sh: 0); > 0 needs --contextual_ckpt')
    p.add_argument('--contextual_ckpt', default=None, help='state dict under the key names of the reference\'s vgg19_conv.pth; no default path')
    p.add_argument('--aug', choices=['ada', 'noaug', 'fixed'], default='ada', help="augmentation mode; 'fixed' needs --p")
    p.add_argument('--p', type=float, default=None, help='augmentation probability for --aug=fixed')
    p.add_argument('--target', type=float, default=0.6, help='ADA target')
    p.add_argument('--augpipe', choices=list(augment.AUGPIPE_SPECS), default='bgc', help='augmentation pipeline')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--workers', type=int, default=3, help='DataLoader worker processes')
    p.add_argument('--kimg', type=float, default=25000, help='training length in thousands of images')
    p.add_argument('--tick', type=float, default=4, help='status line every so many thousand images')
    p.add_argument('--snap', type=int, default=50, help='snapshot every so many ticks')
    p.add_argument('--image-snap', type=int, default=None, help='image grids every so many ticks (default: --snap; 0: none)')
    p.add_argument('--resume', help='a snapshot of this driver (.pt) or a reference network pickle (.pkl)')
    p.add_argument('--device', default='cuda')
    p.add_argument('--metrics', default='none', help="'none' or a comma-separated list out of l1, psnr, ssim: reconstruction error of the snapshot "
                   "grid's diagonal cells on image-snapshot ticks (the reference's fid50k_full etc. need a detector network and are refused); "
                   "parsing: pixel accuracy and mean IoU of the grid's predicted parsing against the loader's gt_parsing")
    p.add_argument('--metric-regions', default='none', help="'none' or a comma-separated list out of upper, lower, garment, skin, other: the selected "
                   "l1 / psnr / ssim over these gt_parsing regions too (Metric/recon_<name>_<region>)")
    return p.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    metrics = None
    if a.metrics.strip().lower() not in ('', 'none'):
        from . import metrics as metrics_mod
        try:
            metrics = metrics_mod.parse_metrics(a.metrics)
        except ValueError as e:
            raise SystemExit(str(e))
    regions = None
    if a.metric_regions.strip().lower() not in ('', 'none'):
        from . import metrics as metrics_mod
        try:
            regions = metrics_mod.parse_regions(a.metric_regions)
            metrics_mod.check_region_options(metrics, regions)
        except ValueError as e:
            raise SystemExit(str(e))
    try:
        check_augment_options(a.aug, a.p, a.augpipe)
    except ValueError as e:
        raise SystemExit(str(e))
    return training_loop(a.outdir, a.data, batch=a.batch, batch_gpu=a.batch_gpu, gamma=a.gamma, l1_weight=a.l1_weight, mask_weight=a.mask_weight,
                         vgg_weight=a.vgg_weight, contextual_weight=a.contextual_weight, aug=a.aug, target=a.target, seed=a.seed, workers=a.workers,
                         kimg=a.kimg, tick=a.tick, snap=a.snap, resume=a.resume, device=a.device, image_snap=a.image_snap, vgg_ckpt=a.vgg_ckpt, contextual_ckpt=a.contextual_ckpt, metrics=metrics,
                         augpipe=a.augpipe, p=a.p, metric_regions=regions)
