"""The training loader's GPU half on the MI355X: ``normalize_batch(part='train')`` against the per-sample CPU route, pg_train_fetch
(csrc/train_fetch.hip) against `fetch_reference` in torch on the same GPU tensors, and a whole `TrainFeed` iteration against the CPU route of the
same items and records -- all bit for bit -- with the launch count and the absence of host synchronisation checked."""

import numpy as np
import pytest
import torch

from test_train_loader import PERSONS, RECORDS, index_of, write_train_root

PIL = pytest.importorskip('PIL.Image')

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def train_set(tmp_path_factory):
    from training.dataset import TrainSet
    return TrainSet(write_train_root(str(tmp_path_factory.mktemp('train'))), shuffle=False, device='cpu')


@pytest.fixture(scope='module')
def items(train_set):
    """The four persons' unrouted items and their CPU routing."""
    from training import patch_routing as P
    from training.dataset import NO_ERASE
    out = []
    for _, name, _ in PERSONS:
        u = train_set.unrouted(index_of(train_set, name), NO_ERASE)
        cpu = P.normalize(u['upper_img'], u['lower_img'], u['upper_mask'], u['lower_mask'], u['sleeve'], u['person_kp'], u['person_kp'], 2, device='cpu',
                          part='train')
        out.append((u, cpu))
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize('n', [1, 3, 16])
def test_normalize_batch_train_equals_the_cpu_route_in_three_launches(items, n):
    from training import patch_routing as P
    gpu = lambda a: torch.from_numpy(a).cuda()
    samples = []
    for i in range(n):
        u = items[i % 4][0]
        samples.append((gpu(u['upper_img']), gpu(u['lower_img']), gpu(u['upper_mask']), gpu(u['lower_mask']), gpu(u['sleeve']), u['person_kp'], u['person_kp']))
    torch.cuda.synchronize()
    P.normalize_batch(samples, 2, part='train')                # warm-up: plugin loading
    torch.cuda.synchronize()
    P.traffic_counter = dict(bytes=0, launches=0)
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = P.normalize_batch(samples, 2, part='train')
    finally:
        torch.cuda.set_sync_debug_mode(0)
        launches = P.traffic_counter['launches']
        P.traffic_counter = None
    assert launches == 3 and len(got) == 6
    shapes = [(n, 128, 128, 30), (n, 128, 128, 15), (n, 512, 512, 3), (n, 512, 512, 3), (n, 128, 128, 30), (n, 128, 128, 15)]
    for k, (g, shape) in enumerate(zip(got, shapes)):
        assert g.device.type == 'cuda' and g.dtype == torch.uint8 and tuple(g.shape) == shape
        for i in range(n):
            assert torch.equal(g[i].cpu(), items[i % 4][1][k]), (n, i, k)
    assert int(got[3][0].sum()) > 0 and int(got[4][min(2, n - 1)].sum()) > 0


def _random_batch(n, seed):
    """A collate_train-shaped batch on the GPU with random bytes, plus routed-shaped tensors whose lower masks have equal channels; the records
    cycle through RECORDS; sample 0 holds every byte value and a NaN skin median; the last sample's routed lower mask of part 0 is empty."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    rb = lambda *s: torch.randint(0, 256, s, generator=g, device='cuda', dtype=torch.int32).to(torch.uint8)
    sparse = lambda t: t * (rb(*t.shape[:-1], 1) < 90)
    image, pose = rb(n, 512, 512, 3), rb(n, 512, 512, 3)
    image[0, 0, :256] = torch.arange(256, device='cuda', dtype=torch.uint8)[:, None]
    skin = torch.randint(0, 512, (n, 3), generator=g, device='cuda').to(torch.float32) / 2
    skin[0, 1] = float('nan')
    recs = [RECORDS[i % len(RECORDS)] for i in range(n)]
    batch = dict(image=image, pose=pose, retain_mask=(rb(n, 512, 512, 1) > 128).to(torch.uint8), gt_parsing=rb(n, 512, 512, 1) % 7,
                 random_mask=sparse(rb(n, 512, 512, 1)), skin=skin, label=torch.arange(n, device='cuda', dtype=torch.int32) % 3, bound_train=rb(n, 512),
                 erase=torch.tensor([[r[0], r[1], r[2], r[4]] for r in recs], dtype=torch.int32).cuda(),
                 band_u=torch.tensor([r[3] for r in recs], dtype=torch.float32).cuda())
    masks_lower = (rb(n, 128, 128, 5, 1) < 60).to(torch.uint8).mul(255).expand(n, 128, 128, 5, 3).reshape(n, 128, 128, 15).contiguous()
    for i in range(n):
        masks_lower[i, :20 + 11 * (i % 7)] = 0                 # the first non-zero row varies
    masks_lower[n - 1, :, :, 0:3] = 0
    routed = (rb(n, 128, 128, 30), rb(n, 128, 128, 15), sparse(rb(n, 512, 512, 3)), sparse(rb(n, 512, 512, 3)), rb(n, 128, 128, 30), masks_lower)
    return batch, routed, recs


@pytest.mark.parametrize('n', [1, 3, 16])
def test_fetch_kernel_equals_fetch_reference(n):
    from training import train_fetch as F
    batch, routed, recs = _random_batch(n, 11 + n)
    ext = F.lower_mask_extents(routed)
    want = F.fetch_reference(batch, routed, ext)
    F.launch_counter = dict(fetch=0)
    try:
        got = F.fetch(batch, routed, ext)
        assert F.launch_counter == dict(fetch=1)
    finally:
        F.launch_counter = None
    assert list(got) == list(want) == list(F.KEYS)
    for k in F.KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype == torch.float32
        assert torch.equal(_bits(got[k]), _bits(want[k])), (n, k)                       # NaN included
    assert torch.isnan(got['retain'][0, 4]).all() and not torch.isnan(got['retain'][0, 3]).any()
    # the erase did what the record says (not only what the reference function says)
    unit_lower = routed[1].permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1
    ext_h = ext.cpu()
    for i, rec in enumerate(recs):
        lower = got['style_input'][i, 30:]
        if int(ext_h[i, 0]) < 0 or rec[0] == 0:
            assert torch.equal(lower, unit_lower[i]), (i, rec)
        elif rec[0] == 1:
            assert (lower[0:3] == -1).all() and torch.equal(lower[6:9], unit_lower[i, 6:9])
            assert (lower[3:6, :rec[2]] == -1).all() and torch.equal(lower[3:6, rec[2]:], unit_lower[i, 3:6, rec[2]:])
        else:
            ty = int(ext_h[i, 0])
            by = 128 if rec[3] > 0.99 else (ty + 1 if rec[3] == 0.0 else None)
            if by is not None:
                assert (lower[0:3, ty:by] == -1).all() and torch.equal(lower[0:3, by:], unit_lower[i, 0:3, by:]) and torch.equal(lower[0:3, :ty], unit_lower[i, 0:3, :ty])
    assert int(ext_h[n - 1, 0]) == -1 and (n == 1 or int(ext_h[0, 0]) == 20)


def test_fetch_refuses_bad_arguments():
    from training import train_fetch as F
    from torch_utils.ops import _native as nat
    batch, routed, _ = _random_batch(2, 5)
    ext = F.lower_mask_extents(routed)
    with pytest.raises(nat.NativeOpError):
        F.fetch(dict(batch, skin=batch['skin'].double()), routed, ext)
    with pytest.raises(nat.NativeOpError):
        F.fetch(dict(batch, image=batch['image'].permute(0, 2, 1, 3)), routed, ext)
    with pytest.raises(nat.NativeOpError):
        F.fetch(batch, (routed[0][:, :, :126],) + routed[1:], ext)
    lib = F._init().lib
    assert lib.pg_train_fetch(None, 2, 512, 512, 128, 128, None) == -1


def test_a_train_feed_iteration_equals_the_cpu_route_without_a_host_sync(train_set):
    from training import train_fetch as F
    from training import tryon
    from training import patch_routing as P
    from training.dataset import EraseRecord, collate_train
    records = RECORDS[:6]
    host = lambda pin: collate_train([train_set.unrouted(i % 4, EraseRecord(*rec)) for i, rec in enumerate(records)], pin=pin)
    cpu_feed = F.TrainFeed(train_set, batch_gpu=3, rounds=2, device='cpu')
    want = cpu_feed.feed(host(False))
    gpu_feed = F.TrainFeed(train_set, batch_gpu=3, rounds=2, device='cuda')
    pinned = host(True)
    gpu_feed.feed(pinned)                                      # warm-up: plugin loading
    torch.cuda.synchronize()
    P.traffic_counter, tryon.launch_counter, F.launch_counter = dict(bytes=0, launches=0), dict(row_extent=0, inputs=0, triptych=0), dict(fetch=0)
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = gpu_feed.feed(pinned)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        counts = (P.traffic_counter['launches'], tryon.launch_counter['row_extent'], F.launch_counter['fetch'])
        P.traffic_counter = tryon.launch_counter = F.launch_counter = None
    torch.cuda.synchronize()
    assert counts == (3, 1, 1)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert set(g) == set(w) == set(F.KEYS) | {'gen_z'}
        for k in F.KEYS:
            assert g[k].device.type == 'cuda' and g[k].shape == w[k].shape
            assert torch.equal(_bits(g[k].cpu()), _bits(w[k])), k
    assert float(got[0]['denorm_upper_mask'].sum()) > 1000 and float(got[0]['denorm_lower_mask'].sum()) > 1000


def test_training_loop_trains_snapshots_and_resumes(train_set, tmp_path):
    """The driver on the synthetic directory: narrow networks, batch 2, three iterations -> finite losses in stats.jsonl, cur_nimg == 6, a
    snapshot; a second run resumed from it starts from the saved weights."""
    import json
    import os
    from training import training_loop as T
    width = dict(channel_base=4096, channel_max=512)
    kw = dict(batch=2, batch_gpu=2, seed=3, workers=2, tick=0.004, snap=1, device='cuda', width=width, dataset_kwargs=dict(shuffle=False))
    run = str(tmp_path / 'run')
    step = T.training_loop(run, train_set.path, kimg=0.006, **kw)
    assert step.cur_nimg == 6 and step.batch_idx == 3
    with open(os.path.join(run, 'stats.jsonl')) as f:
        lines = [json.loads(line) for line in f]
    assert lines and lines[-1]['Progress/kimg'] == 0.006
    losses = {k: v for line in lines for k, v in line.items() if k.startswith('Loss/')}
    assert {'Loss/G/loss', 'Loss/G/L1', 'Loss/G/mask_loss', 'Loss/D/real', 'Loss/D_parsing/real'} <= set(losses), sorted(losses)
    assert all(np.isfinite(v) for v in losses.values())
    snaps = sorted(f for f in os.listdir(run) if f.startswith('network-snapshot-'))
    assert snaps
    saved = torch.load(os.path.join(run, snaps[-1]), map_location='cpu', weights_only=True)
    assert set(saved) == {'G', 'D', 'D_parsing', 'G_ema', 'augment_p', 'cur_nimg'} and saved['cur_nimg'] == 6
    assert any(k.startswith('synthesis.') for k in saved['G']) and any(k.startswith('mapping.') for k in saved['G_ema'])
    seen = {}

    def on_start(G, D, D_parsing, G_ema):
        seen.update(G=G.state_dict(), D=D.state_dict(), D_parsing=D_parsing.state_dict(), G_ema=G_ema.state_dict())
        seen.update({k: {n: t.detach().cpu().clone() for n, t in v.items()} for k, v in seen.items()})
    step2 = T.training_loop(str(tmp_path / 'run2'), train_set.path, kimg=0.007, resume=os.path.join(run, snaps[-1]), on_start=on_start, **kw)
    for key in ('G', 'D', 'D_parsing', 'G_ema'):
        assert set(seen[key]) == set(saved[key])
        assert all(torch.equal(seen[key][n], saved[key][n]) for n in saved[key]), key
    assert step2.cur_nimg == 8
    with pytest.raises(NotImplementedError):
        T.training_loop(str(tmp_path / 'run3'), train_set.path, kimg=0.002, vgg_weight=50, **kw)
