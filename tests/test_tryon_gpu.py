"""The try-on driver's kernels on the MI355X (csrc/tryon.hip): pg_tryon_inputs against ``to_generator_inputs`` on the GPU bit for bit,
pg_tryon_row_extent_u8 against the loader's ``_bbox``, the batched GPU route against the CPU per-sample loader, pg_tryon_triptych_u8 against the
test.py restatement, a GPU end-to-end run against the CPU one, and a batch with no host sync and one launch of each kernel."""

import os

import numpy as np
import pytest
import torch

from test_tryon_cpu import PARTS, _small_generator, _test_py_triptych, crafted_triptych_case, pairs_root  # noqa: F401

PIL = pytest.importorskip('PIL.Image')

pytestmark = pytest.mark.gpu


def test_torch_divides_by_the_rounded_reciprocal_on_the_gpu():
    """What every kernel here restates: torch's ``u / 127.5 - 1`` on a GPU is ``u * (1.0f / 127.5f) - 1``, for all 256 byte values."""
    u = torch.arange(256, dtype=torch.uint8)
    got = (u.cuda().to(torch.float32) / 127.5 - 1).cpu().numpy()
    want = np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(127.5)) - np.float32(1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _random_batch(n, part, seed):
    """A collate_unrouted-shaped batch on the GPU with random bytes (0 and 255 included), a NaN skin median, labels 0 / 1 / 2, arbitrary bound rows,
    plus routed-shaped tensors; sample 0's first image row holds every byte value, one canvas is empty."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    rb = lambda *s: torch.randint(0, 256, s, generator=g, device='cuda', dtype=torch.int32).to(torch.uint8)
    sparse = lambda t: t * (rb(*t.shape[:-1], 1) < 90)                      # zero pixels: the masks vary
    image, pose, clothes = rb(n, 512, 512, 3), rb(n, 512, 512, 3), rb(n, 512, 512, 3)
    image[0, 0, :256] = torch.arange(256, device='cuda', dtype=torch.uint8)[:, None]
    retain = rb(n, 512, 512, 1)
    retain[:, 100:] = (retain[:, 100:] > 128).to(torch.uint8)             # 0 / 1 below row 100, any byte above
    skin = (torch.randint(0, 512, (n, 3), generator=g, device='cuda').to(torch.float32) / 2)
    skin[0, 1] = float('nan')
    label = torch.arange(n, device='cuda', dtype=torch.int32) % 3
    bound = rb(n, 512)
    canvas = sparse(rb(n, 512, 512, 3))
    den_up, wo_sleeve, den_lo = sparse(rb(n, 512, 512, 3)), sparse(rb(n, 512, 512, 3)), sparse(rb(n, 512, 512, 3))
    wo_sleeve[:, :37] = 0
    wo_sleeve[:, 400:] = 0
    den_lo[:, :213] = 0
    if n > 1:
        wo_sleeve[1] = 0
        den_lo[1] = 0
    norm_img, norm_lower = rb(n, 128, 128, 30), rb(n, 128, 128, 15)
    batch = dict(image=image, clothes=clothes, pose=pose, retain_mask=retain, skin=skin, label=label, bound=bound, canvas=None if part == 'full' else canvas)
    routed = (norm_img, norm_lower, den_up, wo_sleeve, den_lo) if part == 'upper' else (norm_img, norm_lower, den_up, den_lo)
    return batch, routed


@pytest.mark.parametrize('n', [1, 3, 16])
@pytest.mark.parametrize('part', PARTS)
def test_inputs_kernel_equals_to_generator_inputs(part, n):
    from training import tryon
    from training.dataset import to_generator_inputs
    batch, routed = _random_batch(n, part, 7 + n)
    ext = tryon.row_extents(tryon._canvases(batch, routed, part)[2])
    got = tryon.batch_inputs(batch, routed, ext, part)
    want = to_generator_inputs(tryon.loader_tuple(batch, routed, ext, part), 'cuda')
    assert list(got) == list(want)
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a.view(torch.int32) if a.numel() else a, b.view(torch.int32) if b.numel() else b), (part, n, k)   # NaN included
    assert torch.isnan(got['retain'][0, 4]).all() and not torch.isnan(got['retain'][0, 3]).any()


def test_row_extent_kernel_matches_bbox():
    from training import tryon
    from training.dataset import _bbox
    c = np.zeros((7, 512, 512, 3), np.uint8)
    c[1, 0, 0, 0] = 1                       # a single pixel in row 0
    c[2, 511, 511, 2] = 255                 # ... in row 511
    c[3, 0, 300, 1] = 7
    c[3, 511, 2, 0] = 7
    c[4, 200:260, 17:400] = 3
    c[5] = 255
    c[6, 77, 5, 2] = 1
    got = tryon.row_extents(torch.from_numpy(c).cuda()).cpu()
    for i in range(7):
        bb = _bbox((c[i].sum(axis=2, keepdims=True) > 0).astype(np.uint8))
        assert got[i].tolist() == ([-1, -1] if bb is None else [bb[1], bb[3]]), i


@pytest.mark.parametrize('part', PARTS)
def test_batched_gpu_route_equals_the_cpu_loader(pairs_root, part):
    from training.dataset import TryOnTestSet, collate_unrouted, to_generator_inputs
    from training import tryon
    ds = TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu', part=part)
    idx = list(range(len(ds)))
    want = to_generator_inputs(torch.utils.data.default_collate([ds[i] for i in idx]), 'cuda')
    batch = tryon.upload(collate_unrouted([ds.unrouted(i) for i in idx], pin=True), 'cuda')
    routed, ext = tryon.route(batch, part)
    got = tryon.batch_inputs(batch, routed, ext, part)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (part, k)


def test_triptych_kernel_equals_test_py():
    from training import tryon
    fin, clothes, image = crafted_triptych_case()
    with np.errstate(invalid='ignore'):
        want = _test_py_triptych(fin, clothes, image)
    got = tryon.triptych(torch.from_numpy(fin).cuda(), torch.from_numpy(clothes).cuda(), torch.from_numpy(image).cuda()).cpu().numpy()
    assert got.shape == (2, 512, 960, 3) and np.array_equal(got, want)
    # a real generator output
    torch.manual_seed(0)
    G = _small_generator().cuda()
    batch, routed = _random_batch(2, 'full', 3)
    routed = tuple(routed)
    ext = tryon.row_extents(routed[3])
    with torch.no_grad():
        _, fin, _ = G(**tryon.batch_inputs(batch, routed, ext, 'full'), noise_mode='const')
    got = tryon.triptych(fin, batch['clothes'], batch['image']).cpu().numpy()
    want = _test_py_triptych(fin.cpu().numpy(), batch['clothes'].cpu().numpy(), batch['image'].cpu().numpy())
    assert np.array_equal(got, want)


def test_gpu_end_to_end_against_the_cpu_run(pairs_root, tmp_path):
    from training.dataset import TryOnTestSet
    from training import tryon
    G = _small_generator()
    outs = {}
    for dev in ('cpu', 'cuda'):
        ds = TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu', part='upper')
        outs[dev] = tryon.run_tryon(ds, G.to(dev), str(tmp_path / dev), batch_size=2, device=dev, workers=0 if dev == 'cpu' else 2)
    assert [os.path.basename(f) for f in outs['cpu']] == [os.path.basename(f) for f in outs['cuda']]
    for a, b in zip(outs['cpu'], outs['cuda']):
        x, y = np.array(PIL.open(a)).astype(int), np.array(PIL.open(b)).astype(int)
        assert np.array_equal(x[:, :640], y[:, :640]), b                     # clothes and person: identical
        d = np.abs(x[:, 640:] - y[:, 640:])
        assert d.max() <= 1 and (d > 0).mean() <= 0.01, (b, d.max(), (d > 0).mean())


@pytest.mark.parametrize('part', PARTS)
def test_a_batch_runs_without_a_host_sync(pairs_root, part):
    from training.dataset import TryOnTestSet, collate_unrouted
    from training import tryon
    ds = TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu', part=part)
    host_batch = collate_unrouted([ds.unrouted(i) for i in range(len(ds))], pin=True)
    G = _small_generator().cuda()
    want = tryon.tryon_batch(tryon.upload(host_batch, 'cuda'), G, part).cpu()          # warm-up (one-time host-side caches of the network)
    torch.cuda.synchronize()
    tryon.launch_counter = dict(row_extent=0, inputs=0, triptych=0)
    host = torch.empty(want.shape, dtype=torch.uint8, pin_memory=True)
    torch.cuda.set_sync_debug_mode('error')
    try:
        trip = tryon.tryon_batch(tryon.upload(host_batch, 'cuda'), G, part)
        host.copy_(trip, non_blocking=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        counts = tryon.launch_counter
        tryon.launch_counter = None
    torch.cuda.synchronize()
    assert counts == dict(row_extent=1, inputs=1, triptych=1)
    assert torch.equal(host, want)
