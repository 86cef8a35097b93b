"""The mixed-outfit try-on mode (``part='outfit'``) on the MI355X: the batched routing with a second set of key points, the native front with a second
clothes source (csrc/tryon_front.hip), the four-panel packer (pg_tryon_panels_u8, csrc/tryon.hip) and the driver.  Every comparison is equality: against
the CPU route, against the host loader, and against the ``full`` mode through the two identities tests/test_outfit_cpu.py states."""

import ctypes
import os

import numpy as np
import pytest
import torch

from test_outfit_cpu import dataset, sample, same
from test_tryon_cpu import _small_generator, crafted_triptych_case, pairs_root  # noqa: F401
from test_tryon_front_cpu import CRAFTED, J, assert_same_batch, crafted_root, write_narrow  # noqa: F401

PIL = pytest.importorskip('PIL.Image')

pytestmark = pytest.mark.gpu

MIXED = ['person_b.jpg person_b.jpg person_a.jpg', 'dress_c.jpg person_a.jpg person_b.jpg', 'person_a.jpg person_b.jpg dress_c.jpg']


def _both(ds, idx=None):
    """(the uploaded raw batch, the uploaded host batch) of the pairs `idx` (default: all) of `ds`."""
    from training.dataset import collate_raw, collate_unrouted
    from training import tryon
    idx = range(len(ds)) if idx is None else idx
    return (tryon.upload(collate_raw([ds.raw(i) for i in idx], pin=True), 'cuda'),
            tryon.upload(collate_unrouted([ds.unrouted(i) for i in idx], pin=True), 'cuda'))


# --------------------------------------------------------------------------------------------------- routing

@pytest.fixture(scope='module')
def routing_case(pairs_root):
    """Four samples and their per-sample CPU routing (computed once): U = L; U != L; U != L with lower key points that lose the left hip (confidence
    0.05: the torso and the left thigh of the lower garment have no crop, whatever the clothes' key points say); U != L without a sleeve mask."""
    from training import patch_routing as P
    ds = dataset(pairs_root, MIXED + ['person_a.jpg person_b.jpg dress_c.jpg'], 'outfit', sleeve=True)
    samples = [sample(ds.unrouted(i)) for i in range(4)]
    lost = samples[2][7].copy()
    lost[J['lhip'], 2] = 0.05
    samples[2] = samples[2][:7] + (lost,)
    samples[3] = samples[3][:4] + (None,) + samples[3][5:]
    want = [P.normalize(*s[:7], 2, 'cpu', part='outfit', lower_keypoints=s[7]) for s in samples]
    assert not want[2][1][..., 0:6].any() and want[1][1][..., 0:6].any()                   # lower parts 0 and 6 are gone in sample 2 only
    return samples, want


@pytest.mark.parametrize('idx', [[1], [0, 1, 2, 3]])
def test_batched_outfit_routing_equals_the_cpu_route(routing_case, idx):
    from training import patch_routing as P
    samples, want = routing_case
    P.traffic_counter = dict(bytes=0, launches=0)
    try:
        got = P.normalize_batch([samples[i] for i in idx], 2, 'cuda', part='outfit')
    finally:
        counts, P.traffic_counter = P.traffic_counter, None
    assert counts['launches'] == 3
    assert len(got) == 4
    for k in range(4):
        assert got[k].shape[0] == len(idx) and got[k].dtype == torch.uint8
        for j, i in enumerate(idx):
            assert torch.equal(got[k][j].cpu(), want[i][k]), (idx, i, k)
    seven = P.normalize_batch([samples[i][:7] for i in idx], 2, 'cuda', part='outfit')     # a 7-tuple routes as full
    full = P.normalize_batch([samples[i][:7] for i in idx], 2, 'cuda', part='full')
    assert all(torch.equal(a, b) for a, b in zip(seven, full))


# --------------------------------------------------------------------------------------------------- the native front

def _crafted_lines():
    names = [n + '.jpg' for n, _ in CRAFTED] + ['nobody.jpg', 'base.jpg', 'median.png']
    return [f'{names[i]} {names[i - 1]} {names[(i + 1) % len(names)]}' for i in range(len(names))]      # each: U of one line, L of the next


@pytest.mark.parametrize('sleeve', [False, True])
@pytest.mark.parametrize('which', ['pairs', 'crafted', 'narrow'])
def test_native_outfit_front_equals_the_host_loader(pairs_root, crafted_root, tmp_path, which, sleeve):
    from training import tryon_front
    if which == 'narrow':                                                  # W = 318, left = 97: the byte-wise loads of the third source too
        root, lines = str(tmp_path), ['narrow_b.jpg narrow_a.jpg narrow_a.jpg', 'narrow_a.jpg narrow_b.jpg narrow_b.jpg', 'narrow_a.jpg narrow_a.jpg narrow_b.jpg']
        write_narrow(root)
    else:
        root, lines = (pairs_root, MIXED) if which == 'pairs' else (crafted_root, _crafted_lines())
    raw, want = _both(dataset(root, lines, 'outfit', sleeve))
    assert raw['lower_img'].shape[2] == (318 if which == 'narrow' else 320)
    assert_same_batch(tryon_front.front_batch(raw, 'outfit'), want, (which, sleeve))
    if which == 'pairs':
        first = lambda b: {k: (v[1:2] if isinstance(v, (torch.Tensor, list)) else v) for k, v in b.items()}      # N = 1, a U != L line
        assert_same_batch(tryon_front.front_batch(first(raw), 'outfit'), first(want), (which, sleeve, 'n=1'))


# --------------------------------------------------------------------------------------------------- a whole batch

def test_outfit_batches_from_both_fronts_and_against_full(pairs_root):
    from training import tryon, tryon_front
    G = _small_generator().cuda()
    raw, host = _both(dataset(pairs_root, MIXED, 'outfit', sleeve=True))
    want = tryon.tryon_batch(host, G, 'outfit')
    got = tryon.tryon_batch(tryon_front.front_batch(raw, 'outfit'), G, 'outfit')
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 512, 1280, 3) and torch.equal(got, want)
    garments = tryon.triptych(torch.zeros(3, 3, 512, 512, device='cuda'), host['clothes'], host['lower_clothes'])
    assert torch.equal(got[:, :, 0:640], garments[:, :, 0:640])             # upper clothes | lower clothes, with the triptych's source arithmetic
    # U U P lines: person | result are the full mode's, and both garment panels its clothes panel
    raw, _ = _both(dataset(pairs_root, ['person_b.jpg person_b.jpg person_a.jpg', 'dress_c.jpg dress_c.jpg person_b.jpg'], 'outfit', sleeve=True))
    _, full = _both(dataset(pairs_root, ['person_b.jpg person_a.jpg', 'dress_c.jpg person_b.jpg'], 'full', sleeve=True))
    got = tryon.tryon_batch(tryon_front.front_batch(raw, 'outfit'), G, 'outfit')
    want = tryon.tryon_batch(full, G, 'full')
    assert torch.equal(got[:, :, 640:], want[:, :, 320:])
    assert torch.equal(got[:, :, 0:320], want[:, :, 0:320]) and torch.equal(got[:, :, 320:640], want[:, :, 0:320])


def test_an_outfit_batch_is_the_same_launches_and_no_host_sync(pairs_root):
    from training import patch_routing as P
    from training import tryon, tryon_front
    raw, _ = _both(dataset(pairs_root, MIXED, 'outfit', sleeve=True))
    G = _small_generator().cuda()
    want = tryon.tryon_batch(tryon_front.front_batch(raw, 'outfit'), G, 'outfit').cpu()    # warm-up (plugins loaded, the network's host-side caches)
    torch.cuda.synchronize()
    tryon_front.launch_counter = dict.fromkeys(tryon_front.LAUNCHES, 0)
    tryon.launch_counter = dict(row_extent=0, inputs=0, triptych=0, panels=0)
    P.traffic_counter = dict(bytes=0, launches=0)
    pinned = torch.empty(want.shape, dtype=torch.uint8, pin_memory=True)
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = tryon.tryon_batch(tryon_front.front_batch(raw, 'outfit'), G, 'outfit')
        pinned.copy_(out, non_blocking=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        front, staging, routing = tryon_front.launch_counter, tryon.launch_counter, P.traffic_counter
        tryon_front.launch_counter = tryon.launch_counter = P.traffic_counter = None
    torch.cuda.synchronize()
    assert front == dict(stats=1, bit_rows=1, compose=1)
    assert routing['launches'] == 3
    assert staging == dict(row_extent=1, inputs=1, triptych=0, panels=1)
    assert torch.equal(pinned, want)


# --------------------------------------------------------------------------------------------------- the panel kernel

def test_panels_kernel_equals_the_numpy_panels(monkeypatch):
    from training import tryon
    fin, clothes, image = crafted_triptych_case()
    lower = np.ascontiguousarray(clothes[::-1, :, ::-1])
    with np.errstate(invalid='ignore'):
        want = tryon.panels_numpy(fin, [clothes, lower, image])
    cuda = lambda a: torch.from_numpy(a).cuda()
    got = tryon.panels(cuda(fin), [cuda(clothes), cuda(lower), cuda(image)])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 512, 1280, 3) and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got[:, :, 0:320], tryon.triptych(cuda(fin), cuda(clothes), cuda(image))[:, :, 0:320])
    # a toy size: n = 2, H = 8, W = 16, x0 = 4, cw = 8 (one workgroup, rows shorter than a wavefront)
    monkeypatch.setattr(tryon, 'X0', 4)
    monkeypatch.setattr(tryon, 'CW', 8)
    rng = np.random.default_rng(5)
    fin = rng.uniform(-1.2, 1.2, (2, 3, 8, 16)).astype(np.float32)
    fin[1, 2, 7, 4:8] = [np.nan, np.inf, -np.inf, 1.0]
    srcs = [rng.integers(0, 256, (2, 8, 16, 3), dtype=np.uint8) for _ in range(3)]
    with np.errstate(invalid='ignore'):
        want = tryon.panels_numpy(fin, srcs)
    got = tryon.panels(cuda(fin), [cuda(s) for s in srcs])
    assert tuple(got.shape) == (2, 8, 32, 3) and np.array_equal(got.cpu().numpy(), want)


# --------------------------------------------------------------------------------------------------- the C ABI's argument checks

def test_the_entry_points_reject_an_outfit_without_its_lower_sources(pairs_root):
    from training import tryon, tryon_front
    raw, _ = _both(dataset(pairs_root, MIXED, 'outfit', sleeve=True))
    lib = tryon_front._init().lib
    plan = tryon_front.plan_batch(raw, 'outfit')
    for t in (plan['out']['image'], plan['out']['lower_clothes'], plan['scratch']['bit_rows']):
        t.fill_(7)
    io, (n, H, W) = plan['io'], plan['dims']
    call = lambda name, mode: getattr(lib, 'pg_tryon_front_' + name)(ctypes.byref(io), n, H, W, plan['left'], mode, None)
    assert call('bit_rows', 7) == -1 and call('compose', 7) == -1                           # no such mode
    keep = (io.lower_src_img, io.lower_src_parsing, io.lower_clothes)
    io.lower_src_img = None
    assert call('bit_rows', 3) == -1 and call('compose', 3) == -1
    io.lower_src_img, io.lower_src_parsing = keep[0], None
    assert call('bit_rows', 3) == -1 and call('compose', 3) == -1
    io.lower_src_parsing, io.lower_clothes = keep[1], None
    assert call('compose', 3) == -1
    io.lower_clothes = keep[2]
    assert call('compose', 2) == -1                                                         # lower_clothes belongs to the outfit mode alone
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (plan['out']['image'], plan['out']['lower_clothes'], plan['scratch']['bit_rows']))     # nothing ran
    # the argument lists from before the outfit mode still bind: the struct filled by keyword leaves the appended fields NULL
    p = lambda k: raw[k].data_ptr()
    stats = torch.zeros([3, tryon_front.STATS], dtype=torch.int32, device='cuda')
    old = tryon_front.FrontIO(person_img=p('person_img'), clothes_img=p('clothes_img'), person_parsing=p('person_parsing'),
                              clothes_parsing=p('clothes_parsing'), stats=stats.data_ptr())
    assert not old.lower_src_img and not old.lower_src_parsing and not old.lower_clothes
    assert lib.pg_tryon_front_stats(ctypes.byref(old), 3, 510, 320, None) == -2
    assert lib.pg_tryon_front_bit_rows(ctypes.byref(old), 3, 512, 320, 96, 7, None) == -1
    assert lib.pg_tryon_front_stats(ctypes.byref(old), 3, 512, 320, None) == 0               # without a lower parsing its four counts stay zero
    torch.cuda.synchronize()
    assert stats[:, :8].any() and not stats[:, 784:].any()
    # the panel packer
    pk = tryon._init().lib.pg_tryon_panels_u8
    fin, out = torch.zeros(1, 3, 8, 16, device='cuda'), torch.zeros(1, 8, 32, 3, dtype=torch.uint8, device='cuda')
    src = torch.zeros(1, 8, 16, 3, dtype=torch.uint8, device='cuda')
    ptrs = (ctypes.c_void_p * 4)(*[src.data_ptr()] * 4)
    assert pk(fin.data_ptr(), ptrs, 0, out.data_ptr(), 1, 8, 16, 4, 8, None) == -1
    assert pk(fin.data_ptr(), ptrs, 4, out.data_ptr(), 1, 8, 16, 4, 8, None) == -1
    assert pk(fin.data_ptr(), ptrs, 3, out.data_ptr(), 1, 8, 16, 12, 8, None) == -1          # x0 + cw > W
    assert pk(fin.data_ptr(), ptrs, 3, out.data_ptr(), 1, 8, 16, 2, 8, None) == -2           # x0 % 4 != 0
    ptrs[1] = None
    assert pk(fin.data_ptr(), ptrs, 3, out.data_ptr(), 1, 8, 16, 4, 8, None) == -1


# --------------------------------------------------------------------------------------------------- the driver

def test_gpu_end_to_end_in_the_outfit_mode(pairs_root, tmp_path):
    from training import tryon
    G = _small_generator().cuda()
    ds = dataset(pairs_root, MIXED[:2], 'outfit', sleeve=True)
    files = {front: tryon.run_tryon(ds, G, str(tmp_path / front), batch_size=2, device='cuda', workers=0, front=front) for front in ('host', 'native')}
    names = ['person_a___person_b___person_b.png', 'person_b___dress_c___person_a.png']
    assert [os.path.basename(f) for f in files['host']] == [os.path.basename(f) for f in files['native']] == names
    for a, b in zip(files['host'], files['native']):
        with open(a, 'rb') as fa, open(b, 'rb') as fb:
            assert fa.read() == fb.read(), b
    assert np.array(PIL.open(files['host'][1])).shape == (512, 1280, 3)
    # 16-bit: a generator whose 512^2 block is 16 channels wide (`set_half` refuses the narrower one above)
    from training import networks as PN
    from detgen import fill_module_
    G = fill_module_(PN.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=64, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                          synthesis_kwargs=dict(channel_base=8192, channel_max=512, conv_clamp=256)), 'outfit.').eval().cuda()
    half = tryon.run_tryon(ds, G, str(tmp_path / 'bf16'), batch_size=2, device='cuda', workers=0, front='native', precision='bf16')
    assert G.synthesis.half_dtype is None
    assert [os.path.basename(f) for f in half] == names and all(os.path.getsize(f) > 0 for f in half)
    assert same(np.array(PIL.open(half[0]))[:, :960], np.array(PIL.open(files['host'][0]))[:, :960])      # the three source panels do not pass the generator
