"""The native front half of the try-on loader on the MI355X (csrc/tryon_front.hip through training/tryon_front.py): every map of
``collate_unrouted`` rebuilt on the device from a ``collate_raw`` batch, against the loader's own host code -- equality on every byte and on the
float32 skin (NaN positions equal), no tolerance.  The crafted people come from tests/test_tryon_front_cpu.py."""

import ctypes

import pytest
import torch

from test_tryon_cpu import PARTS, _small_generator, pairs_root  # noqa: F401
from test_tryon_front_cpu import assert_same_batch, crafted_root, write_narrow  # noqa: F401

PIL = pytest.importorskip('PIL.Image')

pytestmark = pytest.mark.gpu


def _both(root, part, sleeve=True):
    """(the uploaded raw batch, the uploaded host batch) of every pair under `root`."""
    from training.dataset import TryOnTestSet, collate_raw, collate_unrouted
    from training import tryon
    ds = TryOnTestSet(root, use_sleeve_mask=sleeve, device='cpu', part=part)
    idx = range(len(ds))
    return (tryon.upload(collate_raw([ds.raw(i) for i in idx], pin=True), 'cuda'),
            tryon.upload(collate_unrouted([ds.unrouted(i) for i in idx], pin=True), 'cuda'))


@pytest.mark.parametrize('sleeve', [False, True])
@pytest.mark.parametrize('part', PARTS)
def test_native_front_equals_the_host_loader(pairs_root, part, sleeve):
    from training import tryon_front
    raw, want = _both(pairs_root, part, sleeve)
    assert_same_batch(tryon_front.front_batch(raw, part), want, (part, sleeve))
    one = {k: (v[:1] if isinstance(v, (torch.Tensor, list)) else v) for k, v in raw.items()}              # N = 1
    assert_same_batch(tryon_front.front_batch(one, part), {k: (v[:1] if isinstance(v, (torch.Tensor, list)) else v) for k, v in want.items()},
                      (part, sleeve, 'n=1'))


@pytest.mark.parametrize('part', PARTS)
def test_native_front_on_the_crafted_people(crafted_root, part):
    """Equal pants and skirt, the four dress branches, no lower garment, garments on the image's edges, empty skin, a .5 median, a missing elbow,
    a negative hip row, ``people: []``, a limb of zero length, key points outside the frame: each as the person of one pair and the clothes of the next."""
    from training import tryon_front
    raw, want = _both(crafted_root, part)
    assert_same_batch(tryon_front.front_batch(raw, part), want, part)


@pytest.mark.parametrize('part', PARTS)
def test_native_front_on_a_narrow_image(tmp_path, part):
    """W = 318, left = 97: the byte-wise source loads, and quads of pixels that straddle the image's edges."""
    from training import tryon_front
    write_narrow(str(tmp_path))
    raw, want = _both(str(tmp_path), part)
    assert tuple(raw['person_img'].shape) == (2, 512, 318, 3)
    assert_same_batch(tryon_front.front_batch(raw, part), want, part)


@pytest.mark.parametrize('part', PARTS)
def test_tryon_batch_from_the_native_front_equals_the_host_front(pairs_root, part):
    from training import tryon, tryon_front
    raw, host = _both(pairs_root, part)
    G = _small_generator().cuda()
    want = tryon.tryon_batch(host, G, part)
    got = tryon.tryon_batch(tryon_front.front_batch(raw, part), G, part)
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize('part', PARTS)
def test_a_native_front_batch_is_three_launches_and_no_host_sync(pairs_root, part):
    from training import tryon, tryon_front
    raw, host = _both(pairs_root, part)
    G = _small_generator().cuda()
    want = tryon.tryon_batch(tryon_front.front_batch(raw, part), G, part).cpu()          # warm-up (plugins loaded, the network's host-side caches)
    torch.cuda.synchronize()
    tryon_front.launch_counter = dict.fromkeys(tryon_front.LAUNCHES, 0)
    pinned = torch.empty(want.shape, dtype=torch.uint8, pin_memory=True)
    torch.cuda.set_sync_debug_mode('error')
    try:
        trip = tryon.tryon_batch(tryon_front.front_batch(raw, part), G, part)
        pinned.copy_(trip, non_blocking=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        counts = tryon_front.launch_counter
        tryon_front.launch_counter = None
    torch.cuda.synchronize()
    assert counts == dict(stats=1, bit_rows=1, compose=1) and sum(counts.values()) <= 4
    assert torch.equal(pinned, want)


def test_the_entry_points_reject_what_they_cannot_read(pairs_root):
    from torch_utils.ops._native import NativeOpError
    from training import tryon_front
    raw, _ = _both(pairs_root, 'upper')
    bad = dict(raw, person_parsing=raw['person_parsing'].to(torch.int32))
    with pytest.raises(NativeOpError, match='person_parsing'):
        tryon_front.front_batch(bad, 'upper')
    bad = dict(raw, clothes_img=raw['clothes_img'].transpose(1, 2).contiguous().transpose(1, 2))       # same shape, other strides
    assert not bad['clothes_img'].is_contiguous()
    with pytest.raises(NativeOpError, match='clothes_img'):
        tryon_front.front_batch(bad, 'upper')
    bad = dict(raw, bands=raw['bands'].to(torch.float32))
    with pytest.raises(NativeOpError, match='bands'):
        tryon_front.front_batch(bad, 'upper')
    # the C ABI itself: argument errors come back as PG_ERRORS codes, before anything is launched
    lib = tryon_front._init().lib
    io = tryon_front.FrontIO()
    assert lib.pg_tryon_front_stats(ctypes.byref(io), 1, 512, 320, None) == -1                               # NULL pointers
    assert lib.pg_tryon_front_bit_rows(ctypes.byref(io), 1, 512, 320, 96, 0, None) == -1
    assert lib.pg_tryon_front_compose(ctypes.byref(io), 1, 512, 320, 96, 0, None) == -1
    p = lambda k: raw[k].data_ptr()
    stats = torch.zeros([3, tryon_front.STATS], dtype=torch.int32, device='cuda')
    io = tryon_front.FrontIO(person_img=p('person_img'), clothes_img=p('clothes_img'), person_parsing=p('person_parsing'),
                             clothes_parsing=p('clothes_parsing'), stats=stats.data_ptr())
    assert lib.pg_tryon_front_stats(ctypes.byref(io), 3, 510, 320, None) == -2                               # H % 4 != 0
    assert lib.pg_tryon_front_stats(ctypes.byref(io), 0, 512, 320, None) == -1
    assert lib.pg_tryon_front_bit_rows(ctypes.byref(io), 3, 512, 320, 200, 0, None) == -1                    # left + W > H
    assert lib.pg_tryon_front_bit_rows(ctypes.byref(io), 3, 512, 320, 96, 7, None) == -1                     # no such mode
    torch.cuda.synchronize()
    assert not stats.any()                                                                                   # nothing ran
