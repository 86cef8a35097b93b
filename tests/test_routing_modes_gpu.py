"""The lower-garment and full-outfit try-on modes on the MI355X: the erode-window parameter of the two paste kernels through the C ABI
(pg_patch_compose_u8_k, pg_patch_compose_ordered_u8_k) against the oracle's erode + paste, bit for bit; ``normalize(part=...)`` and
``normalize_batch(part=...)`` on the GPU against the test-side restatement (tests/routing_modes_ref.py) and each other; a batch of 16 routed
without a host sync in three launches; one routed 'full' batch through GeneratorFull_v20."""

import ctypes

import numpy as np
import pytest
import torch

from test_routing_modes import CASES, routing_case

pytestmark = pytest.mark.gpu


def _lib():
    from training import patch_routing as P
    return P._init().lib


def _compose_k(patch, mask, canvas, canvas2, ksize):
    lib = _lib()
    h, w = canvas.shape[:2]
    st = lib.pg_patch_compose_u8_k(patch.data_ptr(), mask.data_ptr(), canvas.data_ptr(), canvas2.data_ptr() if canvas2 is not None else None,
                                   h, w, mask.shape[2], ksize, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def _images(seed, h=96, w=120):
    rng = np.random.default_rng(seed)
    patch = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    canvas = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = (rng.random((h, w, 3)) > 0.01).astype(np.uint8) * 255
    mask[:, :, 0][rng.random((h, w)) > 0.997] = 254                  # near-white is not white
    return patch, canvas, mask


@pytest.mark.parametrize('ksize', [1, 3, 5, 7, 8, 16])
def test_compose_k_matches_erode_and_paste(ksize):
    from oracle import patch_routing_ref as R
    patch, canvas, mask = _images(ksize)
    m = (R.erode_u8(mask[..., 0], ksize)[..., None] == 255).astype(np.uint8)
    c1, c2 = torch.from_numpy(canvas).cuda(), torch.zeros(canvas.shape, dtype=torch.uint8, device='cuda')
    assert _compose_k(torch.from_numpy(patch).cuda(), torch.from_numpy(mask).cuda(), c1, c2, ksize) == 0
    assert np.array_equal(c1.cpu().numpy(), patch * m + canvas * (1 - m))
    assert np.array_equal(c2.cpu().numpy(), patch * m)
    assert 0.02 < m.mean() < 0.99


def test_compose_k8_equals_the_old_entry_and_bad_windows_are_refused():
    lib = _lib()
    patch, canvas, mask = (torch.from_numpy(a).cuda() for a in _images(8))
    a, b = canvas.clone(), canvas.clone()
    a2, b2 = torch.zeros_like(canvas), torch.zeros_like(canvas)
    assert _compose_k(patch, mask, a, a2, 8) == 0
    h, w = canvas.shape[:2]
    assert lib.pg_patch_compose_u8(patch.data_ptr(), mask.data_ptr(), b.data_ptr(), b2.data_ptr(), h, w, 3, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a2, b2)
    before = canvas.clone()
    for k in (0, -1, 17, 64):
        assert _compose_k(patch, mask, canvas, None, k) == -1, k                # refused before any launch: the canvas is untouched
        assert lib.pg_patch_compose_ordered_u8_k(ctypes.c_void_p(canvas.data_ptr()), 1, h, w, 3, k, None) == -1, k
    assert torch.equal(canvas, before)


def _ordered_table(jobs):
    """jobs: list of (canvas, canvas2 | None, [(patch, mask, to_canvas2)]) -> the pg_compose_job table in device memory."""
    from training import patch_routing as P
    t = np.zeros(len(jobs), dtype=P._COMPOSE_DT)
    for j, (canvas, canvas2, parts) in enumerate(jobs):
        t[j]['canvas'], t[j]['canvas2'], t[j]['nparts'] = canvas.data_ptr(), canvas2.data_ptr() if canvas2 is not None else 0, len(parts)
        for k, (p, m, c2) in enumerate(parts):
            t[j]['patch'][k], t[j]['mask'][k], t[j]['to_canvas2'][k] = p.data_ptr(), m.data_ptr(), c2
    return torch.from_numpy(t.view(np.uint8).reshape(-1)).cuda()


@pytest.mark.parametrize('ksize', [3, 5, 7, 8])
def test_ordered_compose_k_matches_the_paste_sequence(ksize):
    """Three canvases of up to four parts each (one with a second canvas that skips some parts, one with no parts): the oracle's erode + paste in
    part order on zero canvases, bit for bit; for ksize 8 also the old entry."""
    from oracle import patch_routing_ref as R
    lib = _lib()
    rng = np.random.default_rng(100 + ksize)
    h, w = 80, 72
    specs = [[1, 0, 1, 1], [0, 1], []]                                  # to_canvas2 flags per part
    jobs, want = [], []
    for j, flags in enumerate(specs):
        parts, c, c2 = [], np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)
        for flag in flags:
            p = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            m = np.zeros((h, w, 3), np.uint8)
            y0, x0 = rng.integers(0, h // 2), rng.integers(0, w // 2)
            m[y0:y0 + rng.integers(8, h // 2), x0:x0 + rng.integers(8, w // 2)] = 255
            m[:, :, 0][rng.random((h, w)) > 0.998] = 0
            e = (R.erode_u8(m[..., 0], ksize)[..., None] == 255).astype(np.uint8)
            c = p * e + c * (1 - e)
            if flag:
                c2 = p * e + c2 * (1 - e)
            parts.append((torch.from_numpy(p).cuda(), torch.from_numpy(m).cuda(), flag))
        canvas = torch.full((h, w, 3), 7, dtype=torch.uint8, device='cuda')       # every pixel is written
        canvas2 = torch.full((h, w, 3), 7, dtype=torch.uint8, device='cuda') if j == 0 else None
        jobs.append((canvas, canvas2, parts))
        want.append((c, c2 if j == 0 else None))
    tab = _ordered_table(jobs)
    assert lib.pg_patch_compose_ordered_u8_k(tab.data_ptr(), len(jobs), h, w, 3, ksize, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = [(c.clone(), c2.clone() if c2 is not None else None) for c, c2, _ in jobs]
    for (g, g2), (c, c2) in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), c)
        if c2 is not None:
            assert np.array_equal(g2.cpu().numpy(), c2)
    if ksize == 8:
        assert lib.pg_patch_compose_ordered_u8(tab.data_ptr(), len(jobs), h, w, 3, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        for (c, c2, _), (g, g2) in zip(jobs, got):
            assert torch.equal(c, g) and (c2 is None or torch.equal(c2, g2))


@pytest.mark.parametrize('part', ['lower', 'full'])
def test_normalize_and_batch_match_the_restatement_per_sample(part):
    import routing_modes_ref as MR
    from training import patch_routing as P
    cases = list(CASES) + ['all_joints']
    samples = [routing_case(case, 40 + i) for i, case in enumerate(cases)]
    P.traffic_counter = dict(bytes=0, launches=0)
    try:
        got = P.normalize_batch(samples, 2, part=part)
        launches = P.traffic_counter['launches']
    finally:
        P.traffic_counter = None
    assert launches == 3 and len(got) == 4
    names = ('norm_img', 'norm_img_lower', 'denorm_upper_img', 'denorm_lower_img')
    for i, s in enumerate(samples):
        want = MR.normalize(part, *s, 2)
        own = P.normalize(*s, 2, part=part)
        assert len(own) == 4
        for nm, g, w_, o in zip(names, got, want, own):
            assert g.device.type == 'cuda' and g.dtype == torch.uint8 and tuple(g[i].shape) == w_.shape, (cases[i], nm)
            assert np.array_equal(o.cpu().numpy(), w_), (cases[i], nm, 'normalize')
            assert torch.equal(g[i], o), (cases[i], nm, 'normalize_batch')


@pytest.mark.parametrize('part', ['upper', 'lower', 'full'])
def test_batch_of_16_routes_without_a_host_sync(part):
    from training import patch_routing as P
    samples = []
    for i in range(16):
        up, lo, um, lm, sleeve, ckp, pkp = routing_case(['all_joints', 'no_left_arm_with_sleeve_mask', 'missing_knees_and_nose'][i % 3], 200 + i)
        gpu = lambda a: torch.from_numpy(a).cuda() if a is not None else None
        samples.append((gpu(up), gpu(lo), gpu(um), gpu(lm), gpu(sleeve), ckp, pkp))
    torch.cuda.synchronize()
    want = P.normalize_batch(samples, 2, part=part)
    P.traffic_counter = dict(bytes=0, launches=0)
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = P.normalize_batch(samples, 2, part=part)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        launches = P.traffic_counter['launches']
        P.traffic_counter = None
    assert launches == 3 and len(got) == (5 if part == 'upper' else 4)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert int(got[3 if part != 'upper' else 4].sum()) > 0


def test_routed_full_batch_through_the_generator():
    from training import networks as PN
    from training import patch_routing as P
    from detgen import fill_module_
    n = 4
    samples = [routing_case('all_joints', 300 + i) for i in range(n)]
    norm_img, norm_lower, den_up, den_lo = P.normalize_batch(samples, 2, part='full')
    unit = lambda t: t.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1
    mask = lambda t: (t.to(torch.int32).sum(dim=3, keepdim=True) > 0).permute(0, 3, 1, 2).float()
    g = torch.Generator(device='cpu').manual_seed(5)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    inp = dict(z=torch.zeros([n, 0], device='cuda'), c=torch.cat([unit(norm_img), unit(norm_lower)], dim=1), retain=u(n, 6, 512, 512), pose=u(n, 5, 512, 512),
               denorm_upper_input=unit(den_up), denorm_lower_input=unit(den_lo), denorm_upper_mask=mask(den_up), denorm_lower_mask=mask(den_lo))
    assert inp['denorm_lower_mask'].sum() > 1000
    torch.manual_seed(0)
    G = fill_module_(PN.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                          synthesis_kwargs=dict(channel_base=32768, channel_max=512, conv_clamp=256)), 'cfg3.').cuda().eval()
    with torch.no_grad():
        img, finetune_img, pred_parsing = G(**inp, noise_mode='const')
    assert img.shape == finetune_img.shape == (n, 3, 512, 512) and pred_parsing.shape == (n, 7, 512, 512)
    assert all(torch.isfinite(t).all() for t in (img, finetune_img, pred_parsing))
