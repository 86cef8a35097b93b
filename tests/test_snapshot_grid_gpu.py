"""The image snapshots on the GPU: ``pg_patch_denorm_u8`` against the unfused launches it replaces (``pg_warp_perspective_u8`` of every patch and mask,
then ``pg_patch_compose_ordered_u8_k``) byte for byte, ``pg_snapshot_cells_u8`` against the restatement's NumPy arithmetic, `setup_snapshot_grid` on
the GPU against its CPU route on the three-person directory of tests/test_snapshot_grid_cpu.py, and `render` with a narrow generator."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_snapshot_grid_cpu import write_vis_root             # noqa: E402


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------------------- pg_patch_denorm_u8

def part(rng, p, ph, pw, m, dev):
    """Part p: patch values in [20 p + 10, 20 p + 29] (so a canvas pixel tells which part won it), a white mask with two 254 pixels (the erode bites around
    them, and along the warped border), forward matrix m."""
    patch = torch.from_numpy(rng.integers(20 * p + 10, 20 * p + 30, (ph, pw, 3), dtype=np.uint8))
    mask = np.full((ph, pw, 3), 255, dtype=np.uint8)
    for _ in range(2):
        mask[rng.integers(1, ph - 1), rng.integers(1, pw - 1)] = 254
    return patch.to(dev), torch.from_numpy(mask).to(dev), np.array(m, dtype=np.float64)


def make_jobs(rng, H, W, ph, pw, dev):
    """Jobs with 0, 1 and 10 parts; overlapping parts (the order decides); a part reaching past every canvas border under small ones; a strongly
    perspective part next to an affine one.  (CPU-route check when choosing the matrices: every canvas with parts has >= 5 % non-zero pixels, and each
    of the canvases listed in `two` has at least two winning parts.)"""
    sx, sy = W / pw, H / ph
    affine = lambda a, b, tx, ty, sh=0.0: [[a, sh, tx], [-sh, b, ty], [0, 0, 1]]
    jobs = [[],
            [part(rng, 0, ph, pw, affine(0.6 * sx, 0.7 * sy, 0.1 * W, 0.1 * H, 0.05), dev)],
            [part(rng, p, ph, pw, affine(0.45 * sx, 0.5 * sy, (0.02 + 0.05 * p) * W, (0.45 - 0.045 * p) * H, 0.02 * p), dev) for p in range(10)],
            [part(rng, 0, ph, pw, affine(1.5 * sx, 1.5 * sy, -0.25 * W, -0.25 * H), dev),
             part(rng, 1, ph, pw, affine(0.5 * sx, 0.4 * sy, 0.3 * W, 0.2 * H), dev)],
            [part(rng, 0, ph, pw, [[0.8 * sx, 0.1, 0.05 * W], [0.05, 0.8 * sy, 0.05 * H], [0.012 / sx, 0.008 / sy, 1]], dev),
             part(rng, 1, ph, pw, affine(0.3 * sx, 0.9 * sy, 0.65 * W, 0.05 * H), dev)]]
    return jobs, (2, 3, 4)


def unfused(jobs, H, W, ksize):
    from training import patch_routing as P
    from torch_utils.ops import _native as nat
    dev = torch.device('cuda', 0)
    flat = [(t, m, (W, H)) for parts in jobs for patch, mask, m in parts for t in (patch, mask)]
    warped = P.warp_perspective_batch(flat)
    out = torch.full([len(jobs), H, W, 3], 7, dtype=torch.uint8, device=dev)
    ct = np.zeros(len(jobs), dtype=P._COMPOSE_DT)
    k = 0
    for j, parts in enumerate(jobs):
        ct[j]['canvas'], ct[j]['nparts'] = out.data_ptr() + j * H * W * 3, len(parts)
        for q in range(len(parts)):
            ct[j]['patch'][q], ct[j]['mask'][q] = warped[k].data_ptr(), warped[k + 1].data_ptr()
            k += 2
    tab = P._upload_table(ct, dev)
    nat.check(P._init().lib.pg_patch_compose_ordered_u8_k(tab.data_ptr(), len(jobs), H, W, 3, ksize, nat.stream_of(out)), 'pg_patch_compose_ordered_u8_k')
    torch.cuda.synchronize()
    return out


def check_coverage(canvases, jobs, two):
    for j, parts in enumerate(jobs):
        c = canvases[j].cpu().numpy()
        if not parts:
            assert not c.any()
            continue
        assert (c.any(axis=2)).mean() >= 0.05, j
        winners = set(np.unique((c[..., 0][c[..., 0] > 0] - 10) // 20).tolist())
        assert winners <= set(range(len(parts)))
        if j in two:
            assert len(winners) >= 2, (j, winners)


@pytest.mark.parametrize('H,W', [(40, 136), (64, 80)])
@pytest.mark.parametrize('ksize', [8, 5, 3])
def test_denorm_equals_the_unfused_launches(H, W, ksize):
    from training import snapshot_grid as S
    dev = _cuda()
    jobs, two = make_jobs(np.random.default_rng(H + ksize), H, W, 16, 20, dev)
    S.launch_counter = dict(denorm=0, cells=0)
    try:
        got = S.denorm_canvases(jobs, H, W, ksize)
        assert S.launch_counter == dict(denorm=1, cells=0)
    finally:
        S.launch_counter = None
    want = unfused(jobs, H, W, ksize)
    assert torch.equal(got, want)
    check_coverage(got, jobs, two)
    cpu = S.denorm_canvases([[(a.cpu(), b.cpu(), m) for a, b, m in parts] for parts in jobs[:2]], H, W, ksize)       # the CPU route, on the small jobs
    assert torch.equal(cpu, got[:2].cpu())


def test_denorm_at_the_real_size():
    from training import snapshot_grid as S
    dev = _cuda()
    jobs, two = make_jobs(np.random.default_rng(1), 512, 512, 128, 128, dev)
    jobs = [jobs[2]]
    got = S.denorm_canvases(jobs, 512, 512, 8)
    assert torch.equal(got, unfused(jobs, 512, 512, 8))
    check_coverage(got, jobs, (0,))


def test_denorm_argument_checks():
    from training import snapshot_grid as S
    dev = _cuda()
    lib = S._routing_lib()
    canvas = torch.full([8, 8, 3], 9, dtype=torch.uint8, device=dev)
    job = np.zeros(1, dtype=S._DENORM_DT)
    job['canvas'] = canvas.data_ptr()                         # a job without parts: the canvas is zeroed
    table = torch.from_numpy(job.view(np.uint8).reshape(-1)).to(dev)
    ok = dict(jobs=table.data_ptr(), njobs=1, H=8, W=8, ph=4, pw=4, mc=3, ksize=8, block_w=8)
    call = lambda **kw: lib.pg_patch_denorm_u8(*dict(ok, **kw).values(), None)
    assert call() == 0
    torch.cuda.synchronize()
    assert not canvas.any()
    for bad in (dict(jobs=None), dict(njobs=0), dict(H=0), dict(W=-1), dict(ph=0), dict(pw=0), dict(mc=0), dict(ksize=0), dict(ksize=17), dict(block_w=0)):
        assert call(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------------------- pg_snapshot_cells_u8

@pytest.mark.parametrize('C', [7, 1])
def test_cells_equal_the_numpy_arithmetic(C):
    import snapshot_grid_ref as ref
    from training import snapshot_grid as S
    dev = _cuda()
    rng = np.random.default_rng(C)
    n, H, W, gh, gw, first = 5, 8, 12, 3, 2, 1
    fin = (rng.standard_normal((n, 3, H, W)) * 0.8).astype(np.float32)
    fin.reshape(-1)[:9] = [0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 1.0, -1.0]
    fin.reshape(-1)[16:272] = (np.arange(256, dtype=np.float32) + 0.5) / 127.5 - 1          # around the rounding ties
    par = (rng.integers(-8, 8, (n, C, H, W)) * 0.25).astype(np.float32)                      # multiples of 0.25: exact ties, the lowest index wins in both
    grey = S.grey_table(C)
    grids = [torch.from_numpy(rng.integers(0, 256, ((gh + 1) * H, (gw + 1) * W, 3), dtype=np.uint8)).to(dev) for _ in range(2)]
    before = [g.cpu().numpy().copy() for g in grids]
    S.pack_cells(torch.from_numpy(fin).to(dev), torch.from_numpy(par).to(dev), torch.from_numpy(grey).to(dev), grids[0], grids[1], first, gh, gw)
    # the restatement's bytes for the same values: save_image_grid's conversion (NaN -> 0 is this package's rule; NumPy leaves that cast undefined)
    finite = np.where(np.isnan(fin), np.float32(-1), fin)
    want_img = np.rint((finite - (-1)) * (255 / 2)).clip(0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    want_par = np.rint((ref.parsing_values(par) - (-1)) * (255 / 2)).clip(0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    if C == 7:
        assert grey.tolist() == [0, 43, 85, 128, 170, 212, 255] and len(np.unique(want_par)) == 7
    for g, b, want in zip(grids, before, (want_img, want_par)):
        got = g.cpu().numpy()
        untouched = np.ones(got.shape[:2], dtype=bool)
        for k in range(n):
            r, c = 1 + (first + k) // gw, 1 + (first + k) % gw
            assert np.array_equal(got[r * H:(r + 1) * H, c * W:(c + 1) * W], want[k]), k
            untouched[r * H:(r + 1) * H, c * W:(c + 1) * W] = False
        assert np.array_equal(got[untouched], b[untouched]) and untouched.sum() == (12 - n) * H * W
    lib = S._cells_lib()
    f, p, gy = (torch.zeros(64, device=dev).data_ptr() for _ in range(3))
    for bad in ((1, 17, 4, 4, 1, 1, 0), (1, 0, 4, 4, 1, 1, 0), (2, 1, 4, 4, 1, 1, 0), (1, 1, 4, 4, 1, 1, -1), (0, 1, 4, 4, 1, 1, 0)):
        assert lib.pg_snapshot_cells_u8(f, p, gy, grids[0].data_ptr(), grids[1].data_ptr(), *bad, None) == -1, bad
    assert lib.pg_snapshot_cells_u8(f, p, gy, grids[0].data_ptr(), grids[1].data_ptr(), 1, 1, 4, 6, 1, 1, 0, None) == -2          # W % 4


def test_a_nan_logit_never_wins():
    from training import snapshot_grid as S
    dev = _cuda()
    H, W = 4, 8
    par = np.zeros((1, 3, H, W), dtype=np.float32)
    par[0, :, 0, 0] = [np.nan, 1.0, 1.0]                      # NaN at class 0: the first of the tied maxima behind it
    par[0, :, 0, 1] = [0.5, np.nan, 0.25]
    par[0, :, 0, 2] = [np.nan, np.nan, np.nan]                # nothing to pick: class 0
    par[0, :, 0, 3] = [-np.inf, np.nan, -np.inf]
    par[0, :, 0, 4] = [-1.0, -2.0, np.nan]
    grey = np.array([10, 20, 30], dtype=np.uint8)
    grids = [torch.zeros([2 * H, 2 * W, 3], dtype=torch.uint8, device=dev) for _ in range(2)]
    S.pack_cells(torch.zeros([1, 3, H, W], device=dev), torch.from_numpy(par).to(dev), torch.from_numpy(grey).to(dev), grids[0], grids[1], 0, 1, 1)
    got = grids[1].cpu().numpy()[H:, W:]
    assert got[0, :5, 0].tolist() == [20, 10, 10, 10, 10] and (got == got[..., 0:1]).all() and (got[1:] == 10).all()
    assert np.array_equal(S.cells_numpy(np.zeros((1, 3, H, W), np.float32), par, grey)[1][0], got)          # the CPU route, same rule


# ------------------------------------------------------------------------------------------------------------- the grid

@pytest.fixture(scope='module')
def vis_set(tmp_path_factory):
    from training.dataset import TrainSet
    return TrainSet(write_vis_root(str(tmp_path_factory.mktemp('vis_gpu'))), shuffle=False, device='cpu')


@pytest.fixture(scope='module')
def gpu_grid(vis_set):
    from training import snapshot_grid as S
    _cuda()
    S.launch_counter = dict(denorm=0, cells=0)
    try:
        grid = S.setup_snapshot_grid(vis_set, 'cuda')
        counts = dict(S.launch_counter)
    finally:
        S.launch_counter = None
    torch.cuda.synchronize()
    return grid, counts


def test_gpu_grid_equals_the_cpu_route(vis_set, gpu_grid):
    from training import snapshot_grid as S
    grid, counts = gpu_grid
    assert counts == dict(denorm=1, cells=0)                  # every canvas of the grid in ONE fused launch
    cpu = S.setup_snapshot_grid(vis_set, 'cpu')
    assert torch.equal(grid.upper_canvases().cpu(), cpu.upper_canvases()) and torch.equal(grid.lower_canvases().cpu(), cpu.lower_canvases())
    assert cpu.upper_canvases().flatten(1).any(dim=1).all()
    for name in ('norm_img', 'norm_img_lower', 'bound', 'label'):
        assert torch.equal(getattr(grid, name).cpu(), getattr(cpu, name)), name
    for lo, hi in ((0, 4), (4, 9)):
        got, want = grid.inputs(lo, hi), cpu.inputs(lo, hi)
        assert set(got) == set(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype
            assert torch.equal(got[k].cpu().view(torch.int32), want[k].contiguous().view(torch.int32)), (lo, k)       # bit for bit, NaN included
    for a, b in zip(grid.canvas_grids(), cpu.canvas_grids()):
        assert np.array_equal(a, b)


def test_render_with_a_narrow_generator(vis_set, gpu_grid):
    from training import snapshot_grid as S
    from training import training_loop as T
    grid, _ = gpu_grid
    torch.manual_seed(0)
    G = T.build_networks(4, 'cuda', dict(channel_base=4096, channel_max=512))[0].eval().requires_grad_(False)
    fin_grid, par_grid = grid.render(G, 4)
    side = 4 * 512
    assert fin_grid.shape == par_grid.shape == (side, side, 3) and fin_grid.dtype == np.uint8
    persons = grid.persons['image'].cpu().numpy()
    for out in (fin_grid, par_grid):
        assert (out[:512, :512] == S.CORNER).all()
        for i in range(3):
            assert np.array_equal(out[512 * (i + 1):512 * (i + 2), :512], persons[i]) and np.array_equal(out[:512, 512 * (i + 1):512 * (i + 2)], persons[i])
    assert set(np.unique(par_grid[512:, 512:])) <= set(S.grey_table(7).tolist())
    with torch.no_grad():
        for lo, hi in ((0, 4), (4, 8), (8, 9)):               # every fake cell = that chunk's generator output, packed on its own
            _, fin, par = G(**grid.inputs(lo, hi), noise_mode='const')
            img, pmap = S.cells_numpy(fin.cpu().numpy(), par.cpu().numpy(), S.grey_table(int(par.shape[1])))
            for k in range(hi - lo):
                r, c = 1 + (lo + k) // 3, 1 + (lo + k) % 3
                assert np.array_equal(fin_grid[512 * r:512 * (r + 1), 512 * c:512 * (c + 1)], img[k]), lo + k
                assert np.array_equal(par_grid[512 * r:512 * (r + 1), 512 * c:512 * (c + 1)], pmap[k]), lo + k
