"""The training driver's image snapshots on the CPU: `setup_snapshot_grid` on a SYNTHETIC dataset directory with three visualisation persons (a full
outfit, a dress, a person whose part 7 is missing) against the test-side restatement (tests/snapshot_grid_ref.py) bit for bit, one cell per mode plus a second
one in the row of the person with the missing part (the upper-garment row, so the zero-``M_inv`` branch runs in both) -- the byte conversion and grid assembly against
the restatement's ``save_image_grid``, and the driver writing the four kinds of PNG.

PARITY UNPINNED against the reference's OpenCV rasterising and warps, as for the other modes (DESIGN.md sections 6d, 6h).

Measured: the restatement's NumPy warps take ~4 s per cell, the product's CPU grid ~9 s: all four cells are kept.  The driver run with images
takes the longest (one training image and nine generator passes at the narrowest width the networks accept, on the CPU: ~30 s)."""

import os

import numpy as np
import pytest
import torch

from test_train_loader import write_train_person, write_train_root

PIL = pytest.importorskip('PIL.Image')

VIS = [('a_full', 'full'), ('b_dress', 'dress'), ('c_knee', 'low_knee')]          # rows 0 (lower-garment swaps), 1 (full outfit), 2 (upper garment)
CELLS = [2, 3, 6, 7]                                                              # (row 0, col 2), (row 1, col 0), (row 2, col 0), (row 2, col 1)
WIDTH = dict(channel_base=4096, channel_max=512)       # the narrowest the networks take (res 8 needs 512 channels)


def write_vis_root(root):
    rng = np.random.default_rng(5)
    sub = os.path.join(root, 'Zalando_512_320_v1')
    for name, kind in VIS:
        write_train_person(sub, name, rng, kind)
    with open(os.path.join(sub, 'train_pairs_front_list_220508.txt'), 'w') as f:
        f.write(''.join(f'{n}.jpg {n}.jpg\n' for n, _ in VIS))
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    m = np.zeros((512, 512), np.uint8)
    m[150:330, 200:300] = 255
    PIL.fromarray(m, 'L').save(os.path.join(root, 'train_random_mask_acgpn', 'mask_0.png'))
    os.makedirs(os.path.join(root, 'train_img_front_vis_512_220414'))
    for name, _ in VIS:
        open(os.path.join(root, 'train_img_front_vis_512_220414', name + '.jpg'), 'w').close()          # only the names are read
    return root


@pytest.fixture(scope='module')
def vis_set(tmp_path_factory):
    from training.dataset import TrainSet
    return TrainSet(write_vis_root(str(tmp_path_factory.mktemp('vis'))), shuffle=False, device='cpu')


@pytest.fixture(scope='module')
def grid(vis_set):
    from training import snapshot_grid as S
    return S.setup_snapshot_grid(vis_set, 'cpu')


@pytest.fixture(scope='module')
def want(vis_set):
    import snapshot_grid_ref as ref
    return ref.setup_snapshot_image_grid(vis_set, 3, CELLS)


def test_vis_index_and_cell_rules(vis_set, grid):
    from training import snapshot_grid as S
    assert vis_set.vis_index == [0, 1, 2] and grid.gnum == 3 and len(grid) == 9
    assert [S.cell_sources(i, 3)[2:] for i in (0, 2, 3, 5, 6, 8)] == [(0, 0, 'lower'), (0, 2, 'lower'), (0, 0, 'full'), (2, 2, 'full'), (0, 2, 'upper'),
                                                                      (2, 2, 'upper')]
    assert S.cell_sources(20, 14)[4] == 'lower' and S.cell_sources(4 * 14, 14)[4] == 'full' and S.cell_sources(8 * 14 + 3, 14) == (8, 3, 3, 8, 'upper')
    with pytest.raises(ValueError):
        S.setup_snapshot_grid(vis_set, 'cpu', gnum=2)
    # shared canvases: denorm_upper does not depend on the column in the lower-garment row, nor denorm_lower in the upper-garment row
    assert len(set(grid.upper_index[0:3].tolist())) == 1 and len(set(grid.lower_index[6:9].tolist())) == 1
    assert grid.canvases.shape[0] == 14 and grid.canvases.dtype == torch.uint8
    assert not grid.persons['gt_rows'][1].any() and grid.persons['gt_rows'][0].any()          # the dress has no lower garment


@pytest.mark.parametrize('cell', CELLS)
def test_cpu_route_equals_the_restatement_bit_for_bit(grid, want, cell):
    w = want[cell]
    chw = lambda t: t.permute(2, 0, 1).numpy()
    up, lo = chw(grid.upper_canvases(cell, cell + 1)[0]), chw(grid.lower_canvases(cell, cell + 1)[0])
    assert np.array_equal(up, w['denorm_upper']) and np.array_equal(lo, w['denorm_lower'])
    assert up.any() and lo.any()
    parts = np.concatenate([chw(grid.norm_img[cell]), chw(grid.norm_img_lower[cell])], axis=0)
    assert parts.shape == (45, 128, 128) and np.array_equal(parts, w['parts'])
    assert parts[30:].any() and parts[:30].any()
    bound = w['conditions'][1]
    assert (bound == bound[:, 0:1]).all() and np.array_equal(grid.bound[cell].numpy(), bound[:, 0].astype(np.uint8)) and bound.any() and not bound.all()
    label = w['conditions'][0]
    assert (label == label[0, 0]).all() and float(grid.label[cell]) * 127.5 == label[0, 0]
    got = grid.inputs(cell, cell + 1)
    assert set(got) == set(w['inputs']) | {'z'} and tuple(got['z'].shape) == (1, 0)
    for k, v in w['inputs'].items():
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == v.shape, k
        assert np.array_equal(got[k].numpy().view(np.uint32), v.view(np.uint32)), (cell, k)
    assert np.array_equal(got['denorm_upper_mask'].numpy()[0], w['upper_mask'].astype(np.float32))
    if cell in (6, 7):                                             # the row of the person whose part 7 is missing: its patches are zero, the others' are not
        assert not parts[21:24].any() and not parts[36:39].any() and parts[18:21].any()
        assert parts[33:36].any() == (cell == 6)              # (cell 7: the dress covers the thighs, so the lower patch gives way entirely)


def test_at_least_two_parts_are_visible(grid, vis_set):
    """The paste order matters somewhere: in the compared upper canvas of cell 3, at least two parts own pixels (each part pasted alone leaves pixels that
    the full canvas keeps)."""
    from training import snapshot_grid as S
    from training import patch_routing as P
    u = vis_set.unrouted(1, None)
    m_invs = P.crop_matrices(u['person_kp'], 512, 512, 2)[1]
    canvas = grid.upper_canvases(3, 4)[0]
    owners = 0
    for ii in (0, 2):
        patch = grid.norm_img[3][:, :, 3 * ii:3 * ii + 3].contiguous()
        alone = P._warp_perspective_cpu(patch, m_invs[ii], (512, 512))
        owners += bool(((alone == canvas).all(dim=2) & (alone != 0).any(dim=2)).sum() > 100)
    assert owners == 2


def test_bytes_and_grid_assembly_against_save_image_grid():
    import snapshot_grid_ref as ref
    from training import snapshot_grid as S
    rng = np.random.default_rng(3)
    g, H, W = 2, 8, 12
    fin = (rng.standard_normal((g * g, 3, H, W)) * 0.8).astype(np.float32)
    fin.reshape(-1)[:8] = [0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, 1.0, -1.0]
    fin.reshape(-1)[8:264] = (np.arange(256, dtype=np.float32) + 0.5) / 127.5 - 1           # around the rounding ties
    par = (rng.integers(-8, 8, (g * g, 7, H, W)) * 0.25).astype(np.float32)                   # exact ties: the lowest index wins
    persons = rng.integers(0, 256, (g, H, W, 3), dtype=np.uint8)
    images = ref.unit(persons.transpose(0, 3, 1, 2))
    side, top = ref.side_and_top(images, g)
    want_img = ref.save_image_grid(side, top, fin, [-1, 1], (g, g))
    want_par = ref.save_image_grid(side, top, ref.parsing_values(par), [-1, 1], (g, g))
    # the product's own base assembly: the side, top and corner cells as `SnapshotGrid.__init__` lays them out (it reads the persons' images only)
    holder = S.SnapshotGrid(g, torch.device('cpu'), dict(image=torch.from_numpy(persons)), *[None] * 8)
    grid_img, grid_par = holder.grid_img, holder.grid_parsing
    assert (grid_img[:H, :W] == S.CORNER).all()               # the reference's corner cell is float 0 in [-1, 1]: rint(127.5) = 128
    grey = torch.from_numpy(S.grey_table(7))
    for lo in (0, 3):                                         # chunks of 3 and 1
        hi = min(lo + 3, g * g)
        S.pack_cells(torch.from_numpy(fin[lo:hi]), torch.from_numpy(par[lo:hi]), grey, grid_img, grid_par, lo, g, g)
    assert np.array_equal(grid_img.numpy(), want_img) and np.array_equal(grid_par.numpy(), want_par)
    nan = np.full((1, 3, H, W), np.nan, dtype=np.float32)
    assert not S.image_bytes(nan).any()


def test_grey_table_and_round_trip():
    from training import snapshot_grid as S
    k = np.arange(7, dtype=np.float32)
    want = np.rint((((k / 6 * 2 - 1.0) + 1) * np.float32(127.5))).clip(0, 255).astype(np.uint8)
    assert S.grey_table(7).tolist() == want.tolist() == [0, 43, 85, 128, 170, 212, 255]
    u = np.arange(256, dtype=np.uint8)
    import snapshot_grid_ref as ref
    assert np.array_equal(S.image_bytes(ref.unit(u)), u)                                     # the persons' cells: the float round trip is the identity
    assert np.array_equal(S.image_bytes(u.astype(np.float32) / np.float32(127.5) - 1), u)


def test_driver_writes_the_four_kinds_of_png(vis_set, tmp_path, capsys):
    from training import training_loop as T
    run = str(tmp_path / 'run')
    T.training_loop(run, vis_set.path, batch=1, batch_gpu=1, kimg=0.001, tick=0.001, snap=1, workers=0, device='cpu', width=WIDTH, aug='noaug',
                    dataset_kwargs=dict(shuffle=False))
    out = capsys.readouterr().out
    assert 'Exporting sample images...' in out
    names = sorted(os.listdir(run))
    for name in ('init_denorm_upper.png', 'init_denorm_lower.png', 'fakes000000_finetune.png', 'fakes000000_parsing.png'):
        assert name in names, names
        im = PIL.open(os.path.join(run, name))
        assert im.size == (4 * 512, 4 * 512) and im.mode == 'RGB'
    upper = np.array(PIL.open(os.path.join(run, 'init_denorm_upper.png')))
    person = vis_set.unrouted(0, None)['image']
    assert np.array_equal(upper[512:1024, 0:512], person) and np.array_equal(upper[0:512, 512:1024], person) and (upper[0:512, 0:512] == 128).all()
    assert upper[512:, 512:].any()


def test_image_interval_and_option():
    """`--snap` drives both kinds of snapshot; `image_snap` / `--image-snap` overrides the image interval, 0 turns it off."""
    from training import training_loop as T
    assert T.image_interval(50, None) == 50 and T.image_interval(50, 7) == 7 and T.image_interval(50, 0) == 0 and T.image_interval(None, None) == 0
    assert T.image_interval(None, 3) == 3
    base = ['--data', 'd', '--outdir', 'o']
    assert T.parse_args(base).image_snap is None and T.parse_args(base + ['--image-snap', '0']).image_snap == 0
    assert T.parse_args(base + ['--snap', '9']).snap == 9


def test_driver_without_vis_directory_says_so(tmp_path, capsys):
    from training import training_loop as T
    root = write_train_root(str(tmp_path / 'train'))
    run = str(tmp_path / 'run')
    T.training_loop(run, root, batch=1, batch_gpu=1, kimg=0.001, tick=0.001, snap=1, workers=0, device='cpu', width=WIDTH, aug='noaug',
                    dataset_kwargs=dict(shuffle=False))
    out = capsys.readouterr().out
    assert 'image snapshots are off' in out and 'Exporting sample images' not in out
    assert not [n for n in os.listdir(run) if n.endswith('.png')] and [n for n in os.listdir(run) if n.endswith('.pt')]
