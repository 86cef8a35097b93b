"""The lower-garment and full-outfit try-on modes (reference test.py --testpart lower | full) on the CPU: the patch routing's NumPy
route of ``normalize(part=...)`` against the test-side restatement of the reference's two ``normalize`` methods (tests/routing_modes_ref.py,
built from the oracle's primitives only), bit for bit; the loader's 16-tuple contract and mode-specific maps for all three modes on
synthetic pairs in the reference's file formats; one batch-1 generator forward per new mode.

PARITY UNPINNED against the reference, as for the upper mode: OpenCV is not available and the reference holds
no fixtures for this step."""

import json
import os

import numpy as np
import pytest
import torch

PIL = pytest.importorskip('PIL.Image')

JOINTS = dict(cnose=(256, 60), cneck=(256, 110), rshoulder=(200, 120), relbow=(180, 200), rwrist=(170, 270), lshoulder=(312, 120), lelbow=(335, 200),
              lwrist=(345, 270), rhip=(220, 290), rknee=(215, 390), rankle=(212, 480), lhip=(292, 290), lknee=(297, 390), lankle=(300, 480),
              reye=(246, 50), leye=(266, 50), rear=(236, 55), lear=(276, 55))
ORDER = ['cnose', 'cneck', 'rshoulder', 'relbow', 'rwrist', 'lshoulder', 'lelbow', 'lwrist', 'rhip', 'rknee', 'rankle', 'lhip', 'lknee', 'lankle',
         'reye', 'leye', 'rear', 'lear']
CASES = {'all_joints': (), 'missing_knees_and_nose': ('lknee', 'rknee', 'cnose'), 'no_left_arm_with_sleeve_mask': ('lelbow', 'lwrist'),
         'no_right_arm_with_sleeve_mask': ('relbow', 'rwrist'), 'nothing_valid': tuple(JOINTS)}


def keypoints(rng, jitter=8.0, drop=()):
    kp = np.zeros((18, 3))
    for k, (x, y) in JOINTS.items():
        kp[ORDER.index(k)] = (x + rng.normal(0, jitter), y + rng.normal(0, jitter), 0.0 if k in drop else 1.0)
    return kp


def routing_case(case, seed):
    """(upper_img, lower_img, upper_mask, lower_mask, sleeve | None, clothes_kp, person_kp) of one named case: the clothes' key points lose the
    case's joints (so that crops go missing), the person's keep all of them except in 'nothing_valid'."""
    rng = np.random.default_rng(seed)
    drop = CASES[case]
    ckp, pkp = keypoints(rng, 8.0, drop), keypoints(rng, 8.0, drop if case == 'nothing_valid' else ())
    up, lo = (rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) for _ in range(2))
    um = np.zeros((512, 512, 3), np.uint8)
    um[90:310, 150:370] = 255
    lm = np.zeros((512, 512, 3), np.uint8)
    lm[270:505, 190:330] = 255
    sleeve = None
    if 'sleeve' in case:
        sleeve = np.zeros((512, 512, 1), np.uint8)
        sleeve[100:300, :215] = 1
        sleeve[100:300, 300:] = 1
    return up, lo, um, lm, sleeve, ckp, pkp


@pytest.mark.parametrize('part', ['lower', 'full'])
@pytest.mark.parametrize('case', ['all_joints', 'missing_knees_and_nose', 'no_left_arm_with_sleeve_mask', 'nothing_valid'])
def test_cpu_normalize_matches_the_restatement_bit_for_bit(part, case):
    import routing_modes_ref as MR
    from training import patch_routing as P
    sample = routing_case(case, 17 + len(case))
    want = MR.normalize(part, *sample, 2)
    got = P.normalize(*sample, 2, device='cpu', part=part)
    assert len(got) == 4
    for nm, g, w_ in zip(('norm_img', 'norm_img_lower', 'denorm_upper_img', 'denorm_lower_img'), got, want):
        assert g.device.type == 'cpu' and g.dtype == torch.uint8 and tuple(g.shape) == w_.shape, nm
        assert np.array_equal(g.numpy(), w_), nm
    if case == 'all_joints':
        assert all(int(w_.astype(np.int64).sum()) > 0 for w_ in want)
    if case == 'nothing_valid':
        assert all(int(w_.astype(np.int64).sum()) == 0 for w_ in want)


def test_modes_differ_where_the_reference_says():
    """The three modes on one sample: full and upper route the upper garment through the same (clothes) crop but erode 5 x 5 instead of 8 x 8;
    full's lower parts are not masked by the upper ones, lower's are; the default is part='upper' and unknown modes are refused."""
    from training import patch_routing as P
    sample = routing_case('all_joints', 3)
    upper = P.normalize(*sample, 2, device='cpu')
    assert len(upper) == 5
    assert all(torch.equal(a, b) for a, b in zip(upper, P.normalize(*sample, 2, device='cpu', part='upper')))
    full = P.normalize(*sample, 2, device='cpu', part='full')
    lower = P.normalize(*sample, 2, device='cpu', part='lower')
    assert torch.equal(full[0], upper[0])                                   # same crops and sources for the upper parts
    up_px = lambda t: int((t.sum(dim=2) > 0).sum())
    assert up_px(full[2]) > up_px(upper[2])                                 # the smaller erode window keeps more of each pasted part
    assert not torch.equal(full[1], lower[1])
    with pytest.raises(ValueError):
        P.normalize(*sample, 2, device='cpu', part='shoes')
    with pytest.raises(ValueError):
        P.normalize_batch([sample], 2, device='cpu', part='')


def test_cpu_compose_window_sizes():
    """The CPU paste of every window size against the oracle's erode: anchor (k/2, k/2), outside taps ignored."""
    from oracle import patch_routing_ref as R
    from training import patch_routing as P
    rng = np.random.default_rng(9)
    h, w = 40, 52
    patch = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    canvas = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = (rng.random((h, w, 3)) > 0.01).astype(np.uint8) * 255
    for k in (1, 2, 3, 5, 7, 8, 16):
        m = (R.erode_u8(mask[..., 0], k)[..., None] == 255).astype(np.uint8)
        c1, c2 = torch.from_numpy(canvas.copy()), torch.zeros(h, w, 3, dtype=torch.uint8)
        P.patch_compose_(c1, torch.from_numpy(patch), torch.from_numpy(mask), c2, ksize=k)
        assert np.array_equal(c1.numpy(), patch * m + canvas * (1 - m)), k
        assert np.array_equal(c2.numpy(), patch * m), k


# ------------------------------------------------------------------------------------------- the loader, all three modes

PERSON_JOINTS = {k: (x - 96, y) for k, (x, y) in JOINTS.items()}        # in the unpadded 320-wide frame


def _write(root, name, rng, top=5, lower=9):
    """One synthetic photo: noise image, a blocky label map (top label `top` over the torso, `lower` over the legs; 6 = dress), its garment
    parsing (sleeves 10 / 11) and jittered OpenPose-18 key points."""
    for d in ('image', 'parsing', 'garment_parsing', 'keypoints'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    img = rng.integers(30, 226, (512, 320, 3), dtype=np.uint8)
    PIL.fromarray(img, 'RGB').save(os.path.join(root, 'image', name + '.jpg'), quality=95)
    lab = np.zeros((512, 320), np.uint8)
    lab[30:90, 130:190] = 13
    lab[15:30, 130:190] = 2
    lab[90:112, 145:175] = 10
    lab[112:300, 100:220] = top
    lab[112:280, 70:100] = 14
    lab[112:280, 220:250] = 15
    lab[290:470, 110:210] = lower
    lab[470:500, 105:150] = 18
    lab[470:500, 170:215] = 19
    PIL.fromarray(lab, 'L').save(os.path.join(root, 'parsing', name + '.png'))
    gp = np.zeros((512, 320, 3), np.uint8)
    gp[112:200, 70:100, 0] = 10
    gp[112:200, 220:250, 0] = 11
    PIL.fromarray(gp, 'RGB').save(os.path.join(root, 'garment_parsing', name + '.png'))
    kp = []
    for k in ORDER:
        x, y = PERSON_JOINTS[k]
        kp += [float(x + rng.normal(0, 4)), float(y + rng.normal(0, 4)), 0.9]
    with open(os.path.join(root, 'keypoints', name + '_keypoints.json'), 'w') as f:
        json.dump(dict(version=1.3, people=[dict(pose_keypoints_2d=kp)]), f)


@pytest.fixture(scope='module')
def pairs_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('mode_pairs'))
    rng = np.random.default_rng(23)
    _write(root, 'top_pants', rng, top=5, lower=9)
    _write(root, 'top_skirt', rng, top=5, lower=12)
    _write(root, 'dress', rng, top=6, lower=6)
    # pairs: <clothes> <person>
    with open(os.path.join(root, 'test_pairs.txt'), 'w') as f:
        f.write('top_pants.jpg top_skirt.jpg\ntop_skirt.jpg top_pants.jpg\ndress.jpg top_pants.jpg\ntop_pants.jpg dress.jpg\n')
    return root


SHAPES = [(3, 512, 512), (3, 512, 512), (3, 512, 512), (3, 512, 512), (30, 128, 128), (15, 128, 128), (3, 512, 512), (3, 512, 512),
          (1, 512, 512), (1, 512, 512), (1, 512, 512), (3, 512, 512), (1, 512, 512), (1, 512, 512)]
DTYPES = [np.uint8] * 11 + [np.float64, np.float64, np.uint8]


def _check_contract(item):
    assert len(item) == 16 and item[14].endswith('.jpg') and item[15].endswith('.jpg')
    for a, shape, dt in zip(item[:14], SHAPES, DTYPES):
        assert tuple(a.shape) == shape and a.dtype == dt, (a.shape, a.dtype, shape, dt)
    image, clothes, pose, cpose, norm_img, norm_lower, dup, dlo, mup, mlo, retain, skin, label, bound = item[:14]
    assert set(np.unique(mup)) <= {0, 1} and set(np.unique(mlo)) <= {0, 1} and set(np.unique(retain)) <= {0, 1}
    assert np.array_equal(mup[0], (dup.sum(axis=0) > 0).astype(np.uint8)) and np.array_equal(mlo[0], (dlo.sum(axis=0) > 0).astype(np.uint8))
    assert set(np.unique(bound)) <= {0, 255} and np.isfinite(skin).all() and len(np.unique(label)) == 1
    assert float(label.max()) in (0.0, 127.5, 255.0)


def _padded_labels(root, name):
    lab = np.array(PIL.open(os.path.join(root, 'parsing', name.replace('.jpg', '.png'))))
    return np.pad(lab, ((0, 0), (96, 96)))


def test_loader_contract_all_modes(pairs_root):
    from training.dataset import TryOnTestSet
    items = {part: [TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu', part=part)[i] for i in range(4)] for part in ('upper', 'lower', 'full')}
    default = TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu')[0]
    for a, b in zip(default, items['upper'][0]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    for part, its in items.items():
        for it in its:
            _check_contract(it)
    with pytest.raises(ValueError):
        TryOnTestSet(pairs_root, part='shoes')

    # full: both garments come from the clothes image; the lower garment's class from the CLOTHES' parsing; the bound starts at the routed lower garment
    f = items['full']
    for i, lab in ((0, 0.0), (1, 127.5)):                                   # clothes in pants -> 0, clothes in a skirt -> 1 (whatever the person wears)
        it = f[i]
        assert float(it[12].max()) == lab
        assert it[5].any() and it[9].sum() > 1000 and it[8].sum() > 1000      # the lower garment was routed onto the person
        rows = np.nonzero(it[9][0].any(axis=1))[0]
        assert (it[13][0, rows[0]:] == 255).all() and (it[13][0, :rows[0]] == 0).all()
    assert float(f[2][12].max()) == 255.0 and f[2][13].sum() == 0 and f[2][9].sum() == 0 and not f[2][5].any()   # a dress as the outfit
    # lower: the clothes' lower garment is routed, the person keeps the top (8 x 8 eroded); label from the clothes unless the person wears a dress
    lo = items['lower']
    assert float(lo[0][12].max()) == 0.0 and float(lo[1][12].max()) == 127.5
    for it, person in ((lo[0], 'top_skirt.jpg'), (lo[1], 'top_pants.jpg')):
        assert it[9].sum() > 1000 and it[5].any()
        plab = _padded_labels(pairs_root, person)
        assert it[8].sum() > 1000 and not it[8][0][~np.isin(plab, (5, 7))].any()        # the person's own top, nothing else
        rows = np.nonzero(np.isin(plab, (9, 12)).any(axis=1))[0]
        assert (it[13][0, rows[0]:] == 255).all() and (it[13][0, :rows[0]] == 0).all()  # the bound: the person's own lower garment
    assert not lo[2][5].any() and lo[2][9].sum() == 0 and float(lo[2][12].max()) == 127.5   # a dress as the garment has no lower part: nothing routed
    assert not lo[3][5].any() and lo[3][9].sum() == 0 and lo[3][13].sum() == 0 and float(lo[3][12].max()) == 255.0   # a person in a dress keeps it
    # upper, as before: a dress garment removes the person's lower garment
    assert items['upper'][2][7].sum() == 0 and float(items['upper'][2][12].max()) == 255.0


@pytest.mark.parametrize('part', ['lower', 'full'])
def test_generator_forward_on_cpu_per_mode(pairs_root, part):
    from training.dataset import TryOnTestSet, to_generator_inputs
    from training import networks as PN
    from detgen import fill_module_
    ds = TryOnTestSet(pairs_root, device='cpu', part=part)
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)))
    inp = to_generator_inputs(batch, 'cpu')
    assert inp['c'].shape == (1, 45, 128, 128) and inp['retain'].shape == (1, 6, 512, 512) and inp['pose'].shape == (1, 5, 512, 512)
    torch.manual_seed(0)
    G = fill_module_(PN.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=64, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                          synthesis_kwargs=dict(channel_base=4096, channel_max=512, conv_clamp=256)), 'cfg1.').eval()
    with torch.no_grad():
        img, finetune_img, pred_parsing = G(**inp, noise_mode='const')
    assert img.shape == finetune_img.shape == (1, 3, 512, 512) and pred_parsing.shape == (1, 7, 512, 512)
    assert all(torch.isfinite(t).all() for t in (img, finetune_img, pred_parsing))
