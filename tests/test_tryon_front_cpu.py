"""The native front half of the try-on loader, host side (training/dataset.py ``raw`` / ``collate_raw``, training/tryon_front.py on a CPU batch, the
driver's ``front=`` option) -- and the crafted people the GPU tests (tests/test_tryon_front_gpu.py) share: each is there because one rule of the loader
can go wrong on it."""

import json
import os

import numpy as np
import pytest
import torch

PIL = pytest.importorskip('PIL.Image')

from test_dataset_loader import ORDER, _write_person  # noqa: E402
from test_tryon_cpu import PARTS, _small_generator, pairs_root  # noqa: E402,F401


# --------------------------------------------------------------------------------------------------- crafted people

def _labels(root, name):
    return np.array(PIL.open(os.path.join(root, 'parsing', name + '.png')))


def _set_labels(root, name, lab):
    PIL.fromarray(lab, 'L').save(os.path.join(root, 'parsing', name + '.png'))


def _keypoints(root, name):
    with open(os.path.join(root, 'keypoints', name + '_keypoints.json')) as f:
        return np.array(json.load(f)['people'][0]['pose_keypoints_2d']).reshape(18, 3)


def _set_keypoints(root, name, kp):
    people = [] if kp is None else [dict(pose_keypoints_2d=[float(v) for v in np.asarray(kp).reshape(-1)])]
    with open(os.path.join(root, 'keypoints', name + '_keypoints.json'), 'w') as f:
        json.dump(dict(version=1.3, people=people), f)


J = {k: i for i, k in enumerate(ORDER)}


def _equal_pants_skirt(lab, kp):
    lab[380:470][lab[380:470] == 9] = 12          # 90 rows of pants, 90 rows of skirt: neither is larger (the ``else`` branch)


def _dress_with_pants(lab, kp):
    lab[112:200][lab[112:200] == 5] = 6           # a dress over pants: the dress counts as a top


def _dress_swallows(lab, kp):
    lab[lab == 9] = 0
    lab[150:400, 100:220] = 6                     # a large dress, a small top above it and a small skirt below: all of it becomes the dress
    lab[400:420, 100:220] = 12


def _dress_to_skirt(lab, kp):
    lab[lab == 9] = 0
    lab[300:330, 100:220] = 6                     # a small dress, tops larger than the skirt: the dress joins the skirt
    lab[330:400, 110:210] = 12


def _dress_to_tops(lab, kp):
    lab[lab == 9] = 0
    lab[112:300][lab[112:300] == 5] = 0
    lab[112:150, 100:220] = 5                     # a small dress, the skirt larger than the tops: the dress joins the tops
    lab[150:180, 100:220] = 6
    lab[290:470, 100:220] = 12


def _no_lower(lab, kp):
    lab[lab == 9] = 0


def _edges(lab, kp):
    lab[0:150, 0:100] = 5                         # a top touching the image's left edge and its top row
    lab[290:512, 0:110] = 9                       # pants touching the left edge and the bottom row
    lab[300:400, 210:320] = 9                     # ... and the right edge


def _no_skin(lab, kp):
    lab[(lab == 10) | (lab == 13)] = 0            # neck and face empty: NaN medians


def _no_elbow(lab, kp):
    kp[J['relbow'], 2] = 0.0                      # both bands of that arm are absent: its hand label disappears entirely


def _high_hips(lab, kp):
    kp[J['lhip']] = [300.0, 20.0, 0.9]            # hips near the top and far apart: the hip rule gives a negative row
    kp[J['rhip']] = [20.0, 30.0, 0.9]


def _zero_limb(lab, kp):
    kp[J['rwrist'], :2] = kp[J['relbow'], :2]     # fore-arm of zero length: a segment with ln == 0, and a degenerate band
    kp[J['lknee'], :2] = np.floor(kp[J['lhip'], :2]) + 0.5          # distinct points with equal integer parts


def _outside(lab, kp):
    kp[J['lwrist']] = [-30.5, 600.2, 0.9]         # key points outside the frame, on every side
    kp[J['rshoulder']] = [340.7, -12.3, 0.9]
    kp[J['rknee'], 0] = 290.0                     # a leg joint within 50 pixels of the frame: demoted


CRAFTED = [('equal', _equal_pants_skirt), ('dresspants', _dress_with_pants), ('swallow', _dress_swallows), ('toskirt', _dress_to_skirt),
           ('totops', _dress_to_tops), ('nolower', _no_lower), ('edges', _edges), ('noskin', _no_skin), ('noelbow', _no_elbow), ('hips', _high_hips),
           ('zerolimb', _zero_limb), ('outside', _outside)]


def write_crafted(root):
    """The crafted people plus 'median' (lossless image, four skin pixels), 'nobody' (``people: []``) and a plain 'base'; every one is the person of one
    pair and the clothes of the next.  Returns the names in pair order."""
    rng = np.random.default_rng(23)
    names = []
    for name, change in CRAFTED:
        _write_person(root, name, rng, dress=name == 'swallow')
        lab, kp = _labels(root, name), _keypoints(root, name)
        change(lab, kp)
        _set_labels(root, name, lab)
        _set_keypoints(root, name, kp)
        names.append(name + '.jpg')
    _write_person(root, 'nobody', rng)
    _set_keypoints(root, 'nobody', None)
    _write_person(root, 'base', rng)
    names += ['nobody.jpg', 'base.jpg']
    # an even count of skin bytes whose two middle ones differ by an odd amount (.5), zero bytes that do not count, an odd count
    _write_person(root, 'median', rng)
    os.remove(os.path.join(root, 'image', 'median.jpg'))
    lab = _labels(root, 'median')
    lab[(lab == 10) | (lab == 13)] = 0
    lab[40, 150:152], lab[100, 150:152] = 13, 10
    _set_labels(root, 'median', lab)
    img = rng.integers(30, 226, (512, 320, 3), dtype=np.uint8)
    img[40, 150], img[40, 151], img[100, 150], img[100, 151] = [10, 0, 1], [20, 5, 255], [31, 6, 0], [40, 7, 0]
    PIL.fromarray(img, 'RGB').save(os.path.join(root, 'image', 'median.png'))
    names.append('median.png')
    with open(os.path.join(root, 'test_pairs.txt'), 'w') as f:
        for i, person in enumerate(names):
            f.write(f'{names[(i + 1) % len(names)]} {person}\n')
    return names


@pytest.fixture(scope='module')
def crafted_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('tryon_crafted'))
    write_crafted(root)
    return root


def write_narrow(root, width=318):
    """Two people in images `width` wide (left = (512 - width) // 2 is odd for 318: no source dword is aligned with the frame's)."""
    rng = np.random.default_rng(31)
    for name, dress in (('narrow_a', False), ('narrow_b', True)):
        _write_person(root, name, rng, dress=dress)
        for folder, file in (('image', name + '.jpg'), ('parsing', name + '.png'), ('garment_parsing', name + '.png')):
            path = os.path.join(root, folder, file)
            a = np.array(PIL.open(path))[:, :width]
            PIL.fromarray(a).save(path, **(dict(quality=95) if file.endswith('.jpg') else {}))
    with open(os.path.join(root, 'test_pairs.txt'), 'w') as f:
        f.write('narrow_b.jpg narrow_a.jpg\nnarrow_a.jpg narrow_b.jpg\n')


def assert_same_batch(got, want, ctx):
    """`got` is the ``collate_unrouted`` batch `want`, key by key: every byte, the float32 skin with its NaN positions, the lists."""
    assert list(got) == list(want), ctx
    for k, w in want.items():
        g = got[k]
        if w is None:
            assert g is None, (ctx, k)
        elif isinstance(w, torch.Tensor):
            assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (ctx, k, g.dtype, g.shape, g.device)
            if w.dtype == torch.float32:
                assert torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(torch.nan_to_num(g), torch.nan_to_num(w)), (ctx, k, g, w)
            else:
                bad = (g != w).reshape(len(w), -1).sum(dim=1).tolist()
                assert torch.equal(g, w), (ctx, k, 'differing entries per sample', bad)
        elif k.endswith('_kp'):
            assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)), (ctx, k)
        else:
            assert g == w, (ctx, k)


def _host_batch(ds):
    from training.dataset import collate_unrouted
    return collate_unrouted([ds.unrouted(i) for i in range(len(ds))])


def _raw_batch(ds):
    from training.dataset import collate_raw
    return collate_raw([ds.raw(i) for i in range(len(ds))])


# --------------------------------------------------------------------------------------------------- raw / collate_raw

@pytest.mark.parametrize('part', PARTS)
def test_raw_items_and_their_keypoints(pairs_root, part):
    from training.dataset import PRIMS, TryOnTestSet
    ds = TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu', part=part)
    for i in range(len(ds)):
        r, u = ds.raw(i), ds.unrouted(i)
        for k in ('person_img', 'clothes_img'):
            assert r[k].dtype == np.uint8 and r[k].shape == (512, 320, 3)
        for k in ('person_parsing', 'clothes_parsing', 'garment_parsing'):
            assert r[k].dtype == np.uint8 and r[k].shape == (512, 320)
        assert r['pose_prims'].dtype == np.int32 and r['pose_prims'].shape == (PRIMS, 8) and set(r['pose_prims'][:, 0]) <= {0, 1, 2}
        assert r['bands'].dtype == np.float64 and r['bands'].shape == (4, 4, 2) and r['band_absent'].shape == (4,)
        assert isinstance(r['hip_top'], int)
        for k in ('person_kp', 'clothes_kp'):
            assert r[k].dtype == np.float64 and np.array_equal(r[k], u[k]), (part, i, k)
        assert r['person_kp'][10, 2] == 0.01 and r['clothes_kp'][13, 2] == 0.01          # the ankles, within 50 pixels of the frame: demoted
        assert (r['person_name'], r['clothes_name']) == (u['person_name'], u['clothes_name'])
    assert TryOnTestSet(pairs_root, use_sleeve_mask=False, part=part).raw(0)['garment_parsing'] is None
    batch = _raw_batch(ds)
    assert batch['person_img'].dtype == torch.uint8 and tuple(batch['person_img'].shape) == (3, 512, 320, 3)
    assert tuple(batch['clothes_parsing'].shape) == (3, 512, 320) and tuple(batch['pose_prims'].shape) == (3, PRIMS, 8)
    assert batch['bands'].dtype == torch.float64 and tuple(batch['bands'].shape) == (3, 4, 4, 2) and batch['band_absent'].dtype == torch.int32
    assert batch['hip_top'].dtype == torch.int32 and tuple(batch['hip_top'].shape) == (3, 2) and batch['hip_top'][:, 0].tolist() == [1, 1, 1]
    assert isinstance(batch['person_kp'], list) and batch['person_name'] == ['person_a.jpg', 'person_b.jpg', 'dress_c.jpg']


def test_the_crafted_people_meet_the_rules_they_are_there_for(crafted_root):
    from training.dataset import TryOnTestSet
    names = [n for n, _ in CRAFTED] + ['nobody', 'base', 'median']
    at = {n: i for i, n in enumerate(names)}                              # pair i: person names[i], clothes names[i + 1]
    ds = TryOnTestSet(crafted_root, use_sleeve_mask=True, part='upper')
    raw = {n: ds.raw(at[n]) for n in ('noelbow', 'hips', 'nobody', 'zerolimb', 'outside')}
    assert raw['noelbow']['band_absent'].tolist() == [0, 0, 1, 1]
    assert raw['hips']['hip_top'] < 0
    assert raw['nobody']['hip_top'] is None and not raw['nobody']['pose_prims'].any() and raw['nobody']['band_absent'].all()
    z = raw['zerolimb']['pose_prims']
    assert any(k == 1 and (x0, y0) == (x1, y1) for k, x0, y0, x1, y1 in z[:, :5].tolist())
    assert np.array_equal(raw['zerolimb']['bands'][3, 0], raw['zerolimb']['bands'][3, 3])
    assert raw['outside']['pose_prims'][:, 1:5].min() < 0 and raw['outside']['person_kp'][9, 2] == 0.01
    host = {n: ds.unrouted(at[n]) for n in ('noskin', 'median', 'equal', 'nolower')}
    assert np.isnan(host['noskin']['skin']).all()
    assert host['median']['skin'].tolist() == [25.5, 6.0, 128.0]
    assert host['equal']['label'] == 1 and host['nolower']['label'] == 1 and not host['nolower']['lower_mask'].any()


# --------------------------------------------------------------------------------------------------- front_batch on a CPU batch

@pytest.mark.parametrize('sleeve', [False, True])
@pytest.mark.parametrize('part', PARTS)
def test_front_batch_on_the_cpu_equals_the_host_loader(pairs_root, part, sleeve):
    from training.dataset import TryOnTestSet
    from training import tryon_front
    ds = TryOnTestSet(pairs_root, use_sleeve_mask=sleeve, device='cpu', part=part)
    assert_same_batch(tryon_front.front_batch(_raw_batch(ds), part), _host_batch(ds), (part, sleeve))


def test_front_batch_on_the_cpu_for_a_narrow_image(tmp_path):
    from training.dataset import TryOnTestSet
    from training import tryon_front
    write_narrow(str(tmp_path))
    ds = TryOnTestSet(str(tmp_path), use_sleeve_mask=True, device='cpu', part='lower')
    raw = _raw_batch(ds)
    assert tuple(raw['person_img'].shape) == (2, 512, 318, 3)
    assert_same_batch(tryon_front.front_batch(raw, 'lower'), _host_batch(ds), 'narrow')


# --------------------------------------------------------------------------------------------------- the driver

def test_the_native_front_writes_the_same_images_on_the_cpu(pairs_root, tmp_path):
    from training.dataset import TryOnTestSet
    from training import tryon
    pairs = tmp_path / 'one_pair.txt'                                      # (the generator is what takes the time on a CPU: one pair per front)
    pairs.write_text('dress_c.jpg person_b.jpg\n')
    ds = TryOnTestSet(pairs_root, test_txt=str(pairs), use_sleeve_mask=True, device='cpu', part='upper')
    G = _small_generator()
    files = {front: tryon.run_tryon(ds, G, str(tmp_path / front), batch_size=1, device='cpu', workers=0, front=front) for front in ('host', 'native')}
    assert [os.path.basename(f) for f in files['host']] == [os.path.basename(f) for f in files['native']] and len(files['host']) == 1
    for a, b in zip(files['host'], files['native']):
        with open(a, 'rb') as fa, open(b, 'rb') as fb:
            assert fa.read() == fb.read(), b


def test_an_unknown_front_is_an_error(pairs_root, tmp_path):
    from training.dataset import TryOnTestSet
    from training import tryon
    ds = TryOnTestSet(pairs_root, part='upper')
    with pytest.raises(ValueError, match='front'):
        tryon.run_tryon(ds, None, str(tmp_path), device='cpu', front='bogus')
    assert tryon.parse_args(['--network', 'n.pkl', '--dataroot', 'd', '--testpart', 'upper', '--outdir', 'o']).front == 'host'
    assert tryon.parse_args(['--network', 'n.pkl', '--dataroot', 'd', '--testpart', 'upper', '--outdir', 'o', '--front', 'native']).front == 'native'
