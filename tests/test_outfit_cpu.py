"""The mixed-outfit try-on mode (``part='outfit'``: the top of one clothes image U, the trousers or skirt of another, L, on one person P) without a
GPU.  There is no reference code for this mode; it is specified as `_host_full`'s statements with the lower-garment quantities taken from L, and two
identities follow, which every test here stands on, byte for byte:

1. ``outfit(U, U, P)`` is ``full(U, P)``;
2. ``outfit(U, L, P)`` has the upper results of ``full(U, P)`` and the lower results of ``full(L, P)``.

The people, the batch comparison and the crafted result image come from the existing try-on tests."""

import functools
import os

import numpy as np
import pytest
import torch

PIL = pytest.importorskip('PIL.Image')

from test_dataset_loader import _write_person  # noqa: E402
from test_tryon_cpu import _small_generator, crafted_triptych_case, pairs_root  # noqa: E402,F401
from test_tryon_front_cpu import _labels, _set_labels, assert_same_batch, crafted_root, write_narrow  # noqa: E402,F401

UNROUTED_KEYS = ['upper_img', 'lower_img', 'upper_mask', 'lower_mask', 'sleeve', 'image', 'clothes', 'pose', 'retain_mask', 'bound', 'canvas', 'skin',
                 'label', 'clothes_kp', 'person_kp', 'person_name', 'clothes_name']                  # of the three existing modes, as they were
RAW_KEYS = ['person_img', 'clothes_img', 'person_parsing', 'clothes_parsing', 'garment_parsing', 'pose_prims', 'bands', 'band_absent', 'hip_top',
            'clothes_kp', 'person_kp', 'person_name', 'clothes_name']
OUTFIT_UNROUTED, OUTFIT_RAW = {'lower_kp', 'lower_clothes', 'lower_name'}, {'lower_kp', 'lower_img', 'lower_parsing', 'lower_name'}      # outfit batches only


def dataset(root, lines, part, sleeve=False):
    """A ``TryOnTestSet`` over `lines` (one string of names each), through a pairs file of its own under `root`."""
    from training.dataset import TryOnTestSet
    name = f'pairs_{part}_{abs(hash(tuple(lines)))}.txt'
    with open(os.path.join(root, name), 'w') as f:
        f.write(''.join(line + '\n' for line in lines))
    return TryOnTestSet(root, test_txt=name, use_sleeve_mask=sleeve, device='cpu', part=part)


def listed_pairs(root):
    with open(os.path.join(root, 'test_pairs.txt')) as f:
        return [tuple(line.split()) for line in f if line.strip()]


def sample(u):
    """The routing sample of an ``unrouted`` item (outfit items: with the lower key points as the eighth entry)."""
    s = (u['upper_img'], u['lower_img'], u['upper_mask'], u['lower_mask'], u['sleeve'], u['clothes_kp'], u['person_kp'])
    return s + ((u['lower_kp'],) if 'lower_kp' in u else ())


@functools.lru_cache(maxsize=None)
def full_of(root, clothes, person, sleeve=False):
    """(the unrouted item, its CPU routing) of ``full(clothes, person)``: computed once, shared, never written to.  Two crafted people (a limb of zero
    length, key points that give a degenerate quadrilateral) have no routing in any mode: the homography solve raises ``LinAlgError``, which is then what
    is returned in the routing's place -- the outfit mode has to raise it too."""
    from training import patch_routing as P
    u = dataset(root, [f'{clothes} {person}'], 'full', sleeve).unrouted(0)
    try:
        return u, P.normalize(*sample(u), 2, 'cpu', part='full')
    except np.linalg.LinAlgError as e:
        return u, e


def same(a, b):
    """Same dtype, shape and values; NaN (the skin medians of a person without skin pixels) equals NaN."""
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


# --------------------------------------------------------------------------------------------------- the pairs file

def test_pairs_file_lines_have_three_names_in_the_outfit_mode(pairs_root):
    ds = dataset(pairs_root, ['person_b.jpg dress_c.jpg person_a.jpg', '', 'person_a.jpg person_a.jpg dress_c.jpg'], 'outfit')
    assert len(ds) == 2
    u = ds.unrouted(0)
    assert (u['clothes_name'], u['lower_name'], u['person_name']) == ('person_b.jpg', 'dress_c.jpg', 'person_a.jpg')
    with pytest.raises(ValueError, match='person_b.jpg person_a.jpg'):
        dataset(pairs_root, ['person_b.jpg person_a.jpg'], 'outfit')
    with pytest.raises(ValueError, match='person_b.jpg dress_c.jpg person_a.jpg'):
        dataset(pairs_root, ['person_b.jpg dress_c.jpg person_a.jpg'], 'upper')
    with pytest.raises(ValueError, match='part'):
        dataset(pairs_root, ['person_b.jpg person_a.jpg'], 'shoes')


# --------------------------------------------------------------------------------------------------- identity 1

@pytest.mark.parametrize('which', ['pairs', 'crafted'])
def test_outfit_routing_with_the_clothes_own_keypoints_is_full(pairs_root, crafted_root, which):
    from training import patch_routing as P
    root = pairs_root if which == 'pairs' else crafted_root
    for clothes, person in listed_pairs(root):
        u, want = full_of(root, clothes, person)
        s = sample(u)
        for lower_kp in (s[5], None):
            if isinstance(want, Exception):
                with pytest.raises(np.linalg.LinAlgError):
                    P.normalize(*s, 2, 'cpu', part='outfit', lower_keypoints=lower_kp)
                continue
            got = P.normalize(*s, 2, 'cpu', part='outfit', lower_keypoints=lower_kp)
            assert len(got) == len(want) == 4 and all(same(g, w) for g, w in zip(got, want)), (clothes, person, lower_kp is None)
    with pytest.raises(ValueError, match='outfit'):
        P.normalize(*s, 2, 'cpu', part='full', lower_keypoints=s[5])


@pytest.mark.parametrize('which', ['pairs', 'crafted'])
def test_outfit_items_of_one_clothes_image_are_fulls_items(pairs_root, crafted_root, which):
    """``U U P`` lines: the first 16 entries are ``full``'s 16-tuple for ``U P`` -- over the crafted people too (a dress over pants, equal pants and skirt,
    the dress branches, no lower garment ...)."""
    root = pairs_root if which == 'pairs' else crafted_root
    pairs = listed_pairs(root)
    outfit = dataset(root, [f'{c} {c} {p}' for c, p in pairs], 'outfit', sleeve=True)
    full = dataset(root, [f'{c} {p}' for c, p in pairs], 'full', sleeve=True)
    for i, (c, p) in enumerate(pairs):
        try:
            want = full[i]
        except np.linalg.LinAlgError:                                      # (people without a routing in any mode: `full_of`)
            with pytest.raises(np.linalg.LinAlgError):
                outfit[i]
            continue
        got = outfit[i]
        assert len(got) == 18 and len(want) == 16
        for k in range(14):
            assert same(got[k], want[k]), (c, p, k)
        assert got[14:16] == want[14:16] == (p, c) and got[17] == c
        assert got[16].dtype == np.uint8 and np.array_equal(got[16], want[1])              # the lower clothes image, CHW: here the clothes


# --------------------------------------------------------------------------------------------------- identity 2

TRIPLES = [('pairs', 'person_b.jpg', 'person_a.jpg', 'dress_c.jpg'), ('pairs', 'dress_c.jpg', 'person_a.jpg', 'person_b.jpg'),
           ('crafted', 'edges.jpg', 'equal.jpg', 'base.jpg'), ('crafted', 'dresspants.jpg', 'toskirt.jpg', 'outside.jpg')]


@pytest.mark.parametrize('sleeve', [False, True])
@pytest.mark.parametrize('which,upper,lower,person', TRIPLES)
def test_outfit_is_fulls_upper_half_of_one_image_and_lower_half_of_the_other(pairs_root, crafted_root, which, upper, lower, person, sleeve):
    from training import patch_routing as P
    root = pairs_root if which == 'pairs' else crafted_root
    o = dataset(root, [f'{upper} {lower} {person}'], 'outfit', sleeve).unrouted(0)
    (fu, routed_u), (fl, routed_l) = full_of(root, upper, person, sleeve), full_of(root, lower, person, sleeve)
    ctx = (upper, lower, person, sleeve)
    assert (o['sleeve'] is None) == (not sleeve) and o['canvas'] is None and not o['bound'].any()
    for k in ('upper_img', 'upper_mask', 'clothes', 'clothes_kp', 'image', 'pose', 'retain_mask', 'person_kp') + (('sleeve',) if sleeve else ()):
        assert same(o[k], fu[k]), (ctx, k)
    assert np.array_equal(o['skin'], fu['skin'], equal_nan=True)
    for k, kl in (('lower_img', 'lower_img'), ('lower_mask', 'lower_mask'), ('lower_kp', 'clothes_kp'), ('lower_clothes', 'clothes')):
        assert same(o[k], fl[kl]), (ctx, k)
    assert o['lower_clothes'].dtype == np.uint8 and o['lower_clothes'].shape == (512, 512, 3)
    assert (o['clothes_name'], o['lower_name'], o['person_name']) == (upper, lower, person)
    got = P.normalize(*sample(o)[:7], 2, 'cpu', part='outfit', lower_keypoints=o['lower_kp'])
    assert len(got) == 4
    assert same(got[0], routed_u[0]) and same(got[2], routed_u[2]), ctx                    # norm_img, denorm_upper: full(U, P)'s
    assert same(got[1], routed_l[1]) and same(got[3], routed_l[3]), ctx                    # norm_img_lower, denorm_lower: full(L, P)'s
    batched = P.normalize_batch([sample(o)], 2, 'cpu', part='outfit')                      # the eighth entry of a sample is the lower key points
    assert all(same(b[0], g) for b, g in zip(batched, got)), ctx


# --------------------------------------------------------------------------------------------------- label and bound

@pytest.fixture(scope='module')
def table_root(tmp_path_factory):
    """pants_a / pants_b: a top and pants; skirt: the pants relabelled as a skirt; dress: a dress alone; top: a top and no lower garment."""
    root = str(tmp_path_factory.mktemp('outfit_table'))
    rng = np.random.default_rng(41)
    for name in ('pants_a', 'pants_b', 'skirt', 'top', 'someone'):
        _write_person(root, name, rng)
    _write_person(root, 'dress', rng, dress=True)
    lab = _labels(root, 'skirt')
    lab[lab == 9] = 12
    _set_labels(root, 'skirt', lab)
    lab = _labels(root, 'top')
    lab[lab == 9] = 0
    _set_labels(root, 'top', lab)
    return root


@pytest.mark.parametrize('upper,lower,label,routed', [('pants_a', 'pants_b', 0, True), ('pants_a', 'skirt', 1, True), ('dress', 'pants_b', 0, True),
                                                       ('dress', 'top', 2, False), ('pants_a', 'top', 1, False)])
def test_label_and_bound_of_an_outfit(table_root, upper, lower, label, routed):
    """L in pants: 0; L in a skirt: 1; U a dress and L in pants: 0, both garments routed (nothing is zeroed for a dress); U a dress and L without a lower
    garment: 2 and a bound of zeros; neither: 1."""
    from training import tryon
    from training.dataset import collate_unrouted
    ds = dataset(table_root, [f'{upper}.jpg {lower}.jpg someone.jpg'], 'outfit')
    item = ds[0]
    assert np.array_equal(item[12], np.full((1, 512, 512), label / 2.0 * 255))
    den_up, den_lo, bound = item[6], item[7], item[13]
    assert den_up.any() and den_lo.any() == routed and item[5].any() == routed
    want = np.zeros((1, 512, 512), np.uint8)
    if routed:
        want[:, np.flatnonzero(den_lo.any(axis=(0, 2)))[0]:] = 255                        # from the routed lower garment's first row on
    assert np.array_equal(bound, want)
    # the same through the batch route: the host part is zeros, `final_bound` and `_canvases` take the full mode's branch
    batch = collate_unrouted([ds.unrouted(0)])
    assert int(batch['label'][0]) == label and not batch['bound'].any() and batch['canvas'] is None
    routed_b, ext = tryon.route(batch, 'outfit')
    assert tryon._canvases(batch, routed_b, 'outfit')[2] is routed_b[3]
    assert np.array_equal(tryon.final_bound(batch['bound'], ext, batch['label'], 'outfit')[0].numpy(), want[0, :, 0])
    inp = tryon.batch_inputs(batch, routed_b, ext, 'outfit')
    assert torch.equal(inp['pose'][0, 4], torch.from_numpy(want[0]).float() / 127.5 - 1)


# --------------------------------------------------------------------------------------------------- the front on the CPU, the batches' keys

def _both(ds):
    from training.dataset import collate_raw, collate_unrouted
    idx = range(len(ds))
    return collate_raw([ds.raw(i) for i in idx]), collate_unrouted([ds.unrouted(i) for i in idx])


@pytest.mark.parametrize('sleeve', [False, True])
def test_front_batch_on_the_cpu_equals_the_host_loader_in_the_outfit_mode(pairs_root, sleeve):
    from training import tryon_front
    ds = dataset(pairs_root, ['person_b.jpg dress_c.jpg person_a.jpg', 'dress_c.jpg person_a.jpg person_b.jpg', 'person_a.jpg person_a.jpg dress_c.jpg'],
                 'outfit', sleeve)
    raw, want = _both(ds)
    assert list(want) == UNROUTED_KEYS[:11] + ['lower_clothes'] + UNROUTED_KEYS[11:] + ['lower_kp', 'lower_name']
    assert list(raw) == RAW_KEYS[:8] + ['lower_img', 'lower_parsing'] + RAW_KEYS[8:] + ['lower_kp', 'lower_name']
    assert raw['lower_img'].dtype == torch.uint8 and tuple(raw['lower_img'].shape) == (3, 512, 320, 3) and tuple(raw['lower_parsing'].shape) == (3, 512, 320)
    assert want['lower_clothes'].dtype == torch.uint8 and tuple(want['lower_clothes'].shape) == (3, 512, 512, 3)
    assert want['lower_name'] == ['dress_c.jpg', 'person_a.jpg', 'person_a.jpg'] and raw['lower_name'] == want['lower_name']
    assert all(np.array_equal(a, b) for a, b in zip(raw['lower_kp'], want['lower_kp']))
    assert_same_batch(tryon_front.front_batch(raw, 'outfit'), want, ('outfit', sleeve))


def test_front_batch_on_the_cpu_for_a_narrow_outfit(tmp_path):
    from training import tryon_front
    write_narrow(str(tmp_path))
    ds = dataset(str(tmp_path), ['narrow_b.jpg narrow_a.jpg narrow_a.jpg', 'narrow_a.jpg narrow_b.jpg narrow_b.jpg'], 'outfit', sleeve=True)
    raw, want = _both(ds)
    assert tuple(raw['lower_img'].shape) == (2, 512, 318, 3)
    assert_same_batch(tryon_front.front_batch(raw, 'outfit'), want, 'narrow outfit')


@pytest.mark.parametrize('part', ['upper', 'lower', 'full'])
def test_the_existing_modes_batches_keep_their_keys(pairs_root, part):
    from training import tryon_front
    from training.dataset import TryOnTestSet
    ds = TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu', part=part)
    raw, want = _both(ds)
    assert list(raw) == RAW_KEYS and list(want) == UNROUTED_KEYS
    assert not OUTFIT_RAW & (set(raw) | set(ds.raw(0))) and not OUTFIT_UNROUTED & (set(want) | set(ds.unrouted(0)))
    assert list(tryon_front.front_batch(raw, part)) == UNROUTED_KEYS
    assert len(ds[0]) == 16


# --------------------------------------------------------------------------------------------------- the four panels

def test_numpy_panels_are_the_triptychs_panels():
    from training import tryon
    fin, clothes, image = crafted_triptych_case()
    with np.errstate(invalid='ignore'):
        got = tryon.panels_numpy(fin, [clothes, clothes, image])
        want = tryon.triptych_numpy(fin, clothes, image)
    assert got.dtype == np.uint8 and got.shape == (2, 512, 1280, 3) and got.flags['C_CONTIGUOUS']
    assert np.array_equal(got[:, :, 0:320], want[:, :, 0:320]) and np.array_equal(got[:, :, 320:640], want[:, :, 0:320])
    assert np.array_equal(got[:, :, 640:], want[:, :, 320:])
    with np.errstate(invalid='ignore'):
        mixed = tryon.panels_numpy(fin, [clothes, image[::-1], image])                     # each panel reads its own source
        assert np.array_equal(mixed[:, :, 320:640], tryon.triptych_numpy(fin, image[::-1], image)[:, :, 0:320])
        assert torch.equal(tryon.panels(torch.from_numpy(fin), [torch.from_numpy(a) for a in (clothes, clothes, image)]), torch.from_numpy(got))
    assert tryon.result_name('a/person_1.jpg', 'top_2.jpg', 'b/skirt_3.png') == 'person_1___top_2___skirt_3.png'
    assert tryon.result_name('a/person_1.jpg', 'top_2.jpg') == 'person_1___top_2.png'


# --------------------------------------------------------------------------------------------------- the driver

def test_cpu_end_to_end_in_the_outfit_mode(pairs_root, tmp_path):
    from training import tryon
    G = _small_generator()                                                 # (the generator is what takes the time on a CPU: one line per run)
    ds = dataset(pairs_root, ['dress_c.jpg dress_c.jpg person_b.jpg'], 'outfit', sleeve=True)
    files = {front: tryon.run_tryon(ds, G, str(tmp_path / front), batch_size=1, device='cpu', workers=0, front=front) for front in ('host', 'native')}
    full = tryon.run_tryon(dataset(pairs_root, ['dress_c.jpg person_b.jpg'], 'full', sleeve=True), G, str(tmp_path / 'full'), batch_size=1, device='cpu')
    assert [os.path.basename(f) for f in files['host']] == [os.path.basename(f) for f in files['native']] == ['person_b___dress_c___dress_c.png']
    got, want = np.array(PIL.open(files['host'][0])), np.array(PIL.open(full[0]))
    assert got.dtype == np.uint8 and got.shape == (512, 1280, 3) and want.shape == (512, 960, 3)
    assert np.array_equal(got[:, 640:], want[:, 320:])                     # person | result: the full mode's
    assert np.array_equal(got[:, :320], want[:, :320]) and np.array_equal(got[:, 320:640], want[:, :320])
    with open(files['host'][0], 'rb') as fa, open(files['native'][0], 'rb') as fb:
        assert fa.read() == fb.read()


def test_cli_accepts_the_outfit_mode():
    from training import tryon
    a = tryon.parse_args(['--network', 'n.pkl', '--dataroot', 'd', '--testpart', 'outfit', '--outdir', 'o', '--front', 'native', '--precision', 'bf16'])
    assert (a.testpart, a.front, a.precision) == ('outfit', 'native', 'bf16')
    assert tryon.MODE_CODE['outfit'] == 3
    with pytest.raises(SystemExit):
        tryon.parse_args(['--network', 'n.pkl', '--dataroot', 'd', '--testpart', 'shoes', '--outdir', 'o'])
