"""The training-set loader on the CPU: `TrainSet` on a SYNTHETIC dataset directory in the reference's layout (two sub-datasets, one of them
MPV_512_320 with its ``_label.png`` parsing names, two random-mask files), its 19-tuple contract, ``normalize(part='train')`` and the whole item
against the test-side restatement (tests/train_loader_ref.py) bit for bit under an explicit list of decision records, the class-merging rules, the
decision sampler's distribution, `fetch_reference` and a `TrainFeed` round through ``StyleGAN2Loss.accumulate_gradients``.

PARITY UNPINNED against the reference's OpenCV rasterising and warps, as for the other modes (DESIGN.md sections 6d, 6g)."""

import json
import math
import os
import random

import numpy as np
import pytest
import torch

from test_dataset_loader import _write_person

PIL = pytest.importorskip('PIL.Image')

# (kind, rows, erase_length, u, use_random_mask): every branch of dataset.py:1160-1170 and :1226
RECORDS = [(0, 0, 0, 0.0, 1), (1, 0, 0, 0.0, 1), (1, 1, 7, 0.0, 0), (1, 1, 12, 0.0, 1), (2, 0, 0, 0.0, 1), (2, 0, 0, float(np.float32(1 - 2 ** -24)), 0),
           (2, 0, 0, 0.37, 1), (0, 0, 0, 0.0, 0)]
PERSONS = [('Zalando_512_320_v1', 'full_a', 'full'), ('Zalando_512_320_v1', 'dress_b', 'dress'), ('MPV_512_320', 'noleft_c', 'no_left_sleeve'),
           ('MPV_512_320', 'knee_d', 'low_knee')]


def write_train_person(root, name, rng, kind):
    """`_write_person`'s photo with long sleeves on the top (so that the sleeve parts hold pixels); 'no_left_sleeve': the garment parsing marks one
    sleeve only; 'low_knee': the left knee's confidence is 0.05 (part 7 goes missing); 'dress': a dress."""
    _write_person(root, name, rng, dress=kind == 'dress')
    path = os.path.join(root, 'parsing', name + '.png')
    lab = np.array(PIL.open(path))
    lab[112:270, 70:100] = lab[112:270, 220:250] = 6 if kind == 'dress' else 5
    PIL.fromarray(lab, 'L').save(path)
    gp = np.zeros((512, 320, 3), np.uint8)
    gp[112:270, 70:100, 0] = 10
    if kind != 'no_left_sleeve':
        gp[112:270, 220:250, 0] = 11
    PIL.fromarray(gp, 'RGB').save(os.path.join(root, 'garment_parsing', name + '.png'))
    if kind == 'low_knee':
        path = os.path.join(root, 'keypoints', name + '_keypoints.json')
        with open(path) as f:
            kp = json.load(f)
        kp['people'][0]['pose_keypoints_2d'][12 * 3 + 2] = 0.05
        with open(path, 'w') as f:
            json.dump(kp, f)


def write_train_root(root):
    rng = np.random.default_rng(21)
    for dataset in ('Zalando_512_320_v1', 'MPV_512_320'):
        sub = os.path.join(root, dataset)
        names = [(n, k) for d, n, k in PERSONS if d == dataset]
        for name, kind in names:
            write_train_person(sub, name, rng, kind)
            if dataset == 'MPV_512_320':
                os.rename(os.path.join(sub, 'parsing', name + '.png'), os.path.join(sub, 'parsing', name + '_label.png'))
        with open(os.path.join(sub, 'train_pairs_front_list_220508.txt'), 'w') as f:
            f.write(''.join(f'{n}.jpg {n}.jpg\n' for n, _ in names))
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    for i in range(2):
        m = np.zeros((512, 512), np.uint8)
        m[150 + 100 * i:330 + 100 * i, 200 - 40 * i:300] = 255
        m[40:60, 250:260] = 1 + i                              # any non-zero value erases
        PIL.fromarray(m, 'L').save(os.path.join(root, 'train_random_mask_acgpn', f'mask_{i}.png'))
    return root


@pytest.fixture(scope='module')
def train_root(tmp_path_factory):
    return write_train_root(str(tmp_path_factory.mktemp('train')))


@pytest.fixture(scope='module')
def train_set(train_root):
    from training.dataset import TrainSet
    return TrainSet(train_root, shuffle=False, device='cpu')


def index_of(ds, name):
    return [i for i, n in enumerate(ds.names) if name in n[0]][0]


SHAPES = [(3, 512, 512), (3, 512, 512), (30, 128, 128), (15, 128, 128), (15, 128, 128), (3, 512, 512), (3, 512, 512), (10, 3, 3), (10, 3, 3), (1, 512, 512),
          (1, 512, 512), (1, 512, 512), (30, 128, 128), (15, 128, 128), (1, 512, 512), (3, 512, 512), (1, 512, 512), (1, 512, 512), (1, 512, 512)]
FLOAT64 = (7, 8, 15, 16)


def test_listing_and_options(train_root):
    from training.dataset import TrainSet, DATASET_LIST
    assert len(DATASET_LIST) == 14
    ds = TrainSet(train_root, shuffle=False)
    assert len(ds) == 4 and ds.vis_index == [] and len(ds.random_masks) == 2
    assert [os.path.basename(n[2]) for n in ds.names] == ['full_a.png', 'dress_b.png', 'noleft_c_label.png', 'knee_d_label.png']
    a, b, c = (TrainSet(train_root, seed=s).names for s in (3, 3, 4))
    assert a == b and sorted(a) == sorted(ds.names) and (a != c or a != ds.names)
    assert len(TrainSet(train_root, dataset_list=['MPV_512_320'])) == 2
    with pytest.raises(IOError):
        TrainSet(train_root, dataset_list=['Zalora_512_320_v1'])


def test_tuple_contract(train_set):
    from training.dataset import EraseRecord
    for name, rec in (('full_a', RECORDS[3]), ('dress_b', RECORDS[4]), ('knee_d', RECORDS[7])):
        item = train_set.item(index_of(train_set, name), EraseRecord(*rec))
        assert len(item) == 19
        for i, (a, shape) in enumerate(zip(item, SHAPES)):
            assert tuple(a.shape) == shape and a.dtype == (np.float64 if i in FLOAT64 else np.uint8), (i, a.shape, a.dtype)
        (image, pose, norm_img, norm_lower, for_train, dup, dlo, Ms, M_invs, gt, mup, mlo, cm, cml, retain, skin, label, b_train, b_test) = item
        assert (image[:, :, :96] == 255).all() and (image[:, :, 416:] == 255).all()          # 320 -> 512 white side bars
        assert set(np.unique(gt)) <= set(range(7)) and {1, 5, 6} <= set(np.unique(gt)) | ({1} if name == 'dress_b' else set())
        for m in (mup, mlo, retain):
            assert set(np.unique(m)) <= {0, 1}
        assert set(np.unique(b_train)) <= {0, 255} and set(np.unique(b_test)) <= {0, 255}
        assert float(label.max()) == float(label.min()) and float(label.max()) in (0.0, 127.5, 255.0)
        assert np.array_equal(mup[0], (dup.astype(np.int64).sum(axis=0) > 0).astype(np.uint8))
        assert np.array_equal(mlo[0], (dlo.astype(np.int64).sum(axis=0) > 0).astype(np.uint8))
        assert pose.any() and np.isfinite(skin).all() and retain[0, 40:80, 96 + 140:96 + 180].all()
        if name == 'dress_b':
            assert float(label.max()) == 255.0 and 4 in np.unique(gt) and not b_train.any() and not dlo.any()
        else:
            assert float(label.max()) == 0.0 and 2 in np.unique(gt)
            assert (b_train[0, :, 0] == 255).argmax() == 290 and (b_test[0, :, 0] == 255).argmax() <= 290       # bbox top of the pants; the hip rule is never lower
        if name == 'knee_d':
            assert not Ms[7].any() and not M_invs[7].any() and Ms[6].any() and sum(bool(Ms[i].any()) for i in range(10)) == 9
        if name == 'full_a':
            assert all(Ms[i].any() for i in range(10))
            assert np.array_equal(for_train[3:6, 12:], norm_lower[3:6, 12:]) and not for_train[0:3].any() and not for_train[3:6, :12].any()


def _routing_args(u):
    return u['upper_img'], u['lower_img'], u['upper_mask'], u['lower_mask'], u['sleeve'], u['person_kp']


@pytest.fixture(scope='module')
def hosts(train_set):
    """Per person: the unrouted host item and the product's CPU routing (the routing does not depend on the record)."""
    from training import patch_routing as P
    from training.dataset import NO_ERASE
    out = {}
    for _, name, _ in PERSONS:
        u = train_set.unrouted(index_of(train_set, name), NO_ERASE)
        args = _routing_args(u)
        out[name] = (u, tuple(t.numpy() for t in P.normalize(*args, args[5], 2, device='cpu', part='train')))
    return out


@pytest.mark.parametrize('name', [p[1] for p in PERSONS])
def test_cpu_normalize_and_item_match_the_restatement_bit_for_bit(train_set, hosts, name, monkeypatch):
    import train_loader_ref as TR
    from training import patch_routing as P
    from training.dataset import EraseRecord
    u, got = hosts[name]
    idx = index_of(train_set, name)
    want = {rec: TR.normalize(*_routing_args(u), 2, rec) for rec in RECORDS[:1]}
    w = want[RECORDS[0]]
    for nm, g, w_ in zip(('img', 'img_lower', 'denorm_upper', 'denorm_lower', 'clothes_masks', 'clothes_masks_lower'), got, (w[0], w[1], w[3], w[4], w[7], w[8])):
        assert g.dtype == np.uint8 and g.shape == w_.shape and np.array_equal(g, w_), (name, nm)
    ms, m_invs = P.crop_matrices(u['person_kp'], 512, 512, 2)
    assert np.array_equal(ms, w[5]) and np.array_equal(m_invs, w[6])

    # non-vacuity (the issue's conditions)
    nonzero = lambda a, ii: bool(a[..., 3 * ii:3 * ii + 3].any())
    if name == 'full_a':
        assert sum(bool(w[5][ii].any()) for ii in range(10)) >= 8 and sum(nonzero(w[0], ii) for ii in range(10)) >= 8 and w[3].any() and w[4].any() and w[8][..., 0:3].any()
    if name == 'noleft_c':                                     # one top sleeve came out empty and was mirrored from the other side
        assert nonzero(w[7], 2) and nonzero(w[7], 4) and np.array_equal(w[7][..., 6:9], w[7][:, ::-1, 12:15]) and nonzero(w[0], 2)
    if name == 'knee_d':
        assert not w[5][7].any() and not nonzero(w[0], 7)

    # the whole item under every record: the routing is the record-independent part, so the product's is computed once and reused
    routed = tuple(torch.from_numpy(a) for a in got)
    monkeypatch.setattr(P, 'normalize', lambda *a, **k: routed)
    random_mask = np.array(PIL.open(train_set.random_masks[idx % 2]))[..., None]
    chw = lambda a: a.transpose(2, 0, 1)
    distinct = set()
    for rec in RECORDS:
        item = train_set.item(idx, EraseRecord(*rec))
        r = TR.normalize(*_routing_args(u), 2, rec) if rec in want else None
        if r is None:                                          # (the restatement's routing does not depend on the record either: re-run its erase only)
            r = _erase_only(TR, w, rec)
        up_e, lo_e, up_m, lo_m = TR.getitem_tail(chw(r[3]), chw(r[4]), random_mask, rec)
        for i, w_ in ((2, chw(r[0])), (3, chw(r[1])), (4, chw(r[2])), (5, up_e), (6, lo_e), (7, r[5]), (8, r[6]), (10, up_m), (11, lo_m), (12, chw(r[7])),
                      (13, chw(r[8]))):
            assert item[i].dtype == w_.dtype and np.array_equal(item[i], w_), (name, rec, i)
        distinct.add(item[4].tobytes() + item[5].tobytes())
    if name == 'full_a':
        assert len(distinct) == len(RECORDS)                   # every record of the list changes something
    if name == 'dress_b':
        assert len({d[:15 * 128 * 128] for d in distinct}) == 1 and not w[8][..., 0:3].any()        # empty routed lower mask: the erase is skipped


def _erase_only(TR, w, rec):
    """The restatement's result under another record: its erase block (:1146-1170) re-run on the routed patches of `w` (the statements before it do
    not read the record).  Checked against a full run for one record per person in `test_erase_only_equals_a_full_run`."""
    kind, rows, erase_length, u, _ = rec
    for_train = [w[1][..., 3 * k:3 * k + 3].copy() for k in range(5)]
    bbox = TR.mask_to_bbox(w[8][..., 0:1])
    h = w[1].shape[0]
    if bbox is not None:
        if kind == 1:
            for_train[0] = np.zeros_like(for_train[0])
            if rows:
                for_train[1][0:erase_length, ...] *= 0
                for_train[3][0:erase_length, ...] *= 0
        elif kind == 2:
            ty = bbox[1]
            by = min(ty + 1 + int(np.floor(np.float32(u) * np.float32(h - ty))), h)
            for_train[0][ty:by, ...] *= 0
    r = list(w)
    r[2] = np.concatenate(for_train, axis=2)
    return r


def test_erase_only_equals_a_full_run(hosts):
    import train_loader_ref as TR
    u, _ = hosts['full_a']
    base = TR.normalize(*_routing_args(u), 2, RECORDS[0])
    for rec in (RECORDS[3], RECORDS[6]):
        full = TR.normalize(*_routing_args(u), 2, rec)
        short = _erase_only(TR, base, rec)
        assert all(np.array_equal(a, b) for a, b in zip(full, short))
        assert not np.array_equal(full[2], base[2])


def test_band_covers_the_reference_range(hosts):
    """u = 0 erases one row (by = ty + 1), u just below 1 erases through the last row (by = h): randint(ty + 1, h)'s two ends."""
    from training.dataset import apply_erase, EraseRecord
    _, got = hosts['full_a']
    lower, masks = got[1], got[5]
    ty = int(np.nonzero(masks[..., 0].any(axis=1))[0][0])
    one = apply_erase(lower, masks, EraseRecord(*RECORDS[4]))
    assert lower[ty, :, 0:3].any() and not one[ty, :, 0:3].any() and np.array_equal(one[ty + 1:], lower[ty + 1:]) and np.array_equal(one[:ty], lower[:ty])
    allrows = apply_erase(lower, masks, EraseRecord(*RECORDS[5]))
    assert not allrows[ty:, :, 0:3].any() and np.array_equal(allrows[..., 3:], lower[..., 3:])


def _labels(**areas):
    """A 512 x 512 x 1 label map with a rows-high, 10-wide block per given LIP label."""
    lab = np.zeros((512, 512, 1), np.uint8)
    for i, (label, rows) in enumerate(areas.items()):
        lab[0:rows, 20 * i:20 * i + 10] = int(label[1:])
    return lab


@pytest.mark.parametrize('areas,want', [
    (dict(l9=30, l12=10, l5=20), dict(tops=200, dresses=0, pants=400, skirt=0)),                      # pants > skirt: the skirt joins the pants (:573-575)
    (dict(l9=10, l12=10, l5=20), dict(tops=200, dresses=0, pants=0, skirt=200)),                      # else (ties too): the pants join the skirt (:576-578)
    (dict(l9=30, l6=50, l5=20), dict(tops=700, dresses=0, pants=300, skirt=0)),                       # dress + pants: the dress is a top (:581-583)
    (dict(l6=50, l5=20, l12=10), dict(tops=0, dresses=800, pants=0, skirt=0)),                        # dress larger than top + skirt: swallows both (:585-588)
    (dict(l6=20, l5=30, l12=10), dict(tops=300, dresses=0, pants=0, skirt=300)),                      # smaller dress, top > skirt: joins the skirt (:590-591)
    (dict(l6=20, l5=10, l12=30), dict(tops=300, dresses=0, pants=0, skirt=300)),                      # smaller dress, top <= skirt: joins the top (:592-593)
    (dict(l5=10, l7=10), dict(tops=200, dresses=0, pants=0, skirt=0)),                                # no dress: untouched; label 7 is a top too
])
def test_class_merging_rules(areas, want):
    from training.dataset import _garment_classes
    tops, dresses, pants, skirt = _garment_classes(_labels(**areas))
    assert dict(tops=int(tops.sum()), dresses=int(dresses.sum()), pants=int(pants.sum()), skirt=int(skirt.sum())) == want


def test_decision_sampler_distribution_and_reproducibility():
    from training.dataset import sample_record, ERASE_NONE, ERASE_DROP_PART0, ERASE_BAND
    n, h = 20000, 128
    draw = lambda seed: [sample_record(random.Random(f'{seed}/{i}'), h) for i in range(n)]
    recs = draw(0)
    assert recs == draw(0) and recs != draw(1)

    def within(count, total, p):                               # five binomial standard deviations
        return abs(count - total * p) <= 5 * math.sqrt(total * p * (1 - p))
    kinds = [r.kind for r in recs]
    assert within(kinds.count(ERASE_NONE), n, 0.20) and within(kinds.count(ERASE_DROP_PART0), n, 0.48) and within(kinds.count(ERASE_BAND), n, 0.32)
    drops = [r for r in recs if r.kind == ERASE_DROP_PART0]
    assert within(sum(r.rows for r in drops), len(drops), 0.75)
    assert within(sum(r.use_random_mask for r in recs), n, 0.9)
    lengths = {r.erase_length for r in drops if r.rows}
    assert lengths == set(range(1, h // 10 + 1)) and all(r.erase_length == 0 for r in recs if not r.rows)
    assert all(0.0 <= r.u < 1.0 and float(np.float32(r.u)) == r.u for r in recs) and all(r.u == 0.0 for r in recs if r.kind != ERASE_BAND)


def test_dataset_draws_reproducible_records(train_root):
    from training.dataset import TrainSet
    a, b = TrainSet(train_root, seed=5), TrainSet(train_root, seed=5)
    ra = [a.record(i) for i in (0, 1, 0, 0, 2)]
    assert ra == [b.record(i) for i in (0, 1, 0, 0, 2)] and len({ra[0], ra[2], ra[3]}) > 1
    assert ra != [TrainSet(train_root, seed=6).record(i) for i in (0, 1, 0, 0, 2)]


def _host_batch(ds, records=RECORDS[:4]):
    from training.dataset import EraseRecord, collate_train
    return collate_train([ds.unrouted(i % len(ds), EraseRecord(*rec)) for i, rec in enumerate(records)])


def test_fetch_reference_shapes_and_values_on_cpu(train_set):
    from training import train_fetch as F
    batch = _host_batch(train_set)
    routed, ext = F.route(batch)
    out = F.fetch_reference(batch, routed, ext)
    n = 4
    shapes = dict(real_img=(n, 3, 512, 512), style_input=(n, 45, 128, 128), retain=(n, 6, 512, 512), pose=(n, 5, 512, 512),
                  denorm_upper_input=(n, 3, 512, 512), denorm_lower_input=(n, 3, 512, 512), denorm_upper_mask=(n, 1, 512, 512),
                  denorm_lower_mask=(n, 1, 512, 512), gt_parsing=(n, 1, 512, 512))
    assert set(out) == set(shapes) == set(F.KEYS)
    for k, shape in shapes.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == torch.float32, k
    assert float(out['real_img'].min()) >= -1 and float(out['real_img'].max()) == 1.0
    assert set(out['gt_parsing'].unique().tolist()) <= set(range(7)) and set(out['denorm_upper_mask'].unique().tolist()) == {0.0, 1.0}
    # against the loader's own 19-tuple under the same records (the float statements applied to it)
    from training.dataset import EraseRecord
    for i, rec in enumerate(RECORDS[:4]):
        item = train_set.item(i, EraseRecord(*rec))
        unit = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32) * float(F._INV) - 1
        assert torch.equal(out['style_input'][i], torch.cat([unit(item[2]), unit(item[4])]))
        assert torch.equal(out['denorm_upper_input'][i], unit(item[5])) and torch.equal(out['denorm_lower_input'][i], unit(item[6]))
        assert torch.equal(out['denorm_lower_mask'][i], torch.from_numpy(item[11]).float())
        assert torch.equal(out['pose'][i], torch.cat([unit(item[1]), unit(item[16]), unit(item[17])]))
        assert torch.equal(out['retain'][i, 3:], unit(item[15])) and torch.equal(out['gt_parsing'][i], torch.from_numpy(item[9]).float())


def test_train_feed_rounds_go_through_the_loss(train_set):
    """`TrainFeed(device='cpu')` -> two rounds of batch 2, accepted by ``StyleGAN2Loss.accumulate_gradients`` (narrow networks, one phase)."""
    import stubs
    from training import train_fetch as F
    from training.loss import StyleGAN2Loss

    class Style45(stubs.StubStyleEncoding):                    # the stubs' encoders at the loader's channel counts
        def __init__(self):
            super().__init__()
            self.conv, self.feat = torch.nn.Conv2d(45, 3, 3, padding=1), torch.nn.Conv2d(6, 3, 1)

        def forward(self, style_input, retain):
            return self.fc(torch.tanh(self.conv(style_input)).mean(dim=(2, 3))), [self.feat(retain)]
    feed = F.TrainFeed(train_set, batch_gpu=2, rounds=2, seed=1, workers=0, device='cpu', z_dim=0)
    rounds = next(feed)
    assert len(rounds) == 2 and all(set(r) == set(F.KEYS) | {'gen_z'} for r in rounds)
    assert all(r['real_img'].shape == (2, 3, 512, 512) and r['gen_z'].shape == (2, 0) and r['style_input'].shape == (2, 45, 128, 128) for r in rounds)
    nets = stubs.build()
    torch.manual_seed(0)
    nets['G_style_encoding'] = Style45()
    loss = StyleGAN2Loss(device=torch.device('cpu'), **nets, augment_pipe=None, style_mixing_prob=0, r1_gamma=10, pl_weight=0, l1_weight=50,
                         vgg_weight=0, contextual_weight=0, mask_weight=1.0)
    stubs.set_phase_trainable(nets, 'Dmain')
    for r in rounds:
        loss.accumulate_gradients(phase='Dmain', sync=True, gain=1, **r)
    grads = [p.grad for p in nets['D'].parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(float(g.abs().sum()) > 0 for g in grads)
