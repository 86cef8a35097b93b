"""The try-on driver (training/tryon.py) without a GPU: the loader's unrouted half + batched CPU routing + the CPU inputs route against the existing
per-sample loader and ``to_generator_inputs``; the NumPy triptych against a restatement of test.py:162-181; a CPU end-to-end run writing the reference's
PNGs; ``build_generator`` on a snapshot in the reference's persistence wire format; the command line of test.sh."""

import os
import pickle
import shlex
import sys
import types

import numpy as np
import pytest
import torch

PIL = pytest.importorskip('PIL.Image')

from test_dataset_loader import _write_person  # noqa: E402

PARTS = ['upper', 'lower', 'full']


@pytest.fixture(scope='module')
def pairs_root(tmp_path_factory):
    """Three pairs: two people in top + pants, one in a dress; the dress is worn by the clothes of pair 2 and by the person of pair 3."""
    root = str(tmp_path_factory.mktemp('tryon_pairs'))
    rng = np.random.default_rng(11)
    _write_person(root, 'person_a', rng)
    _write_person(root, 'person_b', rng)
    _write_person(root, 'dress_c', rng, dress=True)
    with open(os.path.join(root, 'test_pairs.txt'), 'w') as f:
        f.write('person_b.jpg person_a.jpg\ndress_c.jpg person_b.jpg\nperson_a.jpg dress_c.jpg\n')
    return root


def _unrouted_batch(ds, idx):
    from training.dataset import collate_unrouted
    return collate_unrouted([ds.unrouted(i) for i in idx])


def _loader_batch(ds, idx):
    return torch.utils.data.default_collate([ds[i] for i in idx])


# --------------------------------------------------------------------------------------------------- 1. inputs: two paths, bit for bit

@pytest.mark.parametrize('sleeve', [False, True])
@pytest.mark.parametrize('part', PARTS)
def test_unrouted_path_gives_the_loaders_generator_inputs(pairs_root, part, sleeve):
    from training.dataset import TryOnTestSet, to_generator_inputs
    from training import tryon
    ds = TryOnTestSet(pairs_root, use_sleeve_mask=sleeve, device='cpu', part=part)
    idx = list(range(len(ds)))
    batch = _unrouted_batch(ds, idx)
    assert batch['image'].dtype == torch.uint8 and tuple(batch['image'].shape) == (3, 512, 512, 3)
    assert tuple(batch['bound'].shape) == (3, 512) and batch['skin'].dtype == torch.float32 and batch['label'].dtype == torch.int32
    assert (batch['canvas'] is None) == (part == 'full') and (batch['sleeve'] is None) == (not sleeve)
    routed, ext = tryon.route(batch, part)
    got = tryon.batch_inputs(batch, routed, ext, part)

    want_batch = _loader_batch(ds, idx)
    want = to_generator_inputs(want_batch, 'cpu')
    rebuilt = tryon.loader_tuple(batch, routed, ext, part)
    for k, (a, b) in enumerate(zip(rebuilt, want_batch[:14])):
        if k == 3:                                                       # clothes_pose: not read by the generator, not rebuilt
            continue
        assert a.dtype == b.dtype and torch.equal(a, b), (part, sleeve, 'loader entry', k)
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (part, sleeve, k)
    assert batch['person_name'] == list(want_batch[14]) and batch['clothes_name'] == list(want_batch[15])
    if part == 'full':
        assert int(batch['label'][1]) == 2                               # the dress outfit: its bound plane is zero
        assert torch.equal(tryon.final_bound(batch['bound'], ext, batch['label'], part)[1], torch.zeros(512, dtype=torch.uint8))


def test_final_bound_rules_on_arbitrary_rows():
    from training import tryon
    g = torch.Generator().manual_seed(3)
    rows = torch.randint(0, 256, (6, 512), generator=g, dtype=torch.int32).to(torch.uint8)
    ext = torch.tensor([[-1, -1], [0, 0], [10, 200], [511, 511], [0, 511], [300, 301]], dtype=torch.int32)
    label = torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32)
    for part in PARTS:
        got = tryon.final_bound(rows, ext, label, part)
        for i in range(6):
            b = rows[i].numpy()[:, None, None].copy()                    # the loader's statements on a [512, 1, 1] bound
            lo, hi = int(ext[i, 0]), int(ext[i, 1])
            if part == 'upper' and hi >= 0:
                b[0:hi] *= 0
            if part == 'full':
                if lo >= 0:
                    b[lo:] += 255
                if int(label[i]) == 2:
                    b = b * 0
            assert np.array_equal(got[i].numpy(), b[:, 0, 0]), (part, i)


def test_row_extents_cpu_match_the_loaders_bbox():
    from training import tryon
    from training.dataset import _bbox
    c = np.zeros((5, 512, 512, 3), np.uint8)
    c[1, 0, 7, 2] = 1
    c[2, 511, 511, 0] = 255
    c[3, 40:300, 100:200] = 9
    c[4, 0, 0, 0] = 3
    c[4, 511, 3, 1] = 3
    got = tryon.row_extents(torch.from_numpy(c))
    for i in range(5):
        bb = _bbox((c[i].sum(axis=2, keepdims=True) > 0).astype(np.uint8))
        assert got[i].tolist() == ([-1, -1] if bb is None else [bb[1], bb[3]]), i


# --------------------------------------------------------------------------------------------------- 2. triptych against test.py

def _test_py_triptych(gen_imgs, clothes_u8, image_u8):
    """test.py:127-181 for a batch, statement by statement: the tensors are built as torch builds them on a GPU (``u / 127.5`` is ``u * (1.0f /
    127.5f)`` there: tests/test_tryon_gpu.py pins it), cv2's BGR write undone, and the documented NaN rule (0) applied to the result column."""
    inv = np.float32(1.0) / np.float32(127.5)
    image_tensor = image_u8.transpose(0, 3, 1, 2).astype(np.float32) * inv - np.float32(1)
    clothes_tensor = clothes_u8.transpose(0, 3, 1, 2).astype(np.float32) * inv - np.float32(1)
    out = []
    for ii in range(gen_imgs.shape[0]):
        gen_img = gen_imgs[ii]
        gen_img = (gen_img.transpose(1, 2, 0) + 1.0) * 127.5
        gen_img = np.clip(gen_img, 0, 255)
        gen_img[np.isnan(gen_img)] = 0
        gen_img = gen_img.astype(np.uint8)[..., [2, 1, 0]]
        image_np = image_tensor[ii]
        image_np = (image_np.transpose(1, 2, 0) + 1.0) * 127.5
        image_np = image_np.astype(np.uint8)[..., [2, 1, 0]]
        clothes_np = clothes_tensor[ii]
        clothes_np = (clothes_np.transpose(1, 2, 0) + 1.0) * 127.5
        clothes_np = clothes_np.astype(np.uint8)[..., [2, 1, 0]]
        result = np.concatenate([clothes_np[:, 96:416, :], image_np[:, 96:416, :], gen_img[:, 96:416, :]], axis=1)
        out.append(result[..., [2, 1, 0]])                              # cv2.imwrite stores BGR arrays as RGB files
    return np.stack(out)


def crafted_triptych_case(n=2, seed=0):
    """Every byte value in the kept columns of clothes and person; results at +-1, +-1 +- 1 ulp, beyond the clip range, +-inf, NaN, and random values."""
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)
    clothes = rng.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)
    every = np.arange(256, dtype=np.uint8).repeat(3).reshape(256, 3)
    image[0, 0, 96:96 + 256] = every
    clothes[0, 1, 96:96 + 256] = every[::-1]
    fin = rng.uniform(-1.2, 1.2, (n, 3, 512, 512)).astype(np.float32)
    one = np.float32(1)
    specials = np.array([1, -1, np.nextafter(one, 2), np.nextafter(one, 0), np.nextafter(-one, -2), np.nextafter(-one, 0), 0, -0.0, 1e30, -1e30,
                         np.inf, -np.inf, np.nan, 3.0, -3.0, 1e-45, 0.99607843, -0.99607843], dtype=np.float32)
    fin[0, :, 5, 96:96 + specials.size] = specials
    fin[-1, 1, 511, 400:400 + specials.size] = specials
    k = np.arange(256, dtype=np.float32)                                  # the byte boundaries of the result column
    fin[-1, 2, 7, 96:96 + 256] = k / np.float32(127.5) - np.float32(1)
    return fin, clothes, image


def test_numpy_triptych_equals_test_py():
    from training import tryon
    fin, clothes, image = crafted_triptych_case()
    with np.errstate(invalid='ignore'):
        got = tryon.triptych_numpy(fin, clothes, image)
        want = _test_py_triptych(fin, clothes, image)
    assert got.dtype == np.uint8 and got.shape == (2, 512, 960, 3)
    assert np.array_equal(got, want)
    # the source columns reproduce the round trip, one below for some bytes, never more
    person = got[0, 0, 320:320 + 256, 0].astype(int)
    assert np.all((person == np.arange(256)) | (person == np.arange(256) - 1)) and np.any(person != np.arange(256))
    assert got[0, 5, 320 * 2 + 12, 0] == 0                                # NaN -> 0
    assert got[0, 5, 320 * 2 + 10, 1] == 255 and got[0, 5, 320 * 2 + 11, 1] == 0     # +-inf clip


# --------------------------------------------------------------------------------------------------- 3. CPU end to end

def _small_generator():
    from training import networks as PN
    from detgen import fill_module_
    return fill_module_(PN.GeneratorFull_v20(z_dim=0, c_dim=512, w_dim=64, img_resolution=512, img_channels=3, mapping_kwargs=dict(num_layers=1),
                                             synthesis_kwargs=dict(channel_base=4096, channel_max=512, conv_clamp=256)), 'tryon.').eval()


def test_cpu_end_to_end_writes_the_reference_images(pairs_root, tmp_path):
    from training.dataset import TryOnTestSet, to_generator_inputs
    from training import tryon
    ds = TryOnTestSet(pairs_root, use_sleeve_mask=True, device='cpu', part='upper')
    G = _small_generator()
    files = tryon.run_tryon(ds, G, str(tmp_path), batch_size=2, device='cpu', workers=0)
    assert [os.path.basename(f) for f in files] == ['person_a___person_b.png', 'person_b___dress_c.png', 'dress_c___person_a.png']
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(f) for f in files)
    want = []
    for idx in ([0, 1], [2]):                                            # test.py's flow on the loader's own 16-tuples, batched the same way
        batch = _loader_batch(ds, idx)
        with torch.no_grad():
            _, fin, _ = G(**to_generator_inputs(batch, 'cpu'), noise_mode='const')
        want.extend(_test_py_triptych(fin.numpy(), batch[1].permute(0, 2, 3, 1).numpy(), batch[0].permute(0, 2, 3, 1).numpy()))
    for f, w in zip(files, want):
        got = np.array(PIL.open(f))
        assert got.dtype == np.uint8 and got.shape == (512, 960, 3) and np.array_equal(got, w), f


# --------------------------------------------------------------------------------------------------- 4. build_generator

def _snapshot_blob(G, class_name, init_kwargs, module_src, monkeypatch):
    """G pickled the way the reference's torch_utils.persistence writes a persistent network: every module reduces to
    ``_reconstruct_persistent_obj(dict(type='class', version, module_src, class_name, state))`` with the module's __dict__ as state, init kwargs
    as dnnlib.util.EasyDict."""
    fake = types.ModuleType('torch_utils.persistence')

    def _reconstruct_persistent_obj(meta):
        raise AssertionError('the writer side is never called')
    _reconstruct_persistent_obj.__module__ = 'torch_utils.persistence'
    _reconstruct_persistent_obj.__qualname__ = '_reconstruct_persistent_obj'
    fake._reconstruct_persistent_obj = _reconstruct_persistent_obj
    monkeypatch.setitem(sys.modules, 'torch_utils.persistence', fake)
    util = types.ModuleType('dnnlib.util')

    class EasyDict(dict):
        pass
    EasyDict.__module__, EasyDict.__qualname__ = 'dnnlib.util', 'EasyDict'
    util.EasyDict = EasyDict
    monkeypatch.setitem(sys.modules, 'dnnlib.util', util)

    class _P:
        def __init__(self, meta):
            self.meta = meta

        def __reduce__(self):
            return (_reconstruct_persistent_obj, (self.meta,))

    def record(m, name, kwargs):
        state = dict(training=False, _parameters=dict(m._parameters), _buffers=dict(m._buffers),
                     _non_persistent_buffers_set=set(m._non_persistent_buffers_set),
                     _modules={k: (record(v, type(v).__name__, {}) if v is not None else None) for k, v in m._modules.items()},
                     _init_args=(), _init_kwargs=kwargs)
        return _P(dict(type='class', version=6, module_src=module_src, class_name=name, state=state))

    ed = lambda d: EasyDict({k: ed(v) if isinstance(v, dict) else v for k, v in d.items()})
    return pickle.dumps(dict(G=None, D=None, G_ema=record(G, class_name, ed(init_kwargs)), augment_pipe=None))


def test_build_generator_from_a_reference_snapshot(tmp_path, monkeypatch):
    from training import networks as PN
    from training import tryon
    from detgen import fill_module_
    kw = dict(z_dim=0, w_dim=512, mapping_kwargs=dict(num_layers=2),
              synthesis_kwargs=dict(channel_base=2048, channel_max=512, num_fp16_res=3, conv_clamp=256, use_noise=False),
              c_dim=512, img_resolution=512, img_channels=3)                 # train.py:191-202 + the training loop's common kwargs
    G = fill_module_(PN.GeneratorFull_v20(**kw), 'snap.')
    marker = tmp_path / 'executed'
    src = f"open({str(marker)!r}, 'w').write('x')\nclass GeneratorFull_v20: pass\n"
    path = tmp_path / 'network-snapshot-000000.pkl'
    path.write_bytes(_snapshot_blob(G, 'GeneratorFull_v20', kw, src, monkeypatch))
    other = tmp_path / 'other.pkl'
    other.write_bytes(_snapshot_blob(G, 'Generator', kw, src, monkeypatch))
    monkeypatch.undo()                                                   # the reader runs without the writer's stand-ins

    got = tryon.build_generator(str(path), 'cpu')
    assert not marker.exists()
    assert isinstance(got, PN.GeneratorFull_v20) and not got.training
    want, have = G.state_dict(), got.state_dict()
    assert list(have) == list(want)
    assert all(torch.equal(have[k], want[k]) for k in want)
    assert got.synthesis.num_ws == G.synthesis.num_ws and got.mapping.w_dim == 512
    with pytest.raises(ValueError, match='GeneratorFull_v20'):
        tryon.build_generator(str(other), 'cpu')
    assert not marker.exists()


# --------------------------------------------------------------------------------------------------- 5. the command line

TEST_SH = [
    '--dataroot test_datas --testtxt test_pairs.txt --network checkpoints/pasta-gan++/network-snapshot-004408.pkl --outdir test_results/upper '
    '--batchsize 1 --testpart upper --use-sleeve-mask',
    '--dataroot test_datas --testtxt test_pairs.txt --network checkpoints/pasta-gan++/network-snapshot-004408.pkl --outdir test_results/lower '
    '--batchsize 1 --testpart lower --use-sleeve-mask',
    '--dataroot test_datas --testtxt test_pairs.txt --network checkpoints/pasta-gan++/network-snapshot-004408.pkl --outdir test_results/full '
    '--batchsize 1 --testpart full --use-sleeve-mask',
]


def test_cli_accepts_the_reference_command_lines():
    from training import tryon
    for line, part in zip(TEST_SH, PARTS):
        a = tryon.parse_args(shlex.split(line))
        assert (a.dataroot, a.testtxt, a.testpart, a.batchsize, a.use_sleeve_mask) == ('test_datas', 'test_pairs.txt', part, 1, True)
        assert a.network.endswith('network-snapshot-004408.pkl') and a.outdir == 'test_results/' + part
        assert a.device == 'cuda' and a.workers == 0
    a = tryon.parse_args(shlex.split(TEST_SH[0] + ' --trunc 0.7 --seeds 1-3 --class 2 --noise-mode random --projected-w w.npz --device cpu --workers 3'))
    assert (a.device, a.workers) == ('cpu', 3)
    with pytest.raises(SystemExit):
        tryon.parse_args(shlex.split(TEST_SH[0].replace('--testpart upper', '--testpart shoes')))
