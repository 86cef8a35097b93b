"""No result depends on the previous contents of a tensor the product allocates (DESIGN "Fresh memory").

Every launch is run three times: twice from ordinary memory (identical bits required) and once with every `torch.empty*` of the product filled with NaN / the
integer maximum (`poisoned_alloc.poisoned_empty`), packs and caches rebuilt under the fill.  The poisoned result must be finite and bit-identical to the plain
one.  No tolerance anywhere.  The kernel rows of `test_nonfinite_locality.ROWS` are reused as they are; the rows below add what that table does not have.

Plugin export -> row (the `*_abi_version`, `*_packed_size`, `*_plan`, `*_workspace`, `*_blocks`, `*_chunk`, `*_last_route`, `reserve_cus`, `debug_stamps`
exports are exempt, and so is the size query
pg_conv2d_winograd4_stats_tiles; [L] = a row of the locality table):

  pg_bias_act                        bias_act_4d, bias_act_2d, bias_act_grad_4d, bias_act_grad_2d
  pg_bias_act_grad_bias              bias_act_grad_4d, bias_act_grad_2d
  pg_upfirdn2d                       [L] fir_up2, fir_down2, fir_blur*, fir_*_channels_last; fir_generic, fir_after_up2
  pg_upfirdn2d_with_odd_samples      [L] fir_shared_full, fir_shared_odd; fir_shared_odd_extents
  pg_upfirdn2d_bias_act              [L] fir_bias_act*; fir_bias_act_after_up2
  pg_conv2d_pack_weight              [L] direct_*; every fp32 row below that packs
  pg_conv2d_forward                  [L] direct_*, two_source, stream_1x1*; strided_out_f32
  pg_conv2d_forward_splitk           [L] direct_splitk; splitk_tail
  pg_conv2d_winograd_pack_weight     [L] wino_*
  pg_conv2d_winograd_forward         [L] wino_*; f4_stats
  pg_instance_norm_finish            f4_stats
  pg_modconv_dcoefs                  modconv_dcoefs
  pg_modconv_w2                      modconv_w2
  pg_modconv_prep                    modconv_prep_plain, modconv_prep_normalize, modconv_prep_half, modconv_prep_max
  pg_modconv_prep_batched            modconv_prep_batched, modconv_prep_batched_half
  pg_conv2d_up2_forward              [L] up2_fp32; up2_mod
  pg_conv2d_up2_forward_splitk       [L] up2_splitk
  pg_conv2d_up2x3_pack_weight        [L] up2_x3_edge_column, up2_x3_edge_gather
  pg_conv2d_up2x3_forward            [L] up2_x3_edge_column, up2_x3_edge_gather; fir_after_up2
  pg_conv2d_stem7x3_pack_weight      [L] stem7, stem7_wide
  pg_conv2d_stem7x3_forward          [L] stem7, stem7_wide
  pg_conv2d_s2x3_pack_weight         [L] s2x3
  pg_conv2d_s2x3_forward             [L] s2x3
  pg_conv1x1_small                   small_plain, small_full, small_split
  pg_conv1x1_fold_prep               fold_two_outputs, fold_one_output, fold3x3
  pg_conv1x1_fold_heads              fold_two_outputs, fold_one_output
  pg_conv3x3_fold_head               fold3x3
  pg_conv3x3_cin1                    cin1
  pg_instance_norm_stats             in_stats
  pg_spade_norm                      spade_norm
  pg_instance_norm_stats_cl16        in_stats16
  pg_spade_combine_cl16              spade_combine16
  pg_spade_train_forward             spade_train_forward
  pg_spade_train_backward            spade_train_backward_both, spade_train_backward_dx, spade_train_backward_dgb
  pg_spade_masked_sums               spade_feat_assemble
  pg_spade_feat_assemble             spade_feat_assemble
  pg_conv2d_wgrad                    [L] wgrad_3x3_*, wgrad_1x1; wgrad_splits
  pg_conv2d16_wgrad                  wgrad16
  pg_split3_bf16_cl                  [L] wgrad_bf16x3_*; wgrad_bf16x3_splits
  pg_conv2d16_wgrad_x3               [L] wgrad_bf16x3_*; wgrad_bf16x3_splits
  pg_conv2d16_pack_weight            [L] bf16_*; every 16-bit row below that packs
  pg_conv2d16_pack_weight_grouped    pack16_grouped
  pg_conv2d16_pack_weight_batched    pack16_batched
  pg_conv2d16_forward                [L] bf16_k3s1, bf16_k1s1, bf16_k3s2; strided_out_16
  pg_conv2d16_forward_splitk         splitk16
  pg_conv2d16_up2_fused              [L] bf16_up2f
  pg_conv1x1_small16                 small16, head16, head16_skip_up2
  pg_adam_flat_step                  flat_adam_step; route training_step
  pg_maxpool2x2, pg_maxpool2x2_backward            vgg_maxpool
  pg_l1_pair_sum, pg_l1_pair_grad    vgg_l1_pair
  pg_augment_warp, pg_augment_warp_adjoint         augment_warp, augment_warp_tiles
  pg_augment_color                   augment_color, augment_color_tiles
  pg_augment_late                    augment_late, augment_late_tiles
  pg_image_pair_metrics_u8           image_metrics
  pg_region_pair_metrics_u8          region_metrics
  pg_label_confusion_u8              label_confusion
  pg_tryon_front_stats, pg_tryon_front_bit_rows, pg_tryon_front_compose      test_fresh_memory_tryon_front; route tryon_batch
  pg_tryon_row_extent_u8, pg_tryon_inputs          tryon_inputs_upper, tryon_inputs_full; route tryon_batch
  pg_tryon_triptych_u8               tryon_triptych; route tryon_batch
  pg_tryon_panels_u8                 tryon_panels
  pg_train_fetch                     train_fetch
  pg_warp_perspective_u8             test_fresh_memory_patch_normalize (batched and single-sample), snapshot_warp; route tryon_batch
  pg_patch_compose_u8_k              test_fresh_memory_patch_normalize (single-sample route)
  pg_patch_compose_ordered_u8_k      test_fresh_memory_patch_normalize (batched route); route tryon_batch
  pg_patch_denorm_u8                 snapshot_denorm
  pg_snapshot_cells_u8               snapshot_cells
  the transposed convolutions        [L] transposed_phases; transposed16, transposed_wgrad, transposed_wgrad16 (no export of their own: the forward launches and the
                                     weight gradient with x and dy swapped)
  without a row: pg_patch_compose_u8 and pg_patch_compose_ordered_u8 -- the fixed-window forms the `_k` exports replaced; no Python code calls them.
"""

import math

import pytest
import torch

from poisoned_alloc import check_fill, poisoned_empty
from test_nonfinite_locality import ROWS, _bits, _plain

DEV = 'cuda'


def test_poisoned_empty_fills_and_restores_cpu():
    check_fill('cpu')


@pytest.mark.gpu
def test_poisoned_empty_fills_and_restores_gpu():
    assert torch.cuda.is_available(), 'this test needs the MI355X'
    check_fill(DEV)
    # a recycled block of the caching allocator: allocate, fill with 1, free, allocate the same size under the manager
    for dt in (torch.float32, torch.bfloat16):
        t = torch.ones([1 << 16], dtype=dt, device=DEV)
        ptr = t.data_ptr()
        del t
        with poisoned_empty():
            u = torch.empty([1 << 16], dtype=dt, device=DEV)
            assert u.data_ptr() == ptr, 'the allocator did not hand the freed block back: the test does not show what it is about'
            assert bool(torch.isnan(u).all())
    t = torch.ones([1 << 16], dtype=torch.int32, device=DEV)
    del t
    with poisoned_empty():
        assert bool((torch.empty([1 << 16], dtype=torch.int32, device=DEV) == torch.iinfo(torch.int32).max).all())


@pytest.fixture(scope='module')
def native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import conv2d_mfma
    assert conv2d_mfma._init() is not None


# ---------------------------------------------------------------------------------------------------------------- comparison

def _flat(out, prefix='y'):
    """The tensors of a result (tensor, None, tuple / list / dict of results) as [(name, CPU tensor)]; a pitched view becomes its logical extent."""
    if out is None:
        return []
    if torch.is_tensor(out):
        return [(prefix, out.detach().cpu().contiguous())]
    if isinstance(out, dict):
        return [p for k, v in out.items() for p in _flat(v, f'{prefix}.{k}')]
    return [p for i, v in enumerate(out) for p in _flat(v, f'{prefix}[{i}]')]


def _same(a, b, what):
    """a, b: lists of `_flat`."""
    assert [(n, t.shape, t.dtype) for n, t in a] == [(n, t.shape, t.dtype) for n, t in b], what
    assert a, f'{what}: no output to compare'
    for (name, u), (_, v) in zip(a, b):
        if u.dtype == torch.float64:
            bad = u.view(torch.int64) != v.view(torch.int64)
        elif u.dtype.is_floating_point:
            bad = _bits(u) != _bits(v)
        else:
            bad = u != v
        if bool(bad.any()):
            i = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f'{what}: {name} differs in {int(bad.sum())} of {bad.numel()} elements, first at {list(i)}: {u[i].item()} against {v[i].item()} '
                                 f'({int(torch.isnan(u.float()).sum()) if u.dtype.is_floating_point else 0} NaN)')


def _finite(out, what):
    for name, t in out:
        if t.dtype.is_floating_point:
            assert bool(torch.isfinite(t.float()).all()), f'{what}: {name} holds {int((~torch.isfinite(t.float())).sum())} non-finite values'


# ---------------------------------------------------------------------------------------------------------------- the locality table's rows

@pytest.mark.gpu
@pytest.mark.parametrize('row', list(ROWS))
def test_fresh_memory_kernel_rows(row, native):
    case = ROWS[row]()
    ins = {k: _plain(v, case.dtype, case.layout) for k, v in case.ins.items()}
    y0 = _flat(case.run(ins))
    _finite(y0, 'plain run')
    _same(_flat(case.run(ins)), y0, 'two plain runs differ: the kernel is not run-to-run bit-identical')
    with poisoned_empty():
        case_p = ROWS[row]()          # the packs and planes are made here, in NaN-filled memory
        y1 = _flat(case_p.run(ins))
    _finite(y1, 'every torch.empty of the product filled with NaN')
    _same(y1, y0, 'every torch.empty of the product filled with NaN')


# ---------------------------------------------------------------------------------------------------------------- rows the table does not have

def _det(name, shape, scale=1.0):
    from training.synthetic import det_tensor
    return det_tensor('fresh.' + name, list(shape), scale=scale)


def _d(name, shape, scale=1.0):
    return _det(name, shape, scale).to(DEV)


def _labelled(M, fn, want):
    """Run fn() with the launch timeline on; `want(label key)` must hold for the last launch."""
    tl = M.start_timeline()
    try:
        y = fn()
    finally:
        M.stop_timeline()
    assert tl, 'no launch was recorded'
    assert want(tl[-1][0]), tl[-1][0]
    return y


def small_row(cin, h, w, cout=3, full=False, split=False):
    from torch_utils.ops import conv2d_mfma as M
    n = 2
    x, wt = _d(f'small.x{cin}', [n, cin, h, w]), _d(f'small.w{cin}', [cout, cin, 1, 1], 1 / math.sqrt(cin))
    kw = dict(styles=_d('small.s', [n, cin]) + 1.5, bias=_d('small.b', [cout]), skip=_d('small.k', [n, cout, h, w]), scale=0.7, clamp=0.8) if full else {}
    assert M.conv1x1_small_ok(x, wt, kw.get('skip'))
    # the channel-split form takes Cin >= 64 on images that leave more than half of the CUs without a workgroup (pg_conv1x1_small)
    assert split == (cin >= 64 and n * ((h * w // 4 + 255) // 256) < torch.cuda.get_device_properties(0).multi_processor_count // 2)
    return lambda: M.conv1x1_small(x, wt, **kw)


def small16_row(cin, cout, h, w, skip_up2=None):
    """cout = 3 and 32 <= cin: the lane-spread form (conv1x1_head16.hip, launch_t's conditions); anything else: the first form."""
    from torch_utils.ops import conv2d_mfma16 as M16
    n = 2
    x = _d(f's16.x{cin}', [n, cin, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt, st, b = _d(f's16.w{cin}.{cout}', [cout, cin], 1 / math.sqrt(cin)), _d(f's16.s{cin}', [n, cin]) + 1.5, _d(f's16.b{cout}', [cout])
    skip = None if skip_up2 is None else _d('s16.k', [n, cout, h // 2, w // 2] if skip_up2 else [n, cout, h, w])
    return lambda: M16.conv1x1_small(x, wt, styles=st, bias=b, skip=skip, clamp=0.8, skip_up2=bool(skip_up2))


def fold_row(c_a):
    from torch_utils.ops import conv2d_mfma as M
    n, c1, c2, cm, cout, h, w = 2, 11, 6, 12, 6, 8, 12
    x, x2, skip = _d('fold.x', [n, c1, h, w]), _d('fold.x2', [n, c2, h, w]), _d('fold.k', [n, 3, h, w])
    wm, bm, wh, bh, st = _d('fold.wm', [cm, c1 + c2]), _d('fold.bm', [cm]), _d('fold.wh', [cout, cm]), _d('fold.bh', [cout]), _d('fold.s', [n, cm])
    assert M.conv1x1_fold_ok(x, x2, skip)

    def run():
        wn, bn = M.conv1x1_fold_prep(wm, bm, wh, bh, st)
        ya, yb = M.conv1x1_fold_heads(x, x2, wn, bn, c_a, skip=skip, clamp=2.0)
        assert (yb is None) == (c_a == cout)
        return wn, bn, ya, yb
    return run


def fold3x3_row():
    from torch_utils.ops import conv2d_mfma as M
    n, c, cm, h, w = 2, 11, 10, 6, 12
    xa, xb, skip = _d('f3.xa', [n, c, h, w]), _d('f3.xb', [n, c, h, w]), _d('f3.k', [n, 3, h, w])
    wm, bm, wh, bh, st = _d('f3.wm', [cm, 10 * c], 0.3), _d('f3.bm', [cm]), _d('f3.wh', [3, cm]), _d('f3.bh', [3]), _d('f3.s', [n, cm])
    assert M.conv3x3_fold_ok(xa, xb, skip)

    def run():
        wn, bn = M.conv1x1_fold_prep(wm, bm, wh, bh, st)
        return M.conv3x3_fold_head(xa, xb, wn, bn, skip=skip, clamp=2.0)
    return run


def cin1_row():
    from torch_utils.ops import conv2d_mfma as M
    x, wt = _d('cin1.x', [2, 1, 9, 12]), _d('cin1.w', [5, 1, 3, 3])
    assert M.conv3x3_cin1_ok(x, wt)
    return lambda: M.conv3x3_cin1(x, wt, scale=0.5, act='relu')


def splitk_tail_row():
    """The direct split-K kernel with the whole epilogue behind its summing pass."""
    from torch_utils.ops import conv2d_mfma as M
    n, cin, cout, h, w = 2, 512, 40, 8, 8
    assert M._init().lib.pg_conv2d_splitk_plan(n, cin, h, w, cout, 3, 3, 1) > 1
    x, wt = _d('sk.x', [n, cin, h, w]), _d('sk.w', [cout, cin, 3, 3], 1 / math.sqrt(9 * cin))
    packed = M.pack_weight(wt)
    kw = dict(in_scale=_d('sk.s', [n, cin]) + 1.5, out_scale=_d('sk.d', [n, cout]).abs() + 0.5, noise=_d('sk.nz', [h, w]), noise_gain=0.3, bias=_d('sk.b', [cout]),
              act='lrelu', alpha=0.2, gain=1.4, clamp=2.0, residual=_d('sk.r', [n, cout, h, w]))
    return lambda: _labelled(M, lambda: M.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), **kw), lambda key: key[:4] == (3, 3, 1, 'direct'))


def up2_mod_row():
    from torch_utils.ops import conv2d_mfma as M
    n, cin, cout, h, w = 2, 24, 40, 5, 9
    x, wt = _d('up2m.x', [n, cin, h, w]), _d('up2m.w', [cout, cin, 3, 3], 1 / math.sqrt(9 * cin))
    packs = M.pack_up2(wt, flip=True)
    s_in, s_out = _d('up2m.s', [n, cin]) + 1.5, _d('up2m.d', [n, cout]).abs() + 0.5
    return lambda: _labelled(M, lambda: M.conv_up2_forward(x, packs, cout, in_scale=s_in, out_scale=s_out), lambda key: ' up2' in key[4] and ' mod' in key[4])


def splitk16_row():
    from torch_utils.ops import conv2d_mfma as M
    from torch_utils.ops import conv2d_mfma16 as M16
    n, cin, cout, h, w = 2, 512, 64, 8, 8
    assert M16._init().pg_conv2d16_splitk_plan(n, cin, h, w, cout, 3, 3, 1) > 1
    x = _d('sk16.x', [n, cin, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    packed, _, _ = M16.pack_weight(_d('sk16.w', [cout, cin, 3, 3], 1 / math.sqrt(9 * cin)), torch.bfloat16)
    b = _d('sk16.b', [cout])
    return lambda: _labelled(M, lambda: M16.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), bias=b, act='lrelu', alpha=0.2, gain=1.4, clamp=2.0), lambda key: key[3] == 'mfma16')


def strided_out_row(half):
    """The caller allocates y: under the fill its unwritten phases are NaN.  The launch writes phase (1, 0) of a 2 x 2 interleave and nothing else."""
    from torch_utils.ops import conv2d_mfma as M
    from torch_utils.ops import conv2d_mfma16 as M16
    n, cin, cout, h, w = 2, 32, 32, 9, 13
    wt = _d('so.w', [cout, cin, 3, 3], 1 / math.sqrt(9 * cin))
    if half:
        x = _d('so.x', [n, cin, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        packed, _, _ = M16.pack_weight(wt, torch.bfloat16)
    else:
        x, packed = _d('so.x', [n, cin, h, w]), M.pack_weight(wt)

    def run():
        if half:
            y = torch.empty([n, cout, 2 * h, 2 * w], dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)
            M16.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), y=y, out_step=(2, 2), out_off=(1, 0))
        else:
            y = torch.empty([n, cout, 2 * h, 2 * w], dtype=torch.float32, device=DEV)
            M.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), y=y, out_step=(2, 2), out_off=(1, 0))
        run.full = y
        return y[:, :, 1::2, 0::2]

    def after_poison():
        rest = run.full.detach().float().cpu().clone()
        assert bool(torch.isnan(rest[:, :, 0::2, :]).all()) and bool(torch.isnan(rest[:, :, 1::2, 1::2]).all()), 'the launch wrote outside its own phase'
    run.after_poison = after_poison
    return run


def f4_stats_row():
    from torch_utils.ops import conv2d_mfma as M
    n, cin, cout, h, w = 2, 16, 64, 12, 64
    x, wt = _d('st.x', [n, cin, h, w]), _d('st.w', [cout, cin, 3, 3], 1 / math.sqrt(9 * cin))
    packed = M.pack_weight(wt, winograd=M.WINO_F4)
    return lambda: _labelled(M, lambda: M.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), winograd=M.WINO_F4, stats_eps=1e-5), lambda key: key[3] == M.WINO_FORMS[M.WINO_F4][0])


def in_stats_row():
    from torch_utils.ops import conv2d_mfma as M
    x = _d('in.x', [3, 7, 9, 13])
    return lambda: M.instance_norm_stats(x, 1e-5)


def in_stats16_row():
    from torch_utils.ops import conv2d_mfma16 as M16
    x = _d('in16.x', [2, 32, 9, 13]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return lambda: M16.instance_norm_stats16(x, 1e-5)


def spade_rows(kind):
    from torch_utils.ops import conv2d_mfma as M
    from torch_utils.ops import conv2d_mfma16 as M16
    n, c, h, w = 2, 7, 9, 13
    x, dy, gb = _d('sp.x', [n, c, h, w]), _d('sp.dy', [n, c, h, w]), _d('sp.gb', [n, 2 * c, h, w])
    mean, rstd = _d('sp.mu', [n * c]), _d('sp.rs', [n * c]).abs() + 0.5
    if kind == 'norm':
        g, b = gb[:, :c].contiguous(), gb[:, c:].contiguous()
        return lambda: M.spade_norm(x, mean, rstd, g, b)
    if kind == 'train_forward':
        return lambda: M.spade_train_forward(x, mean, rstd, gb)
    if kind.startswith('train_backward'):
        need_dx, need_dgb = kind != 'train_backward_dgb', kind != 'train_backward_dx'
        return lambda: M.spade_train_backward(dy, x, mean, rstd, gb, need_dx=need_dx, need_dgb=need_dgb)
    if kind == 'feat_assemble':
        fu, fl = _d('sp.fu', [n, c, h, w]), _d('sp.fl', [n, c, h, w])
        masks = [(_d(f'sp.m{i}', [n, 1, 2 * h, 2 * w]) > 0).float() for i in range(4)]
        return lambda: M.spade_feat_assemble(fu, fl, *masks)
    assert kind == 'combine16'
    c = 16
    x16 = _d('sp16.x', [n, c, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gb16 = _d('sp16.gb', [n, 2 * c, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    mean, rstd = _d('sp16.mu', [n * c]), _d('sp16.rs', [n * c]).abs() + 0.5
    return lambda: M16.spade_combine16(x16, mean, rstd, gb16, act='lrelu', alpha=0.2, gain=1.4, clamp=2.0)


def modconv_rows(kind):
    from torch_utils.ops import conv2d_mfma as M
    n, cin, cout = 3, 20, 12
    wt, st = _d('mc.w', [cout, cin, 3, 3]), _d('mc.s', [n, cin]) + 1.5
    if kind == 'dcoefs':
        return lambda: M.modconv_dcoefs(wt, st, scale=0.3)
    if kind == 'w2':
        return lambda: M.modconv_w2(wt, scale=0.3)
    w2 = M.modconv_w2(wt, scale=0.3)
    if kind.startswith('prep_batched'):
        half = torch.bfloat16 if kind.endswith('half') else None
        st2, st3 = _d('mc.s2', [n, 16]) + 1.5, _d('mc.s3', [n, 16]) + 1.5
        w2b = M.modconv_w2(_d('mc.w2', [8, 16, 1, 1]))

        def run():
            M.modconv_prep_clear()
            try:
                M.modconv_prep_batched([(w2, st, cout, True, True), (w2b, st2, 8, False, True), (None, st3, 8, False, False)], half_dtype=half)
                assert len(M._prep_registry) == 3
                out = [M.modconv_prep(w2, st, cout, normalize=True, demodulate=True, half_dtype=half), M.modconv_prep(w2b, st2, 8),
                       M.modconv_prep(None, st3, 8, demodulate=False)]
                assert not M._prep_registry, 'a layer call launched on its own instead of taking the batched result'
                return out
            finally:
                M.modconv_prep_clear()
        return run
    kw = {'prep_plain': {}, 'prep_normalize': dict(normalize=True), 'prep_half': dict(normalize=True, half_dtype=torch.float16), 'prep_max': dict(demodulate=False)}[kind]
    return lambda: M.modconv_prep(w2 if kw.get('demodulate', True) else None, st, cout, **kw)


def wgrad_splits_row(bf16x3):
    from test_nonfinite_locality import _env
    from torch_utils.ops import conv2d_mfma as M
    n, cin, cout, h, w = 2, 16, 24, 40, 37
    lib = M._init().lib
    splits = lib.pg_conv2d16_wgrad_plan(6 * n, cin, h, w, cout, 3, 3, 1) if bf16x3 else lib.pg_conv2d_wgrad_plan(n, cin, h, w, cout, 3, 3, 1)
    assert splits > 1, splits
    x, dy = _d('wgs.x', [n, cin, h, w]), _d('wgs.dy', [n, cout, h, w])

    def run():
        with _env(PG_WGRAD_BF16X3='1' if bf16x3 else '0'):
            tl = M.start_wgrad_timeline()
            try:
                dw = M.weight_gradient(x, dy, [cout, cin, 3, 3], (1, 1))
            finally:
                M.stop_wgrad_timeline()
        assert dw is not None and tl[-1][0][3] == ('wgrad_bf16x3' if bf16x3 else 'wgrad'), tl
        return dw
    return run


def wgrad16_row():
    from torch_utils.ops import conv2d_mfma16 as M16
    n, cin, cout, h, w = 2, 6, 24, 20, 37          # six image channels: zero-padded to 8 by the wrapper
    x = _d('wg16.x', [n, cin, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = _d('wg16.dy', [n, cout, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def run():
        dw = M16.weight_gradient(x, dy, [cout, cin, 3, 3], (1, 1))
        assert dw is not None
        return dw
    return run


def pack16_rows(kind):
    """The grouped and batched 16-bit packers through a convolution that reads every lane of the pack."""
    from torch_utils.ops import conv2d_mfma16 as M16
    n, cin, cout, h, w = 2, 48, 40, 9, 13
    x = _d('p16.x', [n, cin, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    st, dco = _d('p16.s', [n, cin]) + 1.5, _d('p16.d', [n, cout]).abs() + 0.5
    if kind == 'grouped':
        ws = _d('p16.wg', [2, cout, cin, 3, 3], 1 / math.sqrt(9 * cin))

        def run():
            packed, per = M16.pack_weight_grouped(ws, torch.bfloat16, scale=0.9, styles=st, dcoefs=dco)
            return [M16.conv2d_forward(x, packed[g], cout, 3, 3, pad=(1, 1), sample_stride=per) for g in range(2)]
        return run
    wt = _d('p16.w', [cout, cin, 3, 3], 1 / math.sqrt(9 * cin))

    def run():
        M16.pack_clear()
        try:
            M16.pack_weight_batched([(wt, False, False, st, dco)], torch.bfloat16)
            packed, per = M16.pack_lookup(wt, torch.bfloat16, False, False, st)
        finally:
            M16.pack_clear()
        return M16.conv2d_forward(x, packed, cout, 3, 3, pad=(1, 1), sample_stride=per)
    return run


def transposed16_row():
    from torch_utils.ops import conv2d_mfma16 as M16
    n, cin, cout, h, w = 2, 16, 32, 7, 9
    x = _d('t16.x', [n, cin, h, w]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = _d('t16.w', [cin, cout, 3, 3], 1 / math.sqrt(9 * cin))
    out_hw = ((h - 1) * 2 - 2 + 3, (w - 1) * 2 - 2 + 3)
    phases = M16.pack_transposed(wt, torch.bfloat16, 2, (1, 1), (h, w), out_hw)
    assert phases is not None and len(phases) == 4
    return lambda: M16.conv_transpose2d_forward(x, phases, cout, out_hw)


def fir_generic_row():
    from test_nonfinite_locality import ROUTE_FIR
    from torch_utils.ops import upfirdn2d as U
    x, f = _d('firg.x', [2, 5, 9, 14]), _d('firg.f', [5, 3]).to(DEV)          # a 2-D, non-separable, odd-sized filter: the generic kernel

    def run():
        y = U.upfirdn2d(x, f, up=2, down=3, padding=[2, 1, 3, 0], flip_filter=True, gain=2.0)
        assert U._plugin.lib.pg_upfirdn2d_last_route() == ROUTE_FIR['generic'], U._plugin.lib.pg_upfirdn2d_last_route()
        return y
    return run


def fir_shared_odd_extents_row():
    from torch_utils.ops import upfirdn2d as U
    x, f = _d('firo.x', [2, 5, 9, 15]), U.setup_filter([1, 3, 3, 1]).to(DEV)
    return lambda: U.filter_with_odd_samples(x, f, padding=[2, 2, 2, 2])


def fir_after_up2_row(bias_act, x3):
    """The FIR pass fed with the pitched view `conv_up2_forward` returns: under the fill the pad lanes behind each of its rows are NaN."""
    from torch_utils.ops import conv2d_mfma as M
    from torch_utils.ops import upfirdn2d as U
    n, cin, cout, h, w = (2, 32, 40, 9, 20) if x3 else (2, 24, 40, 5, 9)
    x, wt = _d(f'fu.x{cin}', [n, cin, h, w]), _d(f'fu.w{cin}', [cout, cin, 3, 3], 1 / math.sqrt(9 * cin))
    f, b = U.setup_filter([1, 3, 3, 1]).to(DEV), _d('fu.b', [cout])
    packs = M.pack_up2(wt)
    assert ('x3' in packs) == x3

    def run():
        y = M.conv_up2_forward(x, packs, cout)
        assert y.stride(2) % 4 == 0 and y.stride(2) > y.shape[3], 'no pad lanes in this view'
        if bias_act:
            z = U.upfirdn2d_bias_act(y, f, padding=[1, 1, 1, 1], gain=4.0, b=b, act='lrelu', act_gain=1.4, clamp=2.0)
            assert z is not None, 'upfirdn2d_bias_act declined the launch'
            return z
        return U.upfirdn2d(y, f, padding=[1, 1, 1, 1], gain=4.0)
    return run


def bias_act_row(shape, grad):
    from torch_utils.ops import bias_act as B
    x, b, dy = _d(f'ba.x{len(shape)}', shape, 2.0), _d(f'ba.b{len(shape)}', [shape[1]]), _d(f'ba.dy{len(shape)}', shape)
    if not grad:
        return lambda: B.bias_act(x, b, act='lrelu', gain=1.4, clamp=1.5)

    def run():          # dx and db of one backward pass (the one-pass kernel with its `work` buffer)
        xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = B.bias_act(xr, br, act='lrelu', gain=1.4, clamp=1.5)
        return [y.detach()] + list(torch.autograd.grad(y, [xr, br], dy))
    return run


def transposed_wgrad_row(half):
    """conv_transpose2d through conv2d_gradfix: the forward (the four-parity kernel / the phase launches) and the weight gradient with x and dy swapped."""
    from torch_utils.ops import conv2d_gradfix as G
    n, cin, cout, h, w = 2, 16, 24, 9, 13
    x, wt = _d('tw.x', [n, cin, h, w]), _d('tw.w', [cin, cout, 3, 3], 1 / math.sqrt(9 * cin))
    dy = _d('tw.dy', [n, cout, 2 * h + 1, 2 * w + 1])
    if half:
        x, dy = (t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for t in (x, dy))

    def run():
        wr = wt.clone().requires_grad_(True)
        y = G.conv_transpose2d(x, wr, stride=2)
        dw, = torch.autograd.grad(y, wr, dy)
        return y.detach(), dw
    return run


def flat_adam_row():
    """pg_adam_flat_step: FlatAdam's own state comes from torch.zeros_like; the gradients reach the bucket through GradBucket's gather."""
    from training import ddp
    from training.flat_adam import FlatAdam
    shapes, dead = [(7,), (33, 17), (513,), (2, 2), (64, 3, 3, 3)], 2
    ps = [torch.nn.Parameter(_d(f'adam.p{i}', s)) for i, s in enumerate(shapes)]
    grads = [[_d(f'adam.g{it}.{i}', s) for i, s in enumerate(shapes)] for it in range(2)]
    grads[1][1].view(-1)[5:8] = torch.tensor([float('nan'), float('inf'), float('-inf')], device=DEV)
    bucket = ddp.GradBucket(ps)
    opt = FlatAdam(bucket, 0.002, (0.0, 0.99), 1e-8)

    def run():
        # (the optimizer keeps state: a run starts from the same parameters and moments)
        with torch.no_grad():
            for i, p in enumerate(ps):
                p.copy_(_d(f'adam.p{i}', shapes[i]))
            for t in (opt.exp_avg, opt.exp_avg_sq, opt.steps[0], opt.steps[1]):
                t.zero_()
        for it in range(2):
            bucket.begin()
            for i, p in enumerate(ps):
                if i == dead:
                    continue
                if bucket.gather:
                    p.grad = grads[it][i].clone()
                else:
                    p.grad.copy_(grads[it][i])
                bucket._touched_host[i] = True
            assert bucket.finish()
            opt.step()
        return [p.detach().clone() for p in ps] + [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.steps[0].clone(), bucket.flat.clone()]
    return run


def vgg_rows(kind):
    from torch_utils.ops import vgg_ops as V
    if kind == 'maxpool':
        x, dy = _d('vgg.x', [2, 5, 9, 14]), _d('vgg.dy', [2, 5, 4, 7])

        def run():
            xr = x.clone().requires_grad_(True)
            y = V.maxpool2x2(xr)
            return y.detach(), torch.autograd.grad(y, xr, dy)[0]
        return run
    outs = []
    for shape in ([2, 3, 7, 9], [1, 5, 37, 41]):          # m = 378 and 7585 elements: neither a multiple of a block
        outs.append((_d(f'vgg.l1.x{shape[1]}', [2 * shape[0]] + shape[1:]), _d(f'vgg.l1.y{shape[1]}', shape)))
    dout = torch.tensor([0.7, -1.3], device=DEV)

    def run():
        res = []
        for x, y in outs:
            xr = x.clone().requires_grad_(True)
            out = V.l1_mean(xr, y, groups=2)
            res += [out.detach(), torch.autograd.grad(out, xr, dout)[0]]
        return res
    return run


_drawn = {}


def _augment_draw(shape):
    """Parameters drawn once, on the CPU and outside the fill (the draw is input generation, not the product call under test)."""
    if shape not in _drawn:
        import augment_late_cases as LC
        from test_augment_late_gpu import draw_spec
        _drawn[shape] = draw_spec('bgcfnc', LC.SHAPES[shape], 23, 1.0)
    return _drawn[shape]


def augment_row(kind, shape):
    from test_augment_late_gpu import pipe_of, to
    from torch_utils.ops import augment_ops as A
    x, params, late = _augment_draw(shape)
    xd, (G, m, C), lated = x.to(DEV), to(params, DEV), to(late, DEV)
    assert G is not None and C is not None and all(t is not None for t in lated)
    dy = _d(f'aug.dy.{shape}', list(x.shape))
    pipe = pipe_of('bgcfnc', device=DEV)
    fn = {'warp': lambda t: A.geometric(t, G, m, pipe.Hz_geom), 'color': lambda t: A.color(t, C), 'late': lambda t: A.late(t, *lated)}[kind]

    def run():
        xr = xd.clone().requires_grad_(True)
        y = fn(xr)
        return y.detach(), torch.autograd.grad(y, xr, dy)[0]
    return run


def _u8(name, shape, lo=0, hi=256):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(sum(map(ord, name))), dtype=torch.int32).to(torch.uint8).to(DEV)


def metrics_rows(kind):
    from torch_utils.ops import image_metrics as IM
    from torch_utils.ops import region_metrics as RM
    a, b = _u8('met.a', [3, 23, 41, 3]), _u8('met.b', [3, 23, 41, 3])
    a, b = a[:, :, :37], b[:, :, 2:39]                  # views: pixel stride 3, row stride 123
    labels = _u8('met.l', [3, 23, 37], 0, 7)
    if kind == 'image':
        return lambda: IM.pair_metrics(a, b)
    if kind == 'region':
        return lambda: RM.region_metrics_table([(a[j], b[j], labels[j]) for j in range(3)], [[1, 2], [3], [0, 4, 5, 6]])
    lut = list(range(7)) + [RM.IGNORE] * 249
    pred = _u8('met.p', [3, 23, 37], 0, 9)
    return lambda: RM.label_confusion_table([(pred[j], labels[j]) for j in range(3)], lut, lut, 7)


def _tryon_random(part):
    if ('tryon', part) not in _drawn:
        from test_tryon_gpu import _random_batch
        batch, routed = _random_batch(2, part, 5)
        batch['skin'][0, 1] = 3.5               # (the fixture's NaN skin median would make `retain` NaN by design: this test wants finite results)
        _drawn[('tryon', part)] = (batch, tuple(routed))
    return _drawn[('tryon', part)]


def tryon_rows(kind):
    from training import tryon as T
    if kind.startswith('inputs'):
        part = kind.split('_')[1]
        batch, routed = _tryon_random(part)

        def run():
            ext = T.row_extents(T._canvases(batch, routed, part)[2])
            return ext, T.batch_inputs(batch, routed, ext, part)
        return run
    if ('trip',) not in _drawn:
        from test_tryon_cpu import crafted_triptych_case
        fin, clothes, image = crafted_triptych_case()
        _drawn[('trip',)] = tuple(torch.from_numpy(t).to(DEV) for t in (fin, clothes, image))
    fin, clothes, image = _drawn[('trip',)]
    if kind == 'triptych':
        return lambda: T.triptych(fin, clothes, image)
    lower = clothes.flip(0).flip(3).contiguous()
    return lambda: T.panels(fin, [clothes, lower, image])


def train_fetch_row():
    from training import train_fetch as TF
    if ('fetch',) not in _drawn:
        from test_train_fetch_gpu import _random_batch
        batch, routed, _ = _random_batch(3, 14)
        batch['skin'][0, 1] = 3.5
        _drawn[('fetch',)] = (batch, routed)
    batch, routed = _drawn[('fetch',)]

    def run():
        ext = TF.lower_mask_extents(routed)
        return ext, TF.fetch(batch, routed, ext)
    return run


def snapshot_rows(kind):
    import numpy as np
    from training import snapshot_grid as S
    if kind == 'denorm':
        from test_snapshot_grid_gpu import make_jobs
        jobs, _ = make_jobs(np.random.default_rng(48), 40, 136, 16, 20, torch.device(DEV))
        return lambda: S.denorm_canvases(jobs, 40, 136, 8)
    if kind == 'warp':
        from test_snapshot_grid_gpu import make_jobs
        jobs, _ = make_jobs(np.random.default_rng(48), 40, 136, 16, 20, torch.device(DEV))
        parts = jobs[2]
        return lambda: S.warp_batch([p[0] for p in parts], [p[2] for p in parts], (136, 40))
    rng = np.random.default_rng(7)
    n, C, H, W, gh, gw, first = 5, 7, 8, 12, 3, 2, 1
    fin = torch.from_numpy((rng.standard_normal((n, 3, H, W)) * 0.8).astype(np.float32)).to(DEV)
    par = torch.from_numpy((rng.integers(-8, 8, (n, C, H, W)) * 0.25).astype(np.float32)).to(DEV)
    grey = torch.from_numpy(S.grey_table(C)).to(DEV)
    base = [torch.from_numpy(rng.integers(0, 256, ((gh + 1) * H, (gw + 1) * W, 3), dtype=np.uint8)).to(DEV) for _ in range(2)]

    def run():
        grids = [g.clone() for g in base]
        S.pack_cells(fin, par, grey, grids[0], grids[1], first, gh, gw)
        return grids
    return run


EXTRA = {
    'small_plain': lambda: small_row(20, 8, 12),
    'small_full': lambda: small_row(20, 8, 12, full=True),
    'small_split': lambda: small_row(64, 8, 8, full=True, split=True),
    'small16': lambda: small16_row(16, 4, 8, 12, skip_up2=False),
    'head16': lambda: small16_row(64, 3, 8, 12),
    'head16_skip_up2': lambda: small16_row(64, 3, 8, 12, skip_up2=True),
    'fold_two_outputs': lambda: fold_row(3),
    'fold_one_output': lambda: fold_row(6),
    'fold3x3': fold3x3_row,
    'cin1': cin1_row,
    'splitk_tail': splitk_tail_row,
    'up2_mod': up2_mod_row,
    'splitk16': splitk16_row,
    'strided_out_f32': lambda: strided_out_row(False),
    'strided_out_16': lambda: strided_out_row(True),
    'f4_stats': f4_stats_row,
    'in_stats': in_stats_row,
    'in_stats16': in_stats16_row,
    'spade_norm': lambda: spade_rows('norm'),
    'spade_train_forward': lambda: spade_rows('train_forward'),
    'spade_train_backward_both': lambda: spade_rows('train_backward_both'),
    'spade_train_backward_dx': lambda: spade_rows('train_backward_dx'),
    'spade_train_backward_dgb': lambda: spade_rows('train_backward_dgb'),
    'spade_feat_assemble': lambda: spade_rows('feat_assemble'),
    'spade_combine16': lambda: spade_rows('combine16'),
    'modconv_dcoefs': lambda: modconv_rows('dcoefs'),
    'modconv_w2': lambda: modconv_rows('w2'),
    'modconv_prep_plain': lambda: modconv_rows('prep_plain'),
    'modconv_prep_normalize': lambda: modconv_rows('prep_normalize'),
    'modconv_prep_half': lambda: modconv_rows('prep_half'),
    'modconv_prep_max': lambda: modconv_rows('prep_max'),
    'modconv_prep_batched': lambda: modconv_rows('prep_batched'),
    'modconv_prep_batched_half': lambda: modconv_rows('prep_batched_half'),
    'wgrad_splits': lambda: wgrad_splits_row(False),
    'wgrad_bf16x3_splits': lambda: wgrad_splits_row(True),
    'wgrad16': wgrad16_row,
    'pack16_grouped': lambda: pack16_rows('grouped'),
    'pack16_batched': lambda: pack16_rows('batched'),
    'transposed16': transposed16_row,
    'fir_generic': fir_generic_row,
    'fir_shared_odd_extents': fir_shared_odd_extents_row,
    'fir_after_up2': lambda: fir_after_up2_row(False, False),
    'fir_after_up2_x3': lambda: fir_after_up2_row(False, True),
    'fir_bias_act_after_up2': lambda: fir_after_up2_row(True, False),
    'fir_bias_act_after_up2_x3': lambda: fir_after_up2_row(True, True),
    'bias_act_4d': lambda: bias_act_row([2, 7, 9, 13], False),
    'bias_act_2d': lambda: bias_act_row([5, 37], False),
    'bias_act_grad_4d': lambda: bias_act_row([2, 7, 9, 13], True),
    'bias_act_grad_2d': lambda: bias_act_row([5, 37], True),
    'transposed_wgrad': lambda: transposed_wgrad_row(False),
    'transposed_wgrad16': lambda: transposed_wgrad_row(True),
    'flat_adam_step': flat_adam_row,
    'vgg_maxpool': lambda: vgg_rows('maxpool'),
    'vgg_l1_pair': lambda: vgg_rows('l1'),
    'augment_warp': lambda: augment_row('warp', 'min'),
    'augment_warp_tiles': lambda: augment_row('warp', 'tiles'),
    'augment_color': lambda: augment_row('color', 'min'),
    'augment_color_tiles': lambda: augment_row('color', 'tiles'),
    'augment_late': lambda: augment_row('late', 'min'),
    'augment_late_tiles': lambda: augment_row('late', 'tiles'),
    'image_metrics': lambda: metrics_rows('image'),
    'region_metrics': lambda: metrics_rows('region'),
    'label_confusion': lambda: metrics_rows('confusion'),
    'tryon_inputs_upper': lambda: tryon_rows('inputs_upper'),
    'tryon_inputs_full': lambda: tryon_rows('inputs_full'),
    'tryon_triptych': lambda: tryon_rows('triptych'),
    'tryon_panels': lambda: tryon_rows('panels'),
    'train_fetch': train_fetch_row,
    'snapshot_denorm': lambda: snapshot_rows('denorm'),
    'snapshot_warp': lambda: snapshot_rows('warp'),
    'snapshot_cells': lambda: snapshot_rows('cells'),
}


def _check_fresh(make):
    """Plain twice, then factory and run under the fill: identical bits, finite."""
    run = make()
    y0 = _flat(run())
    _finite(y0, 'plain run')
    _same(_flat(run()), y0, 'two plain runs differ: the route is not run-to-run bit-identical')
    with poisoned_empty():
        run_p = make()
        y1 = _flat(run_p())
        if hasattr(run_p, 'after_poison'):
            run_p.after_poison()
    _finite(y1, 'every torch.empty filled with NaN')
    _same(y1, y0, 'every torch.empty filled with NaN')


@pytest.mark.gpu
@pytest.mark.parametrize('row', list(EXTRA))
def test_fresh_memory_extra_rows(row, native):
    _check_fresh(EXTRA[row])


# ---------------------------------------------------------------------------------------------------------------- rows that read files

from test_train_fetch_gpu import train_set  # noqa: E402,F401  (the synthetic training root of the loader's own tests)
from test_tryon_cpu import pairs_root  # noqa: E402,F401  (the three synthetic pairs of the try-on tests)


def _raw_batch(root, part):
    key = ('raw', root, part)
    if key not in _drawn:
        from training import tryon
        from training.dataset import TryOnTestSet, collate_raw
        ds = TryOnTestSet(root, use_sleeve_mask=True, device='cpu', part=part)
        _drawn[key] = tryon.upload(collate_raw([ds.raw(i) for i in range(len(ds))], pin=True), DEV)
    return _drawn[key]


@pytest.mark.gpu
@pytest.mark.parametrize('part', ['upper', 'full'])
def test_fresh_memory_tryon_front(pairs_root, part, native):  # noqa: F811
    """`tryon_front.front_batch`: the `stats` / `bit_rows` tables its kernels fill with atomics, and every staged output."""
    from training import tryon_front

    def make():
        raw = _raw_batch(pairs_root, part)
        return lambda: {k: v for k, v in tryon_front.front_batch(raw, part).items() if torch.is_tensor(v)}
    _check_fresh(make)


@pytest.mark.gpu
def test_fresh_memory_patch_normalize(train_set, native):  # noqa: F811
    """`patch_routing.normalize_batch` (warp, compose, de-normalised canvases) on three persons of the synthetic training root."""
    from test_train_loader import PERSONS, index_of
    from training import patch_routing as P
    from training.dataset import NO_ERASE
    gpu = lambda a: torch.from_numpy(a).to(DEV)
    samples = []
    for _, name, _ in PERSONS[:3]:
        u = train_set.unrouted(index_of(train_set, name), NO_ERASE)
        samples.append((gpu(u['upper_img']), gpu(u['lower_img']), gpu(u['upper_mask']), gpu(u['lower_mask']), gpu(u['sleeve']), u['person_kp'], u['person_kp']))
    _check_fresh(lambda: (lambda: list(P.normalize_batch(samples, 2, part='train'))))
    u = train_set.unrouted(index_of(train_set, PERSONS[0][1]), NO_ERASE)           # the single-sample route: one warp launch per patch, patch_compose_
    _check_fresh(lambda: (lambda: list(P.normalize(u['upper_img'], u['lower_img'], u['upper_mask'], u['lower_mask'], u['sleeve'], u['person_kp'], u['person_kp'], 2,
                                                  device=DEV, part='train'))))


# ---------------------------------------------------------------------------------------------------------------- whole routes

def _route_generator(half):
    import cases as C
    from detgen import fill_module_, synthesis_inputs
    from training import networks as PN
    if half:
        import test_tryon_half as TH
        inp = {k: v.to(DEV) for k, v in TH._inputs().items()}

        def make():
            net = fill_module_(PN.GeneratorFull_v20(**TH.G_KW), 'half.G.').eval().requires_grad_(False).to(DEV)
            net.set_half(torch.bfloat16)

            def run():
                with torch.no_grad():
                    return net(**inp, noise_mode='const')
            return run
        return make
    inp = synthesis_inputs(1, w_dim=C.G6_KW['w_dim'], num_ws=14, feat_ch=C.G6_FEAT_CH, seed_tag='g6', labels=True)
    to = lambda t: t.to(DEV) if t is not None else None
    args = (to(inp['ws']), to(inp['pose_feat']), {k: v.to(DEV) for k, v in inp['cat_feat'].items()}, to(inp['denorm_upper_input']),
            to(inp['denorm_lower_input']), to(inp['denorm_upper_mask']), to(inp['denorm_lower_mask']), to(inp['gt_parsing']))

    def make():
        net = fill_module_(PN.SynthesisNetworkFull_v18(**C.G6_KW), 'g6.').to(DEV).eval()
        assert net.num_ws == 14

        def run():
            with torch.no_grad():
                return net(*args, noise_mode='const')
        return run
    return make


def _route_discriminator():
    """Forward + backward, and R1's double backward, of the product discriminator with a half-precision block at resolution 16."""
    from training import networks as PN
    gen = torch.Generator().manual_seed(0)
    x, c = torch.randn(4, 6, 16, 16, generator=gen).to(DEV), torch.randn(4, 6, generator=gen).to(DEV)
    kw = dict(c_dim=6, img_resolution=16, img_channels=6, channel_base=256, channel_max=32, conv_clamp=256, mapping_kwargs=dict(num_layers=1),
              epilogue_kwargs=dict(mbstd_group_size=2))

    def make():
        torch.manual_seed(0)
        d = PN.Discriminator(**kw, num_fp16_res=1).to(DEV).train()

        def grads():
            return {n: p.grad.detach().clone() for n, p in d.named_parameters() if p.grad is not None}

        def run():
            for p in d.parameters():
                p.grad = None
            d(x, c).sum().backward()
            first = grads()
            for p in d.parameters():
                p.grad = None
            xr = x.detach().requires_grad_(True)
            gx, = torch.autograd.grad(d(xr, c).sum(), xr, create_graph=True)
            (gx.square().sum([1, 2, 3]).mean() * 5).backward()
            r1 = grads()
            assert len(first) > 10 and len(r1) > 10
            return dict(first=first, r1=r1)
        return run
    return make


def _route_training_step():
    """Two eager iterations of the discriminator phases of TrainingStep (Dmain, Dreg with R1's double backward, D_parsingmain, both D_parsingreg entries): flat
    Adam, GradBucket's gather, the pre-scaled weight copies, with the product discriminators.  The generator phases are left out: the stub generator of this
    setup is made of aten convolutions, whose weight gradient (MIOpen) is not run-to-run reproducible -- two runs in ordinary memory already differ in
    `G_synthesis.mix.weight` -- so the route is narrowed until its plain runs are bit-identical instead of being given a tolerance."""
    import stubs
    from detgen import fill_module_
    from oracle import network_ref as NR
    from test_hip_parity import _d_kw
    from training import networks as PN
    from training.loss import StyleGAN2Loss
    from training.training_step import TrainingStep
    batch = stubs.batch(4, DEV)

    def make():
        torch.manual_seed(0)
        nets = stubs.build(DEV)
        for name, ch in (('D', 6), ('D_parsing', 10)):
            ref = fill_module_(NR.Discriminator(**_d_kw(ch)), f'fresh.{name}.')
            d = PN.Discriminator(**_d_kw(ch))
            d.load_state_dict(ref.state_dict(), strict=False)
            nets[name] = d.to(DEV).train()
        loss = StyleGAN2Loss(device=torch.device(DEV), **nets, style_mixing_prob=0, r1_gamma=10, l1_weight=50, mask_weight=1.0)
        step = TrainingStep({k: v for k, v in nets.items() if k.startswith('G_')}, nets['D'], nets['D_parsing'], loss, batch_size=4, graphs=False)
        from training.flat_adam import FlatAdam
        assert all(isinstance(ph.opt, FlatAdam) and ph.bucket.gather for ph in step.phases) and step._gained
        ran = []

        def run():
            assert not ran, 'a training step keeps state: one run per instance'
            ran.append(1)
            names = []
            for _ in range(2):
                for ph in step.phases:
                    if ph.name.startswith('D') and step.batch_idx % ph.interval == 0:
                        step._phase(ph, [batch])
                        names.append(ph.name)
                step.batch_idx += 1
            torch.cuda.synchronize()
            assert names == ['Dmain', 'Dreg', 'D_parsingmain', 'D_parsingreg', 'D_parsingmain', 'D_parsingreg', 'Dmain', 'D_parsingmain', 'D_parsingmain'], names
            out = {f'{k}.{n}': p.detach().clone() for k in ('D', 'D_parsing') for n, p in nets[k].named_parameters()}
            out.update({f'adam{i}.{k}': getattr(ph.opt, k).clone() for i, ph in enumerate(step.phases) if ph.name.startswith('D') for k in ('exp_avg', 'exp_avg_sq')})
            return out
        return run
    return make


def _check_route(make, stateful=False):
    """`_check_fresh` for a model: a stateful route (the training step) gets a fresh instance per run."""
    if not stateful:
        return _check_fresh(make)
    y0 = _flat(make()())
    _finite(y0, 'plain run')
    _same(_flat(make()()), y0, 'two plain runs differ: the route is not run-to-run bit-identical')
    with poisoned_empty():
        y1 = _flat(make()())
    _finite(y1, 'every torch.empty filled with NaN')
    _same(y1, y0, 'every torch.empty filled with NaN')


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['generator_fp32', 'generator_bf16', 'discriminator_r1', 'training_step', 'tryon_batch'])
def test_fresh_memory_routes(route, native, pairs_root, monkeypatch):  # noqa: F811
    """The call patterns of the networks: the layers' own pack caches, the cached up = 2 packs, the fold caches, the affine gather, GradBucket.  A fresh model is
    built and run under the fill and must reproduce the bits of the model built and run in ordinary memory."""
    if route == 'generator_fp32':
        _check_route(_route_generator(False))
    elif route == 'generator_bf16':
        _check_route(_route_generator(True))
    elif route == 'discriminator_r1':
        _check_route(_route_discriminator())
    elif route == 'training_step':
        monkeypatch.setenv('PG_FLAT_ADAM', '1')
        monkeypatch.delenv('PG_GAIN_FOLD', raising=False)
        _check_route(_route_training_step(), stateful=True)
    else:
        from test_tryon_cpu import _small_generator
        from training import tryon, tryon_front

        def make():
            raw = _raw_batch(pairs_root, 'upper')
            G = _small_generator().to(DEV)
            return lambda: tryon.tryon_batch(tryon_front.front_batch(raw, 'upper'), G, 'upper')
        _check_route(make)
