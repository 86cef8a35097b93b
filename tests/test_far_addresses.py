"""Every kernel on tensors past 2, 4 and 8 GiB (DESIGN "Far addresses").

Every other test launches on a few megabytes, so no byte offset above 2^31 is ever formed.  Here a case is built at a base batch of P = 3 samples on the CPU
(the factories of `test_nonfinite_locality`, and small ones of the same shape below), moved to the device and REPEATED along N there until the operands
that grow with N lie past the marks

    '31'  byte offset 2^31        '32'  byte offset 2^32        'e31'  element index 2^31

-- as many of them as the entry's own guard (and 24 GiB per row) admit; nothing large is made on the CPU or copied over.  Per launch:

  1. periodicity, bit for bit: output sample n equals output sample n mod P, compared on the device over the whole tensor (a wrapped address in ANY sample,
     no tolerance);
  2. samples 0..P-1 of the far launch meet the case's float64 reference (computed on the CPU from the P base samples) at the bar the kernel form already has
     in its existing float64 test -- the row names that test;
  3. the P base outputs differ from each other and from zero, P is odd and every launch runs under `poisoned_empty()`.  A mark is a power of two in bytes,
     so it is never a whole number of periods of any operand: an address truncated at a mark reads a sample of another phase (or lands mid-sample), and a
     far sample the launch fails to write stays NaN.  A wrap into "some other sample" or into a zero page cannot pass, on the read side or on the write side.

The weight gradients sum over N, so periodicity does not apply: every sample has dy = 0 except the first, the last and the two on either side of each mark
of x and of dy, which carry mutually distinct data; the result is compared with the float64 gradient of those few samples.  The bias gradient sums over N
too: its float64 value is N / P times the base's.

Each row states the marks its operands cross; the harness measures them on the tensors of the launch and requires the statement to be exact.

The guard table at the end needs no GPU: every size guard is called through the C ABI with non-null dummy pointers at the first size past it and must
answer PG_ERR_TOO_LARGE.  (An ACCEPTED size would launch on the dummy pointers, so the accepting side is asserted only where a later host check declines the
call before any launch; for the rest the far rows above are the proof, they run at those sizes.)

The GPU tests carry the `gpu` mark one by one: the guard table has to run where there is no GPU.
"""

import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poisoned_alloc import poisoned_empty
from test_nonfinite_locality import (ROUTE_1X1, ROUTE_FIR, Case, _env, _last_label, _plain, _weights, _wino, conv16_case, conv_case, fir_case, stem_case,
                                     transposed_case, up2_case)

DEV = 'cuda'
P = 3                                   # base batch: what the factories build on the CPU.  Odd on purpose: no mark (a power of two in bytes) is a whole number of periods of
                                        # any operand, so an address truncated mod 2^31, 2^32 or 2^33 bytes lands in a sample of ANOTHER phase (or mid-sample), never on identical bits
GIB = 1 << 30
GAIN = math.sqrt(2)
NAN = float('nan')
MARKS = (('31', 1 << 31, 'bytes'), ('32', 1 << 32, 'bytes'), ('e31', 1 << 31, 'elements'))
ALL = '31 32 e31'


# ---------------------------------------------------------------------------------------------------------------- bars (each from an existing float64 test)

def scale_of(t):
    return max(1.0, float(t.detach().double().abs().max()))


def close(a, b, rtol, atol):
    np.testing.assert_allclose(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy(), rtol=rtol, atol=atol)


def bar_close(rtol, atol_of_scale=None, atol=None):
    """test_hip_parity.close(y, ref, rtol, atol_of_scale * scale_of(ref)) (or a plain atol)."""
    return lambda y, ref: close(y, ref, rtol, atol if atol is not None else atol_of_scale * scale_of(ref))


def bar_max(frac):
    """max |y - ref| <= frac * max |ref| (the float32-class bars of the bf16-pipe forms)."""
    def check(y, ref):
        e, sc = float((y.double().cpu() - ref).abs().max()), float(ref.abs().max())
        assert e <= frac * sc, (e / sc, frac)
    return check


def bar_16bit(ulps, atol, ulp=2.0 ** -8):
    """err <= ulps * ulp * |ref| + atol, element by element (ulp: 2^-8 for bf16, 2^-11 for fp16, as tests/test_conv16.py has them)."""
    def check(y, ref):
        err = (y.double().cpu() - ref).abs()
        bound = ulps * ulp * ref.abs() + atol
        assert bool((err <= bound).all()), float((err - bound).max())
    return check


BAR_DIRECT = (bar_close(1e-4, 2e-5), 'test_conv2d_vs_oracle')
BAR_F2 = (bar_close(1e-4, 1e-5), 'test_conv2d_winograd_vs_oracle_and_direct')
BAR_F4 = (bar_close(0, 1e-4), 'test_conv2d_winograd4_kernel')
BAR_F4_TAIL = (bar_close(0, 1e-4), 'test_conv2d_winograd4_tails_vs_oracle')
BAR_DIRECT_TAIL = (bar_close(1e-4, atol=1e-4), 'test_conv2d_fused_prologue_epilogue_vs_oracle')
BAR_TWO = (bar_close(1e-4, atol=1e-4), 'test_conv2d_two_source_equals_concat')
BAR_STREAM = (bar_close(1e-5, 3e-6), 'test_streaming_1x1_conv / test_streaming_1x1_conv_ring')
BAR_UP2 = (bar_close(1e-5, 2e-6), 'test_fused_up2_transposed_conv')
BAR_UP2_X3 = (bar_max(2e-6), 'test_up2_transposed_conv_on_the_bf16_pipe_is_float32_class')
BAR_S2X3 = (bar_max(2e-6), 'test_conv_s2x3 (e <= 2e-6 of the output scale)')
BAR_STEM = (bar_max(2e-6), 'test_stem7_conv_on_the_bf16_pipe_is_float32_class')
BAR_TRANSPOSED = (bar_close(1e-4, 2e-5), 'test_conv_transpose2d_vs_oracle')
BAR_FIR = (bar_close(2e-5, 3e-6), 'test_upfirdn2d_vs_oracle_multi_tile')
BAR_FIR_TAIL = (bar_close(2e-5, atol=2e-5), 'test_upfirdn2d_bias_act_fused_tail')
BAR_BIAS_ACT = (bar_close(2e-6, atol=2e-6), 'test_bias_act_vs_oracle_layouts')
BAR_HEAD = (bar_close(1e-5, 1e-5), 'test_streaming_head_fp32')
BAR_SPADE = (bar_close(2e-5, atol=2e-5), 'test_support_kernels_vs_oracle')
BAR_SPADE_TRAIN = (bar_close(2e-5, 2e-5), 'test_spade_combine_training_route_vs_float64_autograd (y, dgamma / dbeta)')
BAR_SPADE_DX = (bar_close(1e-4, 2e-5), 'test_spade_combine_training_route_vs_float64_autograd (dx)')
BAR_EXACT = (lambda y, ref: torch.testing.assert_close(y.double().cpu(), ref, rtol=0, atol=0), 'test_vgg_loss_gpu (max-pool and the L1 gradient are exact)')
BAR_16 = (bar_16bit(2, 1e-3), 'test_conv16_fused_tail_random')
BAR_16_FP16 = (bar_16bit(2, 1e-3, 2.0 ** -11), 'test_conv16_fused_tail_random')
BAR_UP2F = (bar_16bit(1, 1e-6), 'test_up2_fused_x_kernel_vs_float64')


def bar_roundoff(y, ref):
    """test_spade16_gpu.test_spade_combine16: the stored value is the float64 number rounded once -- within bf16's unit roundoff of it."""
    bound = torch.maximum(ref.abs() * 2.0 ** -8, torch.full_like(ref, 2.0 ** -134))
    assert float(((y.double().cpu() - ref).abs() / bound).max()) <= 1.0


def bar_head16(cin):
    def check(y, ref):
        assert float((y.double().cpu() - ref).abs().max()) <= 2e-4 * max(1.0, (cin / 64) ** 0.5)
    return (check, 'test_conv1x1_small_head')


# ---------------------------------------------------------------------------------------------------------------- the harness

def _extent(t):
    """Elements from the first to one past the last element of `t` in memory."""
    return 1 + sum((s - 1) * abs(st) for s, st in zip(t.shape, t.stride())) if t.numel() else 0


def crossed(t):
    ext = _extent(t)
    return ' '.join(name for name, mark, unit in MARKS if (ext * t.element_size() if unit == 'bytes' else ext) > mark)


def _repeat(t, case, n):
    """The P base samples of `t` (CPU, float32) on the device in the case's dtype and layout, repeated along N to n samples."""
    v = _plain(t, case.dtype, case.layout)
    reps = n // P
    if case.layout == 'nhwc':
        return v.permute(0, 2, 3, 1).repeat(reps, 1, 1, 1).permute(0, 3, 1, 2)
    if case.layout == 'pitched':
        _, c, h, w = v.shape
        return torch.as_strided(v, [P, c, h, v.stride(2)], v.stride()).repeat(reps, 1, 1, 1)[..., :w]
    return v.repeat(reps, *([1] * (v.ndim - 1)))


def _int_view(y):
    return y.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[y.element_size()])


def periodic_mismatch(y, chunk=256):
    """Samples n of y [N, ...] whose bits differ from sample n mod P, compared on the device in chunks of `chunk` periods: (count, first sample)."""
    yb = _int_view(y)
    base = yb[:P].unsqueeze(0)
    bad = []
    for i in range(0, y.shape[0], chunk * P):
        seg = yb[i:i + chunk * P]
        ne = (seg.unflatten(0, (seg.shape[0] // P, P)) != base).flatten(2).any(2).flatten()
        bad.append(ne)
    bad = torch.cat(bad)
    count = int(bad.sum())
    return count, (int(bad.nonzero()[0]) if count else -1)


def _outputs(out):
    return list(out) if isinstance(out, (tuple, list)) else [out]


class Far:
    """One far launch: make() -> Case (built at P samples); n = the batch of the launch; marks = {operand: the marks it crosses} for the inputs by their
    names and the outputs as 'y' ('y0', 'y1', ... when there are several), operands that cross none left out; bar = (check(y, ref), the test it comes
    from), one per output when they differ; gib = device memory the row holds at its peak."""
    def __init__(self, make, n, marks, bar, gib):
        self.make, self.n, self.marks, self.bar, self.gib = make, n, marks, bar, gib


def _need_memory(gib):
    _release()
    free = torch.cuda.mem_get_info()[0]
    if free < gib * GIB:
        pytest.skip(f'the row needs {gib} GiB of device memory, {free / GIB:.1f} GiB are free')


def _release():
    import gc
    gc.collect()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _row():
    """A row frees its tensors before the next; a HIP error ends the whole run (nothing more is started on a device that has faulted)."""
    try:
        yield
    except RuntimeError as e:
        if 'HIP error' in str(e) or 'hipError' in str(e) or 'illegal memory access' in str(e):
            pytest.exit(f'HIP error, the run ends here: {e}', returncode=3)
        raise
    finally:
        _release()


def run_far(row):
    assert row.n % P == 0 and row.n <= 65535 and row.gib <= 24
    _need_memory(row.gib)
    torch.cuda.reset_peak_memory_stats()
    case = row.make()
    gin = {k: _repeat(v, case, row.n) for k, v in case.ins.items()}
    with poisoned_empty():          # every tensor the product allocates starts as NaN: a sample the launch does not write cannot match the base
        outs = _outputs(case.run(gin))
    torch.cuda.synchronize()
    names = ['y'] if len(outs) == 1 else [f'y{i}' for i in range(len(outs))]
    seen = {k: crossed(v) for k, v in gin.items()}
    seen.update({k: crossed(v) for k, v in zip(names, outs)})
    seen = {k: v for k, v in seen.items() if v}
    for name, y in zip(names, outs):
        assert y.shape[0] == row.n, (name, y.shape)
        yb = y[:P].detach().float()
        if yb[0].numel() > 1:          # (a per-launch scalar handed back once per sample is the same for all of them)
            assert not any(torch.equal(yb[i], yb[j]) for i in range(P) for j in range(i)) and all(float(yb[i].abs().max()) > 0 for i in range(P)), f'{name}: the base samples are not distinct and non-zero'
        count, first = periodic_mismatch(y)
        assert count == 0, f'{name}: {count} of {row.n} samples differ from sample n mod {P} in at least one bit, first sample {first} (operands cross {seen})'
    refs = _outputs(case.ref({k: case.rounded(k) for k in case.ins}))
    bars = row.bar if isinstance(row.bar, list) else [row.bar] * len(outs)
    assert len(refs) == len(outs) == len(bars)
    for name, y, ref, (check, _) in zip(names, outs, refs, bars):
        got = y[:P].detach().float().cpu().reshape(ref.shape)
        e, sc = float((got.double() - ref).abs().max()), float(ref.abs().max())
        print(f'far {name}: N {row.n}, max error of the base against float64 {e:.3e} ({e / sc:.2e} of max |ref|), peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB')
        check(got, ref)
    assert seen == row.marks, f'the row states {row.marks}, the launch crossed {seen}'


# ---------------------------------------------------------------------------------------------------------------- factories the locality table lacks

def _randn(gen, *shape):
    return torch.randn(list(shape), generator=gen)


def _labelled(M, fn, want):
    tl = M.start_timeline()
    try:
        y = fn()
    finally:
        M.stop_timeline()
    key = _last_label(tl)
    assert want(key), key
    return y


def _form_label(M, winograd):
    return lambda key: key[:4] == (3, 3, 1, M.WINO_FORMS[winograd][0])


def tail_case(winograd, cin, cout, h, w):
    """The full fused tail of a 3x3 stride-1 launch: in_scale, out_scale, per-sample noise, bias, lrelu, gain, clamp, residual."""
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(300 + winograd)
    ins = {'x': _randn(gen, P, cin, h, w), 'in_scale': torch.rand([P, cin, 1, 1], generator=gen) + 0.5, 'out_scale': torch.rand([P, cout, 1, 1], generator=gen) + 0.5,
           'noise': _randn(gen, P, 1, h, w), 'residual': _randn(gen, P, cout, h, w)}
    wt, bias = _weights(gen, [cout, cin, 3, 3], 9 * cin), _randn(gen, cout)
    packed, bias_d = M.pack_weight(wt.to(DEV), winograd=winograd), bias.to(DEV)

    def run(g):
        return _labelled(M, lambda: M.conv2d_forward(g['x'], packed, cout, 3, 3, pad=(1, 1), winograd=winograd, in_scale=g['in_scale'], out_scale=g['out_scale'],
                                                     noise=g['noise'], noise_gain=0.3, bias=bias_d, act='lrelu', alpha=0.2, gain=GAIN, clamp=2.0, residual=g['residual']),
                         _form_label(M, winograd))

    def ref(i):
        v = F.conv2d(i['x'] * i['in_scale'], wt.double(), padding=1) * i['out_scale'] + i['noise'] * 0.3 + bias.double().reshape(1, -1, 1, 1)
        return (torch.where(v > 0, v, v * 0.2) * GAIN).clamp(-2.0, 2.0) + i['residual']
    return Case(ins, list(ins), run, ref)


def spade_tail_case(winograd, cin, c, h, w):
    """The SPADE tail: gamma and beta from one launch over interleaved rows, (spade_x - mean) rstd (1 + gamma) + beta, then lrelu, gain and clamp."""
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(400 + winograd)
    ins = {'x': _randn(gen, P, cin, h, w), 'spade_x': _randn(gen, P, c, h, w), 'mean': _randn(gen, P, c, 1, 1), 'rstd': torch.rand([P, c, 1, 1], generator=gen) + 0.5}
    wg, wb = _weights(gen, [c, cin, 3, 3], 9 * cin), _weights(gen, [c, cin, 3, 3], 9 * cin)
    packed = M.pack_spade_gamma_beta(wg.to(DEV), wb.to(DEV), winograd=winograd)

    def run(g):
        return _labelled(M, lambda: M.conv2d_forward(g['x'], packed, 2 * c, 3, 3, pad=(1, 1), winograd=winograd, spade=(g['spade_x'], g['mean'].reshape(-1), g['rstd'].reshape(-1)),
                                                     act='lrelu', alpha=0.2, gain=GAIN, clamp=2.0), _form_label(M, winograd))

    def ref(i):
        v = (i['spade_x'] - i['mean']) * i['rstd'] * (1 + F.conv2d(i['x'], wg.double(), padding=1)) + F.conv2d(i['x'], wb.double(), padding=1)
        return (torch.where(v > 0, v, v * 0.2) * GAIN).clamp(-2.0, 2.0)
    return Case(ins, list(ins), run, ref)


def strided_case(k, winograd, cin, cout, h, w, route1x1=None):
    """y = channels [cout, 2 cout) of a tensor of 2 cout channels: ystride[0] alone is twice the dense one.  The other channels must stay as they were."""
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(500 + 10 * k + winograd)
    ins = {'x': _randn(gen, P, cin, h, w)}
    wt = _weights(gen, [cout, cin, k, k], cin * k * k)
    packed = M.pack_weight(wt.to(DEV), winograd=winograd)

    def run(g):
        big = torch.full([g['x'].shape[0], 2 * cout, h, w], 7.0, dtype=torch.float32, device=DEV)
        y = big[:, cout:]
        _labelled(M, lambda: M.conv2d_forward(g['x'], packed, cout, k, k, pad=(k // 2, k // 2), winograd=winograd, y=y), lambda key: key[:4] == (k, k, 1, M.WINO_FORMS[winograd][0]))
        if route1x1 is not None:
            assert M._init().lib.pg_conv2d_last_1x1_route() == ROUTE_1X1[route1x1]
        assert bool((big[:, :cout] == 7.0).all()), 'the launch wrote outside its channel slice'
        return y
    return Case(ins, ['x'], run, lambda i: F.conv2d(i['x'], wt.double(), padding=k // 2))


def fir_generic_case(shape):
    from oracle import ops_ref as R
    from torch_utils.ops import upfirdn2d as U
    gen = torch.Generator().manual_seed(72)
    ins = {'x': _randn(gen, *shape)}
    f = _randn(gen, 5, 3)                      # 2-D, non-separable, odd-sized: the generic kernel
    fd = f.to(DEV)
    kw = dict(up=2, down=3, padding=[2, 1, 3, 0], flip_filter=True, gain=2.0)

    def run(g):
        y = U.upfirdn2d(g['x'], fd, **kw)
        assert U._plugin.lib.pg_upfirdn2d_last_route() == ROUTE_FIR['generic'], U._plugin.lib.pg_upfirdn2d_last_route()
        return y
    return Case(ins, ['x'], run, lambda i: R.upfirdn2d(i['x'], f.double(), **kw))


def bias_act_case(shape, layout='nchw'):
    from oracle import ops_ref as R
    from torch_utils.ops import bias_act as B
    gen = torch.Generator().manual_seed(73)
    ins = {'x': _randn(gen, *shape) * 2}
    b = _randn(gen, shape[1])
    bd = b.to(DEV)
    return Case(ins, ['x'], lambda g: B.bias_act(g['x'], bd, act='lrelu', gain=1.4, clamp=1.5), lambda i: R.bias_act(i['x'], b.double(), act='lrelu', gain=1.4, clamp=1.5), layout=layout)


def small_case(cin, h, w, cout=3, split=False):
    """pg_conv1x1_small with styles, bias, skip and clamp; `split`: the channel-split form (Cin >= 64 on images that leave half of the CUs idle)."""
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(74 + cin)
    ins = {'x': _randn(gen, P, cin, h, w), 'styles': _randn(gen, P, cin, 1, 1) + 1.5, 'skip': _randn(gen, P, cout, h, w)}
    wt, b = _randn(gen, cout, cin, 1, 1) / math.sqrt(cin), _randn(gen, cout)
    wd, bd = wt.to(DEV), b.to(DEV)

    def run(g):
        n = g['x'].shape[0]
        assert M.conv1x1_small_ok(g['x'], wd, g['skip'])
        assert split == (cin >= 64 and n * ((h * w // 4 + 255) // 256) < torch.cuda.get_device_properties(0).multi_processor_count // 2)
        return M.conv1x1_small(g['x'], wd, styles=g['styles'].reshape(n, cin), bias=bd, skip=g['skip'], scale=0.7, clamp=0.8)

    def ref(i):
        v = F.conv2d(i['x'] * i['styles'], wt.double() * 0.7) + b.double().reshape(1, -1, 1, 1)
        return v.clamp(-0.8, 0.8) + i['skip']
    return Case(ins, list(ins), run, ref)


def fold_case(kind, c, h, w):
    """conv1x1_fold_heads (two inputs, two outputs) / conv3x3_fold_head over per-sample weights [N, Cout, C] that the test supplies."""
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(75)
    cout = 6 if kind == '1x1' else 3
    ctot = 2 * c if kind == '1x1' else 10 * c
    ins = {'xa': _randn(gen, P, c, h, w), 'xb': _randn(gen, P, c, h, w), 'skip': _randn(gen, P, 3, h, w), 'w': _randn(gen, P, cout, ctot, 1) / math.sqrt(ctot), 'b': _randn(gen, P, cout, 1, 1)}

    def run(g):
        n = g['xa'].shape[0]
        wn, bn = g['w'].reshape(n, cout, ctot), g['b'].reshape(n, cout)
        if kind == '1x1':
            assert M.conv1x1_fold_ok(g['xa'], g['xb'], g['skip'])
            return M.conv1x1_fold_heads(g['xa'], g['xb'], wn, bn, 3, skip=g['skip'], clamp=2.0)
        assert M.conv3x3_fold_ok(g['xa'], g['xb'], g['skip'])
        return M.conv3x3_fold_head(g['xa'], g['xb'], wn, bn, skip=g['skip'], clamp=2.0)

    def ref(i):
        wn, bn = i['w'].reshape(P, cout, ctot), i['b'].reshape(P, cout, 1, 1)
        if kind == '1x1':
            v = torch.einsum('noc,nchw->nohw', wn, torch.cat([i['xa'], i['xb']], 1)) + bn
            v = v.clamp(-2.0, 2.0)
            return [v[:, :3] + i['skip'], v[:, 3:]]
        taps = F.unfold(i['xa'], 3, padding=1).reshape(P, 9 * c, h, w)          # channel-major, taps 3 ky + kx inside: w[n, o, 9 c + 3 ky + kx]
        v = torch.einsum('noc,nchw->nohw', wn[:, :, :9 * c], taps) + torch.einsum('noc,nchw->nohw', wn[:, :, 9 * c:], i['xb']) + bn
        return v.clamp(-2.0, 2.0) + i['skip']
    return Case(ins, list(ins), run, ref)


def stats_case(kind, c, h, w):
    """pg_instance_norm_stats, pg_spade_norm, pg_spade_train_forward, pg_spade_train_backward (mean / rstd of x gathered by the first)."""
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(76)
    ins = {'x': _randn(gen, P, c, h, w) * 2 + 0.5}
    if kind != 'stats':
        ins['gb'] = _randn(gen, P, 2 * c, h, w)
    if kind == 'train_backward':
        ins['dy'] = _randn(gen, P, c, h, w)

    def run(g):
        n = g['x'].shape[0]
        mean, rstd = M.instance_norm_stats(g['x'], 1e-5)
        if kind == 'stats':
            return mean.view(n, c), rstd.view(n, c)
        if kind == 'norm':
            return M.spade_norm(g['x'], mean, rstd, g['gb'][:, :c].contiguous(), g['gb'][:, c:].contiguous())
        if kind == 'train_forward':
            return M.spade_train_forward(g['x'], mean, rstd, g['gb'])
        return M.spade_train_backward(g['dy'], g['x'], mean, rstd, g['gb'])

    def ref(i):
        if kind == 'stats':
            return [i['x'].mean([2, 3]), (i['x'].var([2, 3], unbiased=False) + 1e-5).rsqrt()]
        x, gb = i['x'].clone().requires_grad_(True), i['gb'].clone().requires_grad_(True)
        y = F.instance_norm(x, eps=1e-5) * (1 + gb[:, :c]) + gb[:, c:]
        if kind != 'train_backward':
            return y.detach()
        return list(torch.autograd.grad(y, [x, gb], i['dy']))
    return Case(ins, list(ins), run, ref)


def vgg_case(kind, c, h, w):
    from torch_utils.ops import vgg_ops as V
    gen = torch.Generator().manual_seed(77)
    if kind == 'maxpool':
        ins = {'x': _randn(gen, P, c, h, w), 'dy': _randn(gen, P, c, h // 2, w // 2)}

        def run(g):
            xr = g['x'].requires_grad_(True)
            y = V.maxpool2x2(xr)
            return y.detach(), torch.autograd.grad(y, xr, g['dy'])[0]

        def ref(i):
            xr = i['x'].clone().requires_grad_(True)
            y = F.max_pool2d(xr, 2)
            return [y.detach(), torch.autograd.grad(y, xr, i['dy'])[0]]
        return Case(ins, list(ins), run, ref)
    ins = {'x': _randn(gen, P, c, h, w), 't': _randn(gen, P, c, h, w)}

    def run(g):          # one group: the mean over every sample (the same number for each of them: handed back once per sample), and its gradient
        xr = g['x'].requires_grad_(True)
        out = V.l1_mean(xr, g['t'], groups=1)
        dx, = torch.autograd.grad(out, xr, torch.tensor([0.7], device=DEV))
        return dx * float(xr.numel()), out.detach().reshape(1, 1).expand(xr.shape[0], 1)

    def ref(i):          # sign(x - t) * 0.7 (the kernel's 0.7 / numel, scaled back: a float32 product, so the bar is one rounding); the mean over N periodic samples is the base's
        return [torch.sign(i['x'] - i['t']) * float(np.float32(0.7)), (i['x'] - i['t']).abs().mean().reshape(1, 1).expand(P, 1)]
    return Case(ins, list(ins), run, ref)


def head16_case(cin, h, w):
    """conv1x1_head16.hip: the lane-spread three-channel head on bf16 channels-last features."""
    from torch_utils.ops import conv2d_mfma16 as M16
    gen = torch.Generator().manual_seed(78)
    ins = {'x': _randn(gen, P, cin, h, w)}
    wt, st, b = _randn(gen, 3, cin) / math.sqrt(cin), _randn(gen, P, cin) + 1.5, _randn(gen, 3)
    wd, bd = wt.to(DEV), b.to(DEV)

    def run(g):
        n = g['x'].shape[0]
        return M16.conv1x1_small(g['x'], wd, styles=st.to(DEV).repeat(n // P, 1), bias=bd, skip=None, clamp=0.8)

    def ref(i):
        v = torch.einsum('oc,nchw->nohw', wt.double(), i['x'] * st.double().reshape(P, cin, 1, 1)) + b.double().reshape(1, -1, 1, 1)
        return v.clamp(-0.8, 0.8)
    return Case(ins, ['x'], run, ref, dtype=torch.bfloat16, layout='nhwc')


def up2f16_case(cin, cout, h, w):
    """pg_conv2d16_up2_fused on small-integer operands, as test_up2_fused_x_kernel_vs_float64 runs it: every product and partial sum is exact in float32 (the
    kernel folds the filter's y half into its 16-bit weights, which random weights would round), the only error left is the final rounding to bf16."""
    from oracle import ops_ref as R
    from torch_utils.ops import conv2d_mfma as M
    from torch_utils.ops import conv2d_mfma16 as M16
    from training import networks as PN
    gen = torch.Generator().manual_seed(83)
    ints = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=gen).float()
    ins = {'x': ints([P, cin, h, w], -2, 2)}
    wt = ints([cin, cout, 3, 3], -2, 2)          # IOHW
    f2d = torch.outer(torch.tensor([1., 3., 3., 1.]), torch.tensor([1., 3., 3., 1.])) / 64
    fy, fx = PN._separable_taps(f2d)
    packed, per, _ = M16.pack_weight(PN._up2_fused_weights(wt.to(DEV), fy), torch.bfloat16, transpose_oi=True)

    def run(g):
        return _labelled(M, lambda: M16.conv_up2_fused(g['x'], packed, cout, [2.0 * float(v) for v in fx], sample_stride=per), lambda key: key[3] == 'mfma16' and 'up2 fused-x' in key[4])
    return Case(ins, ['x'], run, lambda i: R.upfirdn2d(F.conv_transpose2d(i['x'], wt.double(), stride=2), f2d.double(), padding=1, gain=4), dtype=torch.bfloat16, layout='nhwc')


def conv16_fp16_case(cin, cout, h, w):
    """`conv16_case('k3s1')` in fp16."""
    from torch_utils.ops import conv2d_mfma as M
    from torch_utils.ops import conv2d_mfma16 as M16
    gen = torch.Generator().manual_seed(84)
    ins = {'x': _randn(gen, P, cin, h, w)}
    wt = _weights(gen, [cout, cin, 3, 3], 9 * cin)
    packed, _, _ = M16.pack_weight(wt.to(DEV), torch.float16)

    def run(g):
        return _labelled(M, lambda: M16.conv2d_forward(g['x'], packed, cout, 3, 3, pad=(1, 1)), lambda key: key[:4] == (3, 3, 1, 'mfma16'))
    return Case(ins, ['x'], run, lambda i: F.conv2d(i['x'], wt.half().double(), padding=1), dtype=torch.float16, layout='nhwc')


def stats16_case(kind, c, h, w):
    from torch_utils.ops import conv2d_mfma16 as M16
    gen = torch.Generator().manual_seed(79)
    ins = {'x': _randn(gen, P, c, h, w) * 2 + 0.5}
    if kind == 'combine':          # (mean / rstd are float32 operands of the kernel: kept out of `ins`, whose tensors are rounded to bf16)
        ins['gb'] = _randn(gen, P, 2 * c, h, w)
        mean, rstd = _randn(gen, P * c) * 0.5, torch.rand([P * c], generator=gen) + 0.25

    def run(g):
        n = g['x'].shape[0]
        if kind == 'stats':
            m, r = M16.instance_norm_stats16(g['x'], 1e-5)
            return m.view(n, c), r.view(n, c)
        return M16.spade_combine16(g['x'], mean.to(DEV).repeat(n // P), rstd.to(DEV).repeat(n // P), g['gb'], act='relu', gain=GAIN)

    def ref(i):
        if kind == 'stats':
            return [i['x'].mean([2, 3]), (i['x'].var([2, 3], unbiased=False) + 1e-5).rsqrt()]
        v = (i['x'] - mean.double().view(P, c, 1, 1)) * rstd.double().view(P, c, 1, 1) * (1 + i['gb'][:, :c]) + i['gb'][:, c:]
        return v.clamp(min=0) * float(np.float32(GAIN))
    return Case(ins, list(ins), run, ref, dtype=torch.bfloat16, layout='nhwc')


# ---------------------------------------------------------------------------------------------------------------- the far rows

F2, F4, F4B, F4X3 = (lambda: _wino('WINO_F2')), (lambda: _wino('WINO_F4')), (lambda: _wino('WINO_F4B')), (lambda: _wino('WINO_F4X3'))
# Two geometries of the 3x3 / 1x1 rows at 64 x 64.  A: 64 -> 16 channels, N = 8202 -- x (1 MiB a sample) past all three marks, y past 2 GiB.
# B: 16 -> 64 channels, N = 8190 -- y 8190 MiB, two samples below the 2^31 - 1 ELEMENTS that pg_conv2d_forward admits for y (conv2d.hip: `ext`), past 2 and 4 GiB.
A, B = dict(x=ALL, y='31'), dict(y='31 32')
FAR = {
    # ---- fp32 forward
    'direct_3x3_s1_p1/x': Far(lambda: conv_case(P, 64, 16, 64, 64, 3, pad=1), 8202, A, BAR_DIRECT, 11),
    'direct_3x3_s1_p1/y': Far(lambda: conv_case(P, 16, 64, 64, 64, 3, pad=1), 8190, B, BAR_DIRECT, 11),
    'direct_3x3_s1_p1/strided_y': Far(lambda: strided_case(3, 0, 16, 32, 64, 64), 8190, B, BAR_DIRECT, 11),
    # (N = 65535 at 144 x 64, 2 -> 2 channels: the per-sample noise plane, 36 KiB a sample, passes 2 GiB only there; y and the residual pass 4 GiB)
    'direct_3x3_s1_p1/tail': Far(lambda: tail_case(0, 2, 2, 144, 64), 65535, dict(x='31 32', noise='31', residual='31 32', y='31 32'), BAR_DIRECT_TAIL, 17),
    'direct_1x1/x': Far(lambda: conv_case(P, 64, 16, 64, 64, 1, route1x1='tiled'), 8202, A, BAR_DIRECT, 11),
    'direct_1x1/y': Far(lambda: conv_case(P, 16, 128, 64, 64, 1, route1x1='tiled'), 4092, B, BAR_DIRECT, 10),
    'stream_1x1/x': Far(lambda: conv_case(P, 64, 32, 64, 64, 1, route1x1='stream'), 8202, dict(x=ALL, y='31 32'), BAR_STREAM, 13),
    'stream_1x1/y': Far(lambda: conv_case(P, 16, 64, 64, 64, 1, route1x1='stream'), 8190, B, BAR_STREAM, 11),
    'stream_1x1/strided_y': Far(lambda: strided_case(1, 0, 16, 32, 64, 64, route1x1='stream'), 8190, B, BAR_STREAM, 11),
    'stream_1x1_ring': Far(lambda: conv_case(P, 128, 64, 64, 64, 1, route1x1='ring'), 4101, dict(x=ALL, y='31 32'), BAR_STREAM, 13),
    # (three input channels: x passes 2^31 elements only with FEWER output channels, 3 -> 2 at 128 x 128)
    'direct_7x7_p3_fp32': Far(lambda: conv_case(P, 3, 2, 128, 128, 7, pad=3), 43800, dict(x=ALL, y='31 32'), BAR_DIRECT, 14),
    'direct_3x3_s2_p0_fp32': Far(lambda: conv_case(P, 16, 64, 65, 65, 3, stride=2), 32766, dict(x=ALL, y='31 32'), BAR_DIRECT, 17),
    'two_source': Far(lambda: conv_case(P, 64, 8, 64, 64, 3, pad=1, x2c=32), 16401, dict(x=ALL, x2=ALL, y='31'), BAR_TWO, 19),
    'wino_f2/x': Far(lambda: conv_case(P, 64, 16, 64, 64, 3, pad=1, winograd=F2()), 8202, A, BAR_F2, 11),
    # (the F(2x2) tail adds 32-bit byte offsets to a per-sample base: with the sample base inside those 32 bits, the samples past 4 GiB land on the first ones)
    'wino_f2/y': Far(lambda: conv_case(P, 16, 64, 64, 64, 3, pad=1, winograd=F2()), 8190, B, BAR_F2, 11),
    'wino_f2/strided_y': Far(lambda: strided_case(3, F2(), 16, 32, 64, 64), 8190, B, BAR_F2, 11),
    'wino_f4_a/x': Far(lambda: conv_case(P, 64, 16, 64, 64, 3, pad=1, winograd=F4()), 8202, A, BAR_F4, 11),
    'wino_f4_a/y': Far(lambda: conv_case(P, 16, 64, 64, 64, 3, pad=1, winograd=F4()), 8190, B, BAR_F4, 11),
    'wino_f4_a/strided_y': Far(lambda: strided_case(3, F4(), 16, 32, 64, 64), 8190, B, BAR_F4, 11),
    'wino_f4b_a/x': Far(lambda: conv_case(P, 64, 16, 64, 64, 3, pad=1, winograd=F4B()), 8202, A, BAR_F4, 11),
    'wino_f4b_a/y': Far(lambda: conv_case(P, 16, 64, 64, 64, 3, pad=1, winograd=F4B()), 8190, B, BAR_F4, 11),
    'wino_f4b_a/strided_y': Far(lambda: strided_case(3, F4B(), 16, 32, 64, 64), 8190, B, BAR_F4, 11),
    'wino_f4b_a/tail': Far(lambda: tail_case(F4B(), 2, 2, 144, 64), 65535, dict(x='31 32', noise='31', residual='31 32', y='31 32'), BAR_F4_TAIL, 17),
    'wino_f4b_a/spade_tail': Far(lambda: spade_tail_case(F4B(), 16, 32, 12, 64), 65535, dict(x='31', spade_x='31 32', y='31 32'), BAR_F4_TAIL, 16),
    'wino_f4x3_a/x': Far(lambda: conv_case(P, 64, 16, 64, 64, 3, pad=1, winograd=F4X3()), 8202, A, BAR_F4, 11),
    'wino_f4x3_a/y': Far(lambda: conv_case(P, 16, 64, 64, 64, 3, pad=1, winograd=F4X3()), 8190, B, BAR_F4, 11),
    'wino_f4x3_a/strided_y': Far(lambda: strided_case(3, F4X3(), 16, 32, 64, 64), 8190, B, BAR_F4, 11),
    'wino_f4x3_a/tail': Far(lambda: tail_case(F4X3(), 2, 2, 144, 64), 65535, dict(x='31 32', noise='31', residual='31 32', y='31 32'), BAR_F4_TAIL, 17),
    'wino_f4x3_a/spade_tail': Far(lambda: spade_tail_case(F4X3(), 16, 32, 12, 64), 65535, dict(x='31', spade_x='31 32', y='31 32'), BAR_F4_TAIL, 16),
    # (the up = 2 entries put no bound on y: the pitched [N, 16, 65, 68] output passes 2^31 elements as well)
    'up2_fp32': Far(lambda: up2_case(P, 64, 16, 32, 32, x3=False), 32802, dict(x=ALL, y=ALL), BAR_UP2, 18),
    'up2_x3_edge_column': Far(lambda: up2_case(P, 64, 16, 32, 32, x3=True, edge_column=True), 32802, dict(x=ALL, y=ALL), BAR_UP2_X3, 18),
    's2x3': Far(lambda: conv_case(P, 32, 64, 65, 65, 3, stride=2, s2x3=True, no_grad=True), 16401, dict(x=ALL, y='31 32'), BAR_S2X3, 13),
    'stem7': Far(lambda: stem_case(P, 2, 128, 128), 43800, dict(x=ALL, y='31 32'), BAR_STEM, 14),
    'transposed_phases': Far(lambda: transposed_case(P, 64, 16, 32, 32, 1), 32802, dict(x=ALL, y='31 32'), BAR_TRANSPOSED, 16),
    # ---- heads and folds (N <= 65535 is their guard: gridDim.y)
    'pg_conv1x1_small': Far(lambda: small_case(32, 128, 64, cout=8), 8202, dict(x=ALL, skip='31', y='31'), BAR_HEAD, 13),
    'pg_conv1x1_small/split': Far(lambda: small_case(64, 8, 8, split=True), 63, {}, BAR_HEAD, 1),        # (the split form serves launches that leave CUs idle: it cannot be far)
    'conv1x1_fold': Far(lambda: fold_case('1x1', 16, 128, 64), 16401, dict(xa=ALL, xb=ALL), BAR_HEAD, 21),
    'conv3x3_fold': Far(lambda: fold_case('3x3', 16, 128, 64), 16401, dict(xa=ALL, xb=ALL), BAR_HEAD, 21),
    # ---- FIR (no bound on either side: x and y pass whatever 24 GiB hold)
    'fir_up2': Far(lambda: fir_case('up2', (P, 4, 128, 128)), 16401, dict(x='31 32', y=ALL), BAR_FIR, 21),
    'fir_down2': Far(lambda: fir_case('down2', (P, 16, 128, 128)), 8202, dict(x=ALL, y='31'), BAR_FIR, 11),
    'fir_blur': Far(lambda: fir_case('blur', (P, 16, 128, 136)), 8202, dict(x=ALL, y=ALL), BAR_FIR, 18),          # (136 columns: no multiple of the 16-byte blur kernel's 128-column tile)
    'fir_blur4_pitched': Far(lambda: fir_case('blur', (P, 2, 129, 257), layout='pitched', route='blur4', padding=[1, 1, 1, 1]), 32802, dict(x=ALL, y=ALL), BAR_FIR, 17),
    'fir_blur_channels_last': Far(lambda: fir_case('blur', (P, 16, 128, 128), layout='nhwc', route='channels_last'), 8202, dict(x=ALL, y=ALL), BAR_FIR, 17),
    'fir_bias_act': Far(lambda: fir_case('bias_act', (P, 16, 128, 136)), 8202, dict(x=ALL, y=ALL), BAR_FIR_TAIL, 18),
    'fir_generic': Far(lambda: fir_generic_case((P, 16, 128, 128)), 8202, dict(x=ALL, y='31'), BAR_FIR, 13),
    # ---- bias_act forward
    'bias_act': Far(lambda: bias_act_case((P, 16, 128, 128)), 8202, dict(x=ALL, y=ALL), BAR_BIAS_ACT, 17),
    'bias_act_channels_last': Far(lambda: bias_act_case((P, 16, 128, 128), layout='nhwc'), 8202, dict(x=ALL, y=ALL), BAR_BIAS_ACT, 17),
    # ---- statistics and SPADE
    'pg_instance_norm_stats': Far(lambda: stats_case('stats', 16, 128, 128), 8202, dict(x=ALL), [(bar_close(1e-6, atol=1e-6), 'test_support_kernels_vs_oracle'), (bar_close(2e-5, atol=0), 'test_conv2d_winograd4_output_statistics (rstd)')], 9),
    'pg_spade_norm': Far(lambda: stats_case('norm', 16, 64, 64), 8202, dict(x='31', gb='31 32', y='31'), BAR_SPADE, 13),
    'pg_spade_train_forward': Far(lambda: stats_case('train_forward', 16, 128, 64), 8202, dict(x='31 32', gb=ALL, y='31 32'), BAR_SPADE_TRAIN, 17),
    'pg_spade_train_backward': Far(lambda: stats_case('train_backward', 16, 64, 64), 8202, dict(x='31', gb='31 32', dy='31', y0='31', y1='31 32'), [BAR_SPADE_DX, BAR_SPADE_TRAIN], 15),
    # ---- VGG
    'vgg_maxpool': Far(lambda: vgg_case('maxpool', 16, 128, 128), 8202, dict(x=ALL, dy='31', y0='31', y1=ALL), BAR_EXACT, 21),
    'vgg_l1_pair': Far(lambda: vgg_case('l1', 16, 128, 64), 8202, dict(x='31 32', t='31 32', y0='31 32'), [(bar_close(2.0 ** -22, atol=0), 'test_l1_mean (dx exact there; here scaled back by numel: two float32 roundings)'), (bar_close(2e-6, atol=0), 'test_l1_mean')], 14),
    # ---- 16-bit forward (bf16, channels-last).  pg_conv2d16_forward puts the WHOLE x behind one descriptor (<= 2^31 - 1 bytes) and bounds y by 2^30 - 1 elements: no mark is
    # reachable, the rows run at the largest even batch both guards accept -- offsets up to the last kilobytes below 2^31.
    'bf16_k3s1': Far(lambda: conv16_case('k3s1', P, 32, 32, 64, 64), 8190, {}, BAR_16, 5),
    'bf16_k1s1': Far(lambda: conv16_case('k1s1', P, 32, 32, 64, 64), 8190, {}, BAR_16, 5),
    'bf16_k3s2': Far(lambda: conv16_case('k3s2', P, 64, 64, 64, 64), 4092, {}, BAR_16, 4),
    'bf16_up2f': Far(lambda: up2f16_case(32, 32, 16, 30), 17475, {}, BAR_UP2F, 4),
    'fp16_k3s1': Far(lambda: conv16_fp16_case(32, 32, 64, 64), 8190, {}, BAR_16_FP16, 5),
    # (the heads and the 16-bit statistics take int64 sample bases: bounded by N <= 65535 and by memory only)
    'conv1x1_head16': Far(lambda: head16_case(64, 128, 128), 4200, dict(x=ALL), bar_head16(64), 9),
    'pg_instance_norm_stats_cl16': Far(lambda: stats16_case('stats', 32, 128, 128), 4200, dict(x=ALL), [(bar_close(1e-6, atol=1e-6), 'test_spade16_gpu._check_stats'), (bar_close(2e-5, atol=0), 'test_spade16_gpu._check_stats')], 5),
    # (pg_spade_combine_cl16: N * HW * C / 8 <= 2^31 - 1 vectors of eight channels admits every mark)
    'pg_spade_combine_cl16': Far(lambda: stats16_case('combine', 32, 128, 64), 8202, dict(x=ALL, gb=ALL, y=ALL), (bar_roundoff, 'test_spade_combine16'), 17),
}


@pytest.fixture(scope='module')
def native():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    from torch_utils.ops import conv2d_mfma
    assert conv2d_mfma._init() is not None
    yield
    _release()


@pytest.mark.gpu
@pytest.mark.parametrize('row', list(FAR))
def test_far_samples_repeat_the_base_bit_for_bit(row, native):
    with _row():
        run_far(FAR[row])


# ---------------------------------------------------------------------------------------------------------------- tall images: the 32-bit side inside ONE image

class Tall:
    """One or two samples whose single image lies just under the entry's per-image guard: the smallest channel count the route takes, a large H.  x is a band of
    `t_in` rows repeated down the image, so interior output rows repeat with period `t_out` bit for bit (both multiples of every tile height); the float64
    reference is computed on strips only -- the top rows, the rows around each mark an operand crosses, the bottom rows -- from the x rows each depends on.
    make() -> (op(x) -> y asserting the route, ref(float64 strip of x) -> the same operation on the strip as if it were an image); out_rows(i) = the first
    output row that x row i (even) maps to (i for the stride-1 forms, i / 2 at stride 2, 2 i for up = 2)."""
    def __init__(self, make, n, cin, h, w, t_in, t_out, out_rows, marks, bar, gib):
        self.make, self.n, self.cin, self.h, self.w, self.t_in, self.t_out, self.out_rows, self.marks, self.bar, self.gib = make, n, cin, h, w, t_in, t_out, out_rows, marks, bar, gib


def _mark_rows(t):
    """The image rows of `t` [N, C, H, W] (unit x stride) in which a mark it crosses falls."""
    rows = []
    ext = _extent(t)
    for _, mark, unit in MARKS:
        el = mark // t.element_size() if unit == 'bytes' else mark
        if el < ext:
            rows.append(el % t.stride(0) % t.stride(1) // t.stride(2))
    return rows


def tall_conv(k, winograd, cin, cout, stride=1, route1x1=None, s2x3=False):
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(900 + 10 * k + winograd + stride)
    wt = _weights(gen, [cout, cin, k, k], cin * k * k)
    packed = M.pack_weight(wt.to(DEV), winograd=winograd)
    pad = k // 2 if stride == 1 else 0

    def op(x):
        with torch.no_grad():
            y = _labelled(M, lambda: M.conv2d_forward(x, packed, cout, k, k, stride=stride, pad=(pad, pad), winograd=winograd, s2x3=(None if s2x3 else False)),
                          lambda key: key[:4] == (k, k, stride, M.WINO_FORMS[winograd][0]) and key[4].endswith(' s2x3') == s2x3)
        if route1x1 is not None:
            assert M._init().lib.pg_conv2d_last_1x1_route() == ROUTE_1X1[route1x1]
        return y
    return op, lambda xs: F.conv2d(xs, wt.double(), stride=stride, padding=pad)


def tall_up2(cin, cout):
    from torch_utils.ops import conv2d_mfma as M
    gen = torch.Generator().manual_seed(950)
    wt = _weights(gen, [cout, cin, 3, 3], 9 * cin)
    packs = M.pack_up2(wt.to(DEV))
    op = lambda x: _labelled(M, lambda: M.conv_up2_forward(x, packs, cout, x3=False), lambda key: ' up2' in key[4] and ' x3' not in key[4])
    return op, lambda xs: F.conv_transpose2d(xs, wt.double().transpose(0, 1), stride=2)


def tall_fir():
    from oracle import ops_ref as R
    from torch_utils.ops import upfirdn2d as U
    f = U.setup_filter([1, 3, 3, 1])
    fd = f.to(DEV)

    def op(x):
        y = U.upfirdn2d(x, fd, padding=[2, 1, 2, 1])
        assert U._plugin.lib.pg_upfirdn2d_last_route() == ROUTE_FIR['tiled'], U._plugin.lib.pg_upfirdn2d_last_route()
        return y
    return op, lambda xs: R.upfirdn2d(xs, f.double(), padding=[2, 1, 2, 1])


_same, _half, _twice = (lambda i: i), (lambda i: i // 2), (lambda i: 2 * i)
# x images of 16 x 493376 x 68 floats: 2^31 - 311296 bytes (pg_conv2d_forward admits 2^31 - 1); y images of 32 channels: twice that (the Winograd tails admit 2^32 - 1),
# and two samples of them are 2^31 - 311296 ELEMENTS (pg_conv2d_forward admits 2^31 - 1).  68 columns, 136 for the FIR: a band is no power of two in bytes, so an
# offset truncated at a mark lands in another column and another row of the band.
TALL = {
    'direct_3x3_s1_p1': Tall(lambda: tall_conv(3, 0, 16, 32), 2, 16, 493376, 68, 64, 64, _same, dict(x='31', y='31 32'), BAR_DIRECT, 14),
    'wino_f2': Tall(lambda: tall_conv(3, F2(), 16, 32), 2, 16, 493376, 68, 64, 64, _same, dict(x='31', y='31 32'), BAR_F2, 14),
    'wino_f4b_a': Tall(lambda: tall_conv(3, F4B(), 16, 32), 2, 16, 493376, 68, 64, 64, _same, dict(x='31', y='31 32'), BAR_F4, 14),
    'wino_f4x3_a': Tall(lambda: tall_conv(3, F4X3(), 16, 32), 2, 16, 493376, 68, 64, 64, _same, dict(x='31', y='31 32'), BAR_F4, 14),
    'stream_1x1': Tall(lambda: tall_conv(1, 0, 16, 32, route1x1='stream'), 2, 16, 493376, 68, 64, 64, _same, dict(x='31', y='31 32'), BAR_STREAM, 14),
    # (conv2d_inst_up2.hip: one image of x <= 2^31 - 1 bytes, no bound on y -- one image of y, 16 x 2097025 rows of 68 floats, passes every mark)
    'up2_fp32': Tall(lambda: tall_up2(16, 16), 1, 16, 1048512, 32, 64, 128, _twice, dict(y=ALL), BAR_UP2, 12),
    # (conv2d_s2x3.h: (Cin H W + 4) * 4 bytes below 2^31 - 1, Cin >= 32)
    's2x3': Tall(lambda: tall_conv(3, 0, 32, 32, stride=2, s2x3=True), 2, 32, 258049, 65, 128, 64, _half, dict(x='31'), BAR_S2X3, 6),
    # (pg_upfirdn2d bounds one AXIS by 2^31 - 1 coordinates, not the plane: ONE plane of 15790400 x 136 floats passes every mark)
    'fir_blur': Tall(tall_fir, 1, 1, 15790400, 136, 64, 64, _same, dict(x=ALL, y=ALL), BAR_FIR, 18),
}


@pytest.mark.gpu
@pytest.mark.parametrize('row', list(TALL))
def test_tall_images_repeat_their_band_bit_for_bit(row, native):
    r = TALL[row]
    _need_memory(r.gib)
    torch.cuda.reset_peak_memory_stats()
    with _row():
        op, ref = r.make()
        band = torch.randn([r.n, r.cin, r.t_in, r.w], generator=torch.Generator().manual_seed(97))
        x = band.to(DEV).repeat(1, 1, -(-r.h // r.t_in), 1)
        if x.shape[2] != r.h:
            x = x[:, :, :r.h].contiguous()
        with poisoned_empty():
            y = op(x)
        torch.cuda.synchronize()
        oh = y.shape[2]
        # interior rows repeat with period t_out
        k = (oh - 2 * r.t_out) // r.t_out
        assert k > 1000
        yb = _int_view(y)
        first, bad = yb[:, :, r.t_out:2 * r.t_out].unsqueeze(2), 0
        for j in range(0, k, 4096):
            kk = min(4096, k - j)
            seg = yb[:, :, r.t_out * (1 + j):r.t_out * (1 + j + kk)].unflatten(2, (kk, r.t_out))
            ne = (seg != first).flatten(3).any(3).any(1).any(0)
            if bool(ne.any()):
                bad += int(ne.sum())
                print(f'tall {row}: first differing period {j + int(ne.nonzero()[0])} of {k} (output row {r.t_out * (1 + j + int(ne.nonzero()[0]))})')
        assert bad == 0, f'{bad} of {k} interior periods of {r.t_out} output rows differ from the first in at least one bit'
        # float64 on strips: top, around each mark of x and of y, bottom
        length = 16
        starts = {0, oh - length} | {min(max(q - length // 2, 0), oh - length) for q in _mark_rows(y)} | {min(max(r.out_rows(q) - length // 2, 0), oh - length) for q in _mark_rows(x)}
        worst = 0.0
        for a in sorted(starts):
            i0 = max(0, (a * r.t_in // r.t_out - 8) // 2 * 2)
            i1 = min(r.h, (a + length) * r.t_in // r.t_out + 10)
            want = ref(x[:, :, i0:i1].double().cpu())
            g0 = r.out_rows(i0)
            assert 0 <= a - g0 and a - g0 + length <= want.shape[2], (a, i0, i1, g0, want.shape)
            got, want = y[:, :, a:a + length].float().cpu(), want[:, :, a - g0:a - g0 + length]
            worst = max(worst, float((got.double() - want).abs().max()) / float(want.abs().max()))
            r.bar[0](got, want)
        print(f'tall {row}: {k} interior periods, strips at output rows {sorted(starts)}, worst error {worst:.2e} of the strip maximum, peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB')
        seen = {k_: v for k_, v in (('x', crossed(x)), ('y', crossed(y))) if v}
        assert seen == r.marks, f'the row states {r.marks}, the launch crossed {seen}'
        del x, y, yb, first, seg, ne


# ---------------------------------------------------------------------------------------------------------------- weight gradients: the result sums over N

def _live_samples(n, sample_bytes):
    """The first, the last, and the two samples on either side of each byte / element mark of a tensor of n samples of `sample_bytes` (4-byte elements)."""
    live = {0, n - 1}
    for _, mark, unit in MARKS:
        s = (mark * 4 if unit == 'elements' else mark) // sample_bytes
        live |= {i for i in (s - 1, s) if 0 <= i < n}
    return live


# (N, Cin, Cout, H, W, k, stride, bf16x3, marks, GiB).  The bf16x3 route keeps three bf16 planes of x and of dy beside them (2.5 x the bytes): 24 GiB hold x past 4 GiB.
WGRAD = {
    'wgrad_3x3_s1/x': (8202, 64, 16, 64, 64, 3, 1, False, dict(x=ALL, dy='31'), 11),
    'wgrad_3x3_s1/dy': (8202, 16, 64, 64, 64, 3, 1, False, dict(x='31', dy=ALL), 11),
    'wgrad_1x1/x': (8202, 64, 16, 64, 64, 1, 1, False, dict(x=ALL, dy='31'), 11),
    'wgrad_1x1/dy': (8202, 16, 64, 64, 64, 1, 1, False, dict(x='31', dy=ALL), 11),
    'wgrad_3x3_s2': (32802, 16, 64, 65, 65, 3, 2, False, dict(x=ALL, dy=ALL), 17),
    'wgrad_bf16x3_s1/x': (4200, 64, 16, 64, 64, 3, 1, True, dict(x='31 32'), 14),                  # (pg_split3_bf16_cl: its planes of x, 3 x 2 bytes an element, pass 4 GiB too)
    'wgrad_bf16x3_s1/dy': (4200, 16, 64, 64, 64, 3, 1, True, dict(dy='31 32'), 14),
    'wgrad_bf16x3_s2': (16401, 16, 64, 65, 65, 3, 2, True, dict(x='31 32', dy='31 32'), 23),
}


@pytest.mark.gpu
@pytest.mark.parametrize('row', list(WGRAD))
def test_far_weight_gradient(row, native):
    """dw <= 1e-5 (fp32 kernel) / 4e-6 (bf16x3) of the tensor's largest element: the bars of test_config4_layer_gradients_replayed_in_float64."""
    from torch_utils.ops import conv2d_mfma as M
    n, cin, cout, h, w, k, stride, bf16x3, marks, gib = WGRAD[row]
    _need_memory(gib)
    torch.cuda.reset_peak_memory_stats()
    pad = k // 2
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    live = sorted(_live_samples(n, cin * h * w * 4) | _live_samples(n, cout * oh * ow * 4))
    gen = torch.Generator().manual_seed(600 + cin + stride)
    xl, dyl = _randn(gen, len(live), cin, h, w), _randn(gen, len(live), cout, oh, ow)          # mutually distinct data
    with _row():
        x = _randn(gen, P, cin, h, w).to(DEV).repeat(n // P, 1, 1, 1)          # a live dy paired with another sample's x gives another dw
        dy = torch.zeros([n, cout, oh, ow], device=DEV)
        idx = torch.tensor(live, device=DEV)
        x[idx], dy[idx] = xl.to(DEV), dyl.to(DEV)
        with _env(PG_WGRAD_BF16X3='1' if bf16x3 else '0'):
            assert M._bf16x3_wanted(n, cin, cout, h, w, k, k, stride) == bf16x3
            tl = M.start_wgrad_timeline()
            try:
                with poisoned_empty():
                    dw = M.weight_gradient(x, dy, [cout, cin, k, k], (pad, pad), stride=stride)
            finally:
                M.stop_wgrad_timeline()
        assert dw is not None and _last_label(tl)[3] == ('wgrad_bf16x3' if bf16x3 else 'wgrad'), _last_label(tl)
        want = torch.nn.grad.conv2d_weight(xl.double(), [cout, cin, k, k], dyl.double(), stride=stride, padding=pad)
        e = float((dw.double().cpu() - want).abs().max()) / float(want.abs().max())
        print(f'far wgrad {row}: {len(live)} live samples {live}, error {e:.2e} of the largest element, peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB')
        assert e <= (4e-6 if bf16x3 else 1e-5), e
        seen = {k_: v for k_, v in (('x', crossed(x)), ('dy', crossed(dy))) if v}
        assert seen == marks, f'the row states {marks}, the launch crossed {seen}'
        del x, dy, dw


@pytest.mark.gpu
def test_far_split3_planes(native):
    """pg_split3_bf16_cl on its own: x of 4200 MiB (past 2 and 4 GiB), its three channels-last bf16 planes [3, N, H, W, C] of 6300 MiB (past every mark; 24 GiB hold no
    x past 8 GiB beside them).  The planes repeat with the samples bit for bit, and on the base they re-add to x exactly and fall off by 2^-7 and 2^-15
    (test_weight_gradient_bf16x3 (a))."""
    from torch_utils.ops import _native as nat
    from torch_utils.ops import conv2d_mfma as M
    n, c, h, w = 4200, 64, 64, 64
    _need_memory(12)
    torch.cuda.reset_peak_memory_stats()
    gen = torch.Generator().manual_seed(85)
    xb = _randn(gen, P, c, h, w) * torch.exp(4 * _randn(gen, P, c, 1, 1))
    with _row():
        x = xb.to(DEV).repeat(n // P, 1, 1, 1)
        planes = torch.full([3, n, h, w, c], NAN, dtype=torch.bfloat16, device=DEV)
        nat.check(M._init().lib.pg_split3_bf16_cl(nat.ptr(x), nat.ptr(planes), n, c, h * w, nat.stream_of(x)), 'pg_split3_bf16_cl')
        assert crossed(x) == '31 32' and crossed(planes) == ALL
        count, first = periodic_mismatch(planes.permute(1, 0, 2, 3, 4))
        assert count == 0, f'{count} samples of the planes differ from sample n mod {P}, first {first}'
        back = planes[:, :P].float().permute(0, 1, 4, 2, 3).cpu()
        assert torch.equal((back[0] + back[1]) + back[2], xb)
        assert float(back[1].abs().max()) <= float(xb.abs().max()) * 2.0 ** -7 and float(back[2].abs().max()) <= float(xb.abs().max()) * 2.0 ** -15
        print(f'far split3: peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB')
        del x, planes


# ---------------------------------------------------------------------------------------------------------------- bias gradient: both layouts

@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['planar', 'interleaved'])
def test_far_bias_gradient(layout, native):
    """pg_bias_act_grad_bias over dy, yref and dx of 4200 MiB each (past 2 and 4 GiB; a third tensor of 8 GiB does not fit the 24 GiB of a row): dx periodic bit
    for bit and equal on the base to the float64 derivative of `oracle.ops_ref.bias_act` (3e-6, elements within 1e-6 of the clamp left out: either side is right
    there), db = N / P times the float64 sum of that derivative within 2e-6 of the sum of its magnitudes (both bars of
    test_bias_act_gradient_with_bias_gradient_in_one_pass)."""
    from oracle import ops_ref as R
    from torch_utils.ops import bias_act as B
    n, c, h, w = 4200, 16, 128, 128
    _need_memory(14)
    torch.cuda.reset_peak_memory_stats()
    gen = torch.Generator().manual_seed(81)
    xb, dyb = _randn(gen, P, c, h, w) * 2, _randn(gen, P, c, h, w)
    kw = dict(act='lrelu', alpha=0.2, gain=1.4, clamp=1.5)
    y64 = R.bias_act(xb.double(), None, **kw)
    want_dx = R.bias_act_grad(dyb.double(), xb.double(), None, **kw)[0]
    keep = ((R.bias_act(xb.double(), None, act='lrelu', alpha=0.2, gain=1.4).abs() - 1.5).abs() > 1e-6)          # (the value before the clamp)
    case = Case({}, [], None, None, layout='nhwc' if layout == 'interleaved' else 'nchw')
    with _row():
        y, dy = _repeat(y64.float(), case, n), _repeat(dyb, case, n)          # yref = the forward's output, as BiasActCuda.backward hands it over
        with poisoned_empty():
            out = B._native_grad_bias(dy, y, 1, 'lrelu', 0.2, 1.4, 1.5)
        assert out is not None, 'the layout is expected to be covered'
        dx, db = out
        assert dx.stride() == dy.stride() and crossed(dx) == crossed(dy) == crossed(y) == '31 32'
        count, first = periodic_mismatch(dx)
        assert count == 0, f'dx: {count} samples differ from sample n mod {P}, first {first}'
        got = dx[:P].double().cpu()
        np.testing.assert_allclose(got[keep].numpy(), want_dx[keep].numpy(), rtol=3e-6, atol=3e-6)
        want = want_dx.sum([0, 2, 3]) * (n // P)
        scale = float(want_dx.abs().sum([0, 2, 3]).max()) * (n // P)
        e = float((db.double().cpu() - want).abs().max())
        print(f'far bias gradient ({layout}): {int((~keep).sum())} elements at the clamp left out, db off by {e / scale:.2e} of the sum of |dx|, peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB')
        assert e <= 2e-6 * scale
        del y, dy, dx, out


# ---------------------------------------------------------------------------------------------------------------- past the guard, end to end

@pytest.mark.gpu
def test_conv2d_past_the_element_guard_takes_the_fallback(native):
    """conv2d_gradfix.conv2d on a y past 2^31 elements: pg_conv2d_forward declines (PG_ERR_TOO_LARGE), the caller's fallback runs, and EVERY sample of the result
    meets the float64 reference of its phase at the direct kernel's bar (the cheapest geometry: 1x1, 16 -> 16 at 64 x 64, N = 32802: 8.0 GiB each way).  The fallback is
    aten's convolution in batch chunks (`conv2d_gradfix._aten_batched`): one aten call on this y returns the samples from 32768 on -- element 2^31 on -- as copies
    of the first ones, which the odd period makes visible."""
    from torch_utils.ops import _native as nat
    from torch_utils.ops import conv2d_gradfix as G
    from torch_utils.ops import conv2d_mfma as M
    n, c, h, w = 32802, 16, 64, 64
    _need_memory(22)
    gen = torch.Generator().manual_seed(82)
    xb, wt = _randn(gen, P, c, h, w), _weights(gen, [c, c, 1, 1], c)
    with _row():
        x = xb.to(DEV).repeat(n // P, 1, 1, 1)
        with pytest.raises(nat.NativeNotCovered):          # PG_ERR_TOO_LARGE, before any launch
            M.conv2d_forward(x, M.pack_weight(wt.to(DEV)), c, 1, 1)
        _release()
        with torch.no_grad():
            y = G.conv2d(x, wt.to(DEV))
        assert crossed(y) == ALL and crossed(x) == ALL
        # aten picks its algorithm by batch size and the last chunk is shorter, so bits may differ between samples of one call (conv2d_gradfix._aten_batched):
        # every sample is compared with the float64 reference of its phase at the direct kernel's bar instead (test_conv2d_vs_oracle)
        ref = F.conv2d(xb.double(), wt.double())
        ref_d, tol = ref.to(DEV), 2e-5 * scale_of(ref)
        worst = 0.0
        for i in range(0, n, 3 * 1024):
            seg = y[i:i + 3 * 1024].double()
            seg = seg.unflatten(0, (seg.shape[0] // P, P))
            excess = float(((seg - ref_d).abs() - 1e-4 * ref_d.abs()).max())
            worst = max(worst, excess)
        print(f'far fallback: worst |y - ref| - 1e-4 |ref| over all {n} samples {worst:.3e} (bar {tol:.3e})')
        assert worst <= tol
        del x, y


# ---------------------------------------------------------------------------------------------------------------- guard boundaries (host only: no GPU memory, no launch)

PG_ERR_TOO_LARGE, PG_ERR_UNSUPPORTED = -3, -2
_V, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_P4 = ctypes.POINTER(ctypes.c_int64)


def _lib(name):
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    return ctypes.CDLL(custom_ops.get_plugin(name, build_only=True))


def _call(lib, name, argtypes, *args):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = ctypes.c_int, argtypes
    return fn(*args)


def _strides(n_stride, c, h, w, pitch=None):
    pitch = pitch or w
    return (ctypes.c_int64 * 4)(n_stride if n_stride else c * h * pitch, h * pitch, pitch, 1)


def test_size_guards_refuse_the_first_size_past_them():
    """Every size guard of the far rows' entries, called with non-null dummy pointers (64: 16-byte aligned, never dereferenced on these paths) at the first size it
    refuses: PG_ERR_TOO_LARGE, before any launch.  Where a later host check declines an ACCEPTED size without launching (a 5x5 kernel, pad_x = 2 for F(4x4)), the
    last size the guard admits is shown to pass it: the answer is then PG_ERR_UNSUPPORTED, not PG_ERR_TOO_LARGE."""
    conv, fir = _lib('conv2d_plugin'), _lib('upfirdn2d_plugin')
    d = _V(64)
    fwd = [_V] * 3 + [_I] * 12 + [_P4] + [_I] * 4 + [_V] * 2

    def forward(n, cin, h, w, cout, k, ystr=None, oh=None, ow=None):
        oh, ow = oh or h, ow or w
        return _call(conv, 'pg_conv2d_forward', fwd, d, d, d, n, cin, h, w, cout, k, k, 1, k // 2, k // 2, oh, ow, ystr or _strides(0, cout, oh, ow), 1, 1, 0, 0, None, None)
    # conv2d.hip: one image of x <= 2^31 - 1 bytes (Cin * H * W * 4, and 16 * H * W * 4 for the padded chunk)
    assert forward(1, 64, 4096, 2048, 8, 3) == PG_ERR_TOO_LARGE              # 2^31 bytes
    assert forward(1, 64, 4096, 2047, 8, 5) == PG_ERR_UNSUPPORTED            # 2^31 - 2^20: passes the guards, a 5x5 kernel is declined without a launch
    assert forward(1, 3, 32768, 4096, 2, 3) == PG_ERR_TOO_LARGE              # 16 * H * W * 4 = 2^33 with only three channels
    # y extent <= 2^31 - 1 elements, dense and through ystride[0] alone; N * OH * OW <= 2^31 - 1
    assert forward(8192, 16, 64, 64, 64, 3) == PG_ERR_TOO_LARGE              # 2^31 elements (the far rows run N = 8190)
    assert forward(8191, 16, 64, 64, 64, 5) == PG_ERR_UNSUPPORTED
    assert forward(8193, 16, 64, 64, 32, 3, ystr=_strides(64 * 4096, 32, 64, 64)) == PG_ERR_TOO_LARGE          # the channel slice of the strided rows: sample 8192 starts at element 2^31
    assert forward(8192, 16, 64, 64, 32, 5, ystr=_strides(64 * 4096, 32, 64, 64)) == PG_ERR_UNSUPPORTED
    assert forward(65536, 2, 256, 128, 1, 3) == PG_ERR_TOO_LARGE             # N * OH * OW = 2^31: the per-sample noise plane's 32-bit index
    assert forward(65535, 2, 256, 128, 1, 5) == PG_ERR_UNSUPPORTED

    wino = [_I] + [_V] * 3 + [_I] * 9 + [_P4] + [_V] * 2

    def winograd(form, n, cin, h, w, cout, pad_x=1):
        return _call(conv, 'pg_conv2d_winograd_forward', wino, form, d, d, d, n, cin, h, w, cout, 1, pad_x, h, w + 2 * pad_x - 2, _strides(0, cout, h, w + 2 * pad_x - 2), None, None)
    for form in (1, 2, 3, 4):          # F(2x2), F(4x4), F(4x4) two-workgroup, F(4x4) bf16x3: one image of y <= 2^32 - 1 bytes
        assert winograd(form, 1, 16, 4096, 4096, 64) == PG_ERR_TOO_LARGE, form          # 2^32 bytes: also inside conv_forward's own 2^31 - 1 elements
    for form in (2, 3, 4):
        assert winograd(form, 1, 16, 4096, 4092, 64, pad_x=2) == PG_ERR_UNSUPPORTED, form          # passes the size guards; pad_x = 2 is declined without a launch

    up2 = [_V] * 3 + [_I] * 5 + [_P4] + [_V] * 3
    assert _call(conv, 'pg_conv2d_up2_forward', up2, d, d, d, 1, 64, 4096, 2048, 8, _strides(0, 8, 8193, 4097, 4100), None, None, None) == PG_ERR_TOO_LARGE      # conv2d_inst_up2.hip: one image of x

    wg = [_V] * 4 + [_I] * 13 + [_V]
    # conv2d_wgrad.hip offsets_fit: (64 planes + 4096) * 4 bytes below 2^31 -- a plane of 2^23 - 64 pixels is the first refused
    assert _call(conv, 'pg_conv2d_wgrad', wg, d, d, d, d, 1, 16, 4096, 2048, 16, 3, 3, 1, 1, 1, 4096, 2048, 1, None) == PG_ERR_TOO_LARGE
    assert _call(conv, 'pg_conv2d_wgrad', wg, d, d, d, d, 1, 16, 8388544 // 64, 64, 16, 3, 3, 1, 1, 1, 8388544 // 64, 64, 1, None) == PG_ERR_TOO_LARGE
    # the bf16x3 route: one channels-last image of x or dy below 0x7fff0000 bytes
    assert _call(conv, 'pg_conv2d16_wgrad_x3', wg, d, d, d, d, 1, 64, 4096, 4096, 64, 3, 3, 1, 1, 1, 4096, 4096, 1, None) == PG_ERR_TOO_LARGE

    c16 = [_V] * 3 + [_I] * 14 + [_L] + [_P4] + [_I] * 4 + [_V] * 2
    cl = lambda n_, c_, h_, w_: (ctypes.c_int64 * 4)(h_ * w_ * c_, 1, w_ * c_, c_)          # channels-last strides

    def forward16(n, cin, h, w, cout):
        return _call(conv, 'pg_conv2d16_forward', c16, d, d, d, 2, 2, n, cin, h, w, cout, 3, 3, 1, 1, 1, h, w, 0, cl(n, cout, h, w), 1, 1, 0, 0, None, None)
    assert forward16(1, 64, 4096, 4096, 64) == PG_ERR_TOO_LARGE              # conv2d16.hip: one image of x, 2^31 bytes
    assert forward16(8192, 32, 64, 64, 32) == PG_ERR_TOO_LARGE               # y: 2^30 elements (the far rows run N = 8190)
    assert forward16(8192, 32, 64, 64, 16) == PG_ERR_TOO_LARGE               # conv2d_kernel16.h: the whole x behind one descriptor, 2^31 bytes
    up2f = [_V] * 3 + [_I] * 6 + [_L] + [_P4] + [ctypes.POINTER(_F)] + [_V] * 2
    fx = (_F * 4)(1, 3, 3, 1)
    assert _call(conv, 'pg_conv2d16_up2_fused', up2f, d, d, d, 2, 32768, 32, 32, 32, 32, 0, cl(1, 32, 64, 64), fx, None, None) == PG_ERR_TOO_LARGE      # whole x: 2^31 bytes
    assert _call(conv, 'pg_conv2d16_up2_fused', up2f, d, d, d, 2, 17477, 32, 16, 30, 32, 0, cl(1, 32, 32, 60), fx, None, None) == PG_ERR_TOO_LARGE      # y: y: 2^30 elements and more (the far row runs N = 17475)

    # N <= 65535 (gridDim.y / gridDim.z) of the heads, the folds and the 16-bit statistics
    assert _call(conv, 'pg_conv1x1_small', [_V] * 6 + [_I, _I, _L, _I, _F, _F, _V], d, d, None, None, None, d, 65536, 16, 64, 3, 1.0, -1.0, None) == PG_ERR_TOO_LARGE
    assert _call(conv, 'pg_conv1x1_fold_heads', [_V] * 7 + [_I, _I, _I, _L, _I, _I, _I, _F, _V], d, d, d, d, None, d, d, 65536, 8, 8, 64, 6, 3, 0, -1.0, None) == PG_ERR_TOO_LARGE
    assert _call(conv, 'pg_conv3x3_fold_head', [_V] * 6 + [_I] * 5 + [_F, _V], d, d, d, d, None, d, 65536, 8, 8, 8, 3, -1.0, None) == PG_ERR_TOO_LARGE
    assert _call(conv, 'pg_conv3x3_cin1', [_V] * 3 + [_I] * 4 + [_F, _I, _V], d, d, d, 65536, 8, 8, 4, 1.0, 1, None) == PG_ERR_TOO_LARGE
    assert _call(conv, 'pg_instance_norm_stats_cl16', [_V] * 4 + [_I, _I, _L, _I, _F, _V], d, d, d, d, 2, 65536, 64, 16, 1e-5, None) == PG_ERR_UNSUPPORTED      # (this one answers UNSUPPORTED: spade16.hip:169)
    assert _call(conv, 'pg_spade_combine_cl16', [_V] * 5 + [_I, _I, _L, _I, _I, _F, _F, _F, _V], d, d, d, d, d, 2, 65535, 1 << 16, 8 * 16, 1, 0.0, 1.0, -1.0, None) == PG_ERR_TOO_LARGE      # N * HW * C / 8 = 2^36

    assert _call(conv, 'pg_split3_bf16_cl', [_V, _V, _I, _I, _L, _V], d, d, 65536, 64, 64, None) == PG_ERR_TOO_LARGE               # conv2d_wgrad.hip: gridDim.z
    assert _call(conv, 'pg_split3_bf16_cl', [_V, _V, _I, _I, _L, _V], d, d, 1, 64, 1 << 31, None) == PG_ERR_TOO_LARGE              # ... and HW past 2^31 - 1
    # (spade16.hip's N * C <= 2^31 - 1 behind the check above cannot be reached: N <= 65535 and C <= 8 * 256 come first, their product stays below 2^27)
    # vgg_loss.hip: planes * h * w and groups * m must stay below 2^63 / 4 and 2^63 / 8 -- no tensor reaches them, the calls show the arithmetic does not wrap
    vgg = _lib('vgg_loss_plugin')
    assert _call(vgg, 'pg_maxpool2x2', [_V, _V, _L, _I, _I, _V], d, d, 1 << 62, 2, 2, None) == PG_ERR_TOO_LARGE
    assert _call(vgg, 'pg_maxpool2x2_backward', [_V, _V, _V, _L, _I, _I, _V], d, d, d, 1 << 62, 2, 2, None) == PG_ERR_TOO_LARGE
    assert _call(vgg, 'pg_l1_pair_sum', [_V, _V, _V, _V, _I, _L, ctypes.c_double, _V], d, d, d, d, 2, 1 << 61, 1.0, None) == PG_ERR_TOO_LARGE
    assert _call(vgg, 'pg_l1_pair_grad', [_V, _V, _V, _V, _I, _L, ctypes.c_double, _V], d, d, d, d, 2, 1 << 61, 1.0, None) == PG_ERR_TOO_LARGE

    # upfirdn2d.hip: 32-bit coordinates along one axis (the reference's INT_MAX limits)
    s4, s2 = (ctypes.c_int64 * 4)(1, 1, 1, 1), (ctypes.c_int64 * 2)(4, 1)
    firt = [_V] * 3 + [_I] * 5 + [_P4] + [_I, _I, ctypes.POINTER(ctypes.c_int64)] + [_I, _I, _P4] + [_I] * 7 + [_F, _V]
    assert _call(fir, 'pg_upfirdn2d', firt, d, d, d, 0, 1, 1, 4, 1 << 30, s4, 4, 4, s2, 8, 1 << 30, s4, 2, 2, 1, 1, 2, 2, 0, 1.0, None) == PG_ERR_TOO_LARGE       # inW * up = 2^31


def test_flat_adam_refuses_a_buffer_past_32_bit_offsets():
    """adam_flat_kernel indexes the flat buffer with `int` offsets: FlatAdam asserts the bound instead of relying on the model's size."""
    from training import flat_adam
    assert flat_adam.MAX_FLAT_ELEMENTS == (1 << 31) - 1
    with pytest.raises(AssertionError):
        flat_adam.check_flat_size(1 << 31)
    flat_adam.check_flat_size((1 << 31) - 1)
