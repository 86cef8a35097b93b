"""conv2d / conv_transpose2d entry points of the synthesis path on MI355X.

API of the reference's ``torch_utils/ops/conv2d_gradfix.py``: ``conv2d`` (:35-38),
``conv_transpose2d`` (:40-43), ``no_weight_gradients()`` (:25-31) and the module globals
``enabled`` / ``weight_gradients_disabled`` (:22-23).  In the reference this is where all
conv arithmetic is handed to cuDNN; here float32 NCHW convolutions of the geometries the
generator uses run the hand-written MFMA implicit-GEMM kernel (``conv2d_mfma`` ->
``csrc/conv2d_kernel.h``).  A stride-2 transposed conv is issued as one gather-form
sub-convolution per output phase, so no multiply is spent on stuffed zeros.

Gradients: the INPUT gradient of a convolution is again a convolution (with the O<->I transposed, spatially
flipped weight; a strided conv's is a transposed conv and vice versa), so it runs the same MFMA kernel through
this same autograd Function -- which makes arbitrary-order input gradients (R1, loss_fullbody.py:262-274) native
too, exactly how the reference's ``_conv2d_gradfix`` recurses (conv2d_gradfix.py:118-135).  The WEIGHT gradient
(a reduction over pixels, a different GEMM shape: csrc/conv2d_wgrad.hip) is native for the float32 3x3 (stride 1, 2, transposed)
and 1x1 layers; other geometries and 16-bit layers take ``aten::convolution_backward``; both honour ``no_weight_gradients``.  bf16 / fp16 tensors (the discriminator's fp16 blocks, networks.py:444-523; the half-precision
synthesis stack) run the 16-bit MFMA kernel (``conv2d_mfma16`` -> ``csrc/conv2d_kernel16.h``) on channels-last storage,
input gradients included.  Configurations the kernels do not cover (groups > 1, dilation, exotic kernel sizes) go to
PyTorch-ROCm's convolution on the GPU, as does everything when ``enabled`` is set to False.  CPU tensors take the
pure-torch route of ``impl='ref'`` semantics (torch.nn.functional), like the reference's own fallback (:53-56).
"""

import contextlib
import os

import weakref

import torch

from . import _native as nat
from . import bias_act
from . import conv2d_mfma
from . import conv2d_mfma16

native_input_gradients = os.environ.get('PG_NATIVE_DGRAD', '1') == '1'    # input gradients through the MFMA / Winograd kernels (PG_NATIVE_DGRAD=0: aten)
native_weight_gradients16 = os.environ.get('PG_NATIVE_WGRAD16', '1') == '1'   # weight gradients of the 16-bit 3x3 / 1x1 convs through conv2d16_wgrad (PG_NATIVE_WGRAD16=0: aten / MIOpen)
native_weight_gradients = os.environ.get('PG_NATIVE_WGRAD', '1') == '1'   # weight gradients of stride-1 3x3 / 1x1 fp32 convs through csrc/conv2d_wgrad.hip (exact, deterministic; PG_NATIVE_WGRAD=0: aten / MIOpen)
enabled = True                      # True (default here; the reference's loop sets it, training_loop_fullbody.py:386): hand-written kernels.  False: aten
weight_gradients_disabled = False   # forcefully disable weight gradients (R1, loss_fullbody.py:266)


@contextlib.contextmanager
def no_weight_gradients():
    global weight_gradients_disabled
    old = weight_gradients_disabled
    weight_gradients_disabled = True
    try:
        yield
    finally:
        weight_gradients_disabled = old


def _pair(v):
    if isinstance(v, (tuple, list)):
        assert len(v) == 2
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _native_ok(x, w, stride, dilation, groups):
    return (x.dtype == torch.float32 and w.dtype == torch.float32 and x.ndim == 4 and groups == 1
            and dilation == (1, 1) and stride[0] == stride[1]
            and x.numel() > 0 and w.numel() > 0)       # empty batches / channel sets: nothing to launch, aten returns the empty result


def _native16_ok(x, w, stride, dilation, groups):
    # (round 5: a float32 weight with 16-bit activations is welcome -- the pack converts it, the weight gradient leaves the kernel in float32: the caller's
    # `w.to(x.dtype)`, this route's `.float()` and the two casts of its backward were four elementwise launches per layer call)
    return (x.dtype in conv2d_mfma16.DTYPES and w.dtype in (x.dtype, torch.float32) and x.ndim == 4 and groups == 1 and dilation == (1, 1)
            and stride[0] == stride[1] and x.numel() > 0 and w.numel() > 0)


def _by_group(fn, input, weight, bias, groups, out_axis, **kw):
    """A grouped convolution as `groups` ordinary ones on channel slices (the reference's fused modulated convolution:
    batch folded into the channel axis with groups = N, networks.py:85-94 / conv2d_resample.py:127-131) -- each slice runs on
    the MFMA kernels and is differentiable like any other call."""
    cin_g = input.shape[1] // groups
    w_g = weight.shape[0] // groups
    outs = []
    for g in range(groups):
        wg = weight[g * w_g:(g + 1) * w_g]
        ng = wg.shape[out_axis]
        bg = bias[g * ng:(g + 1) * ng] if bias is not None else None
        outs.append(fn(input[:, g * cin_g:(g + 1) * cin_g], wg, bg, groups=1, **kw))
    return torch.cat(outs, dim=1)


fused_epilogue = os.environ.get('PG_TRAIN_EPILOGUE', '1') != '0'     # training route: bias_act in the convolution's epilogue (PG_TRAIN_EPILOGUE=0: a pass of its own)


def _epilogue_cfg(ep):
    """dict(act, alpha, gain, clamp) of a `bias_act` that follows the convolution -> the tuple the autograd Functions carry, or None when
    it is the identity."""
    if not ep:
        return None
    act = ep.get('act', 'linear')
    spec = bias_act.activation_funcs[act]
    alpha = float(ep['alpha'] if ep.get('alpha') is not None else spec.def_alpha)
    gain = float(ep['gain'] if ep.get('gain') is not None else spec.def_gain)
    clamp = float(ep['clamp'] if ep.get('clamp') is not None else -1)
    if act == 'linear' and gain == 1 and clamp < 0:
        return None
    return (act, alpha, gain, clamp)


ATEN_MAX_ELEMENTS = 1 << 30      # per aten call: input and output of one call stay below 2^31 elements with a factor of two to spare


def _aten_batched(fn, input, grow=1, **kw):
    """`fn(input, **kw)` (an aten convolution) in batch chunks whose input and output stay below ATEN_MAX_ELEMENTS.  aten's GPU convolution indexes a
    batch with 32 bits: on an output past 2^31 elements the samples behind that index came back as copies of the first ones (measured: 16 -> 16 channels,
    1x1, 64 x 64, N = 32802 -- sample 32768 onward), silently.  This is the route a launch takes that the native kernels decline as PG_ERR_TOO_LARGE, so it must
    hold exactly there.  Small tensors take one call, as before (`grow`: output pixels per input pixel, for the estimate that decides it)."""
    n = int(input.shape[0]) if input.ndim == 4 else 1
    wide = max(int(d) for d in kw['weight'].shape[:2]) * int(kw.get('groups', 1))          # no fewer than the channels of either side
    if not input.is_cuda or n <= 1 or input.numel() // max(1, int(input.shape[1])) * wide * grow <= ATEN_MAX_ELEMENTS // 2:
        return fn(input=input, **kw)
    with torch.no_grad():
        one = fn(input=input[:1].detach(), **{k: (v.detach() if torch.is_tensor(v) else v) for k, v in kw.items()})          # (for the output's shape)
    step = max(1, ATEN_MAX_ELEMENTS // max(input[0].numel(), one[0].numel()))
    if step >= n:
        return fn(input=input, **kw)
    if torch.is_grad_enabled() and (input.requires_grad or any(torch.is_tensor(v) and v.requires_grad for v in kw.values())):
        return torch.cat([fn(input=input[i:i + step], **kw) for i in range(0, n, step)])
    out = torch.empty([n, *one.shape[1:]], dtype=one.dtype, device=one.device)
    for i in range(0, n, step):
        out[i:i + step] = fn(input=input[i:i + step], **kw)
    return out


def conv2d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, _epilogue=None):
    """`_epilogue` (private): dict(act, alpha, gain, clamp) -- `bias_act(conv2d(...) , act=...)` of the caller (the bias is this call's
    `bias`), run in the native convolution's epilogue with the derivative taken from the saved output, or as the separate op where the
    native kernels do not take the call."""
    assert isinstance(input, torch.Tensor)
    cfg = _epilogue_cfg(_epilogue)

    def tail(y):
        return y if cfg is None else bias_act.bias_act(y, None, act=cfg[0], alpha=cfg[1], gain=cfg[2], clamp=cfg[3] if cfg[3] >= 0 else None)
    if enabled and input.is_cuda and 1 < groups <= 64 and input.ndim == 4 and input.shape[1] % groups == 0 and weight.shape[0] % groups == 0:
        return tail(_by_group(conv2d, input, weight, bias, groups, 0, stride=stride, padding=padding, dilation=dilation))
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    kh, kw = int(weight.shape[2]), int(weight.shape[3])
    fuse = cfg if (fused_epilogue and cfg is not None and cfg[0] in conv2d_mfma.FUSED_ACTS) else None
    if enabled and input.is_cuda and min(padding) >= 0:
        try:                                           # a VALID request the kernels decline (32-bit indexing limits, LDS budget) takes the aten route
            if _native_ok(input, weight, stride, dilation, groups) and conv2d_mfma.supported(kh, kw, stride[0]):
                y = _Conv2dMfma.apply(input, weight, bias, stride[0], padding, False, (0, 0), fuse)
                return y if fuse is not None else tail(y)
            if _native16_ok(input, weight, stride, dilation, groups) and conv2d_mfma16.supported(kh, kw, stride[0]):
                y = _Conv2dMfma16.apply(input, weight, bias, stride[0], padding, False, (0, 0), fuse)
                return y if fuse is not None else tail(y)
        except nat.NativeNotCovered:
            pass
    if weight.dtype != input.dtype:
        weight = weight.to(input.dtype)
    return tail(_aten_batched(torch.nn.functional.conv2d, input, weight=weight, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=groups))


def _phases_supported(mod, kh, kw, s):
    return s > 1 and kh >= s and kw >= s and all(mod.supported(jy, jx, 1) for jy in {-(-(kh - a) // s) for a in range(s)}
                                                 for jx in {-(-(kw - a) // s) for a in range(s)})


def conv_transpose2d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
    assert isinstance(input, torch.Tensor)
    if enabled and input.is_cuda and 1 < groups <= 64 and input.ndim == 4 and input.shape[1] % groups == 0 and weight.shape[0] % groups == 0:
        return _by_group(conv_transpose2d, input, weight, bias, groups, 1, stride=stride, padding=padding, output_padding=output_padding, dilation=dilation)
    stride, padding, dilation, output_padding = _pair(stride), _pair(padding), _pair(dilation), _pair(output_padding)
    kh, kw = int(weight.shape[2]), int(weight.shape[3])
    if enabled and input.is_cuda:
        try:
            if _native_ok(input, weight, stride, dilation, groups) and _phases_supported(conv2d_mfma, kh, kw, stride[0]):
                return _Conv2dMfma.apply(input, weight, bias, stride[0], padding, True, output_padding)
            if _native16_ok(input, weight, stride, dilation, groups) and _phases_supported(conv2d_mfma16, kh, kw, stride[0]):
                return _Conv2dMfma16.apply(input, weight, bias, stride[0], padding, True, output_padding)
        except nat.NativeNotCovered:
            pass
    if weight.dtype != input.dtype:
        weight = weight.to(input.dtype)
    return _aten_batched(torch.nn.functional.conv_transpose2d, input, grow=2 * max(_pair(stride)) ** 2, weight=weight, bias=bias, stride=stride, padding=padding,
                         output_padding=output_padding, groups=groups, dilation=dilation)


UP2_TRANSPOSED = os.environ.get('PG_UP2_TRANSPOSED', '1') != '0'      # A/B: 0 = the transposed 3x3 stride-2 convolution as four phase launches

UP2_TRANSPOSED_X3 = os.environ.get('PG_UP2_TRANSPOSED_X3', '1') != '0'

_pack_cache = {}      # (storage ptr, version, shape, strides, winograd, flip, transpose) -> (weakref to the source, packed weights)
_PACK_CACHE_MAX_BYTES = 1 << 30


def _packed(weight, winograd, flip=False, transpose_oi=False):
    """Packed form of `weight` for the MFMA kernels, cached for as long as the SOURCE TENSOR OBJECT lives and keeps its version:
    a parameter passed directly hits across steps until the optimizer writes it; the equalised-LR temporaries of the training
    route (``self.weight * self.weight_gain``) hit for the forward, the input gradient and every accumulation round /
    double-backward pass of the graph that holds them, and their entries are dropped the moment autograd releases the
    temporary (weakref callback) -- nothing packed outlives its source.  A byte cap bounds the live set."""
    base = weight._base if weight._base is not None else weight
    key = (weight.data_ptr(), base._version, tuple(weight.shape), tuple(weight.stride()), int(winograd), bool(flip), bool(transpose_oi), nat.cache_epoch[0])
    entry = _pack_cache.get(key)
    hit = entry[1] if entry is not None and entry[0]() is base else None      # same address + version is not identity: a freed
    if hit is None:                                                           # tensor's block is handed to the next one of its size
        w = weight.detach()
        if not w.is_contiguous():
            w = w.contiguous()
        hit = conv2d_mfma.pack_weight(w, flip=flip, transpose_oi=transpose_oi, winograd=winograd)
        if sum(e[1].numel() * e[1].element_size() for e in _pack_cache.values()) + hit.numel() * hit.element_size() > _PACK_CACHE_MAX_BYTES:
            _pack_cache.clear()

        def _evict(ref, key=key):
            e = _pack_cache.get(key)
            if e is not None and e[0] is ref:
                del _pack_cache[key]
        _pack_cache[key] = (weakref.ref(base, _evict), hit)
    return hit


def _epilogue_backward(ctx, dy, y, ep, want_b):
    """dy of the fused bias_act -> dy of the convolution proper (and db from the same pass): `_BiasActGrad` on the saved output, the
    op `BiasActCuda.backward` runs (bias_act.py:160-176) -- differentiable again, so R1-style double backward passes through."""
    act, alpha, gain, clamp = ep
    if want_b:
        return bias_act._BiasActGrad.apply(dy, None, None, y, 1, act, alpha, gain, clamp, True)
    return bias_act._BiasActGrad.apply(dy, None, None, y, 1, act, alpha, gain, clamp), None


class _Conv2dMfma(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, transposed, output_padding, ep=None):
        x = x.contiguous()
        n, cin, h, w = x.shape
        kh, kw = int(weight.shape[2]), int(weight.shape[3])
        if not transposed:
            cout = int(weight.shape[0])
            fz = dict(act=ep[0], alpha=ep[1], gain=ep[2], clamp=ep[3] if ep[3] >= 0 else None) if ep is not None else {}
            wg = conv2d_mfma.use_winograd(kh, kw, stride, cout, cin, pad=padding, hw=(h, w), ep=fz)
            # (s2x3=False: the training route keeps the fp32 kernel for its stride-2 layers -- grad mode is off in here, which is what the inference route's gate reads)
            y = conv2d_mfma.conv2d_forward(x, _packed(weight, wg), cout, kh, kw, stride=stride, pad=padding, bias=bias, winograd=wg, s2x3=False, **fz)
        else:
            assert ep is None
            cout = int(weight.shape[1])
            out_hw = ((h - 1) * stride - 2 * padding[0] + kh + output_padding[0], (w - 1) * stride - 2 * padding[1] + kw + output_padding[1])
            if ((kh, kw, stride) == (3, 3, 2) and tuple(padding) == (0, 0) and tuple(output_padding) == (0, 0) and bias is None and UP2_TRANSPOSED
                    and (n * cout * out_hw[0] * ((out_hw[1] + 3) // 4 * 4)) * 4 < 2 ** 31):
                # the stride-2 transposed 3x3 convolution without padding -- the input gradient of every `down = 2` 3x3 layer (FIR, then a strided convolution with
                # padding 0) -- as ONE launch of the four-parity kernel of the up = 2 layers (csrc/conv2d_up2.h, fp32 MFMA) instead of four gather-form phase
                # launches with a weight pack each (late round 6).  The IOHW weight packs as the kernel's OIHW operand without a copy (transpose_oi).
                main = _packed(weight, 0, flip=False, transpose_oi=True)
                packs = dict(main=main)
                if UP2_TRANSPOSED_X3 and cin % 16 == 0 and cin >= 32:
                    # ... with its main tiles on the bf16 pipe (csrc/conv2d_up2x3.h, float32-class): the split planes of the same pack, kept while the pack lives
                    packs['x3'] = conv2d_mfma.pack_x3('up2', main, cout, cin)
                y = conv2d_mfma.conv_up2_forward(x, packs, cout, x3=None if 'x3' in packs else False)
            else:
                phases = conv2d_mfma.pack_transposed(weight, stride, padding, (h, w), out_hw)
                y = conv2d_mfma.conv_transpose2d_forward(x, phases, cout, out_hw, stride=stride, bias=bias)
        ctx.save_for_backward(x, weight, y if ep is not None else None)
        ctx.cfg = (stride, padding, transposed, output_padding, bias is not None, ep)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        stride, padding, transposed, output_padding, has_bias, ep = ctx.cfg
        kh, kw = int(weight.shape[2]), int(weight.shape[3])
        dx = dw = db = None
        if ep is not None:
            dy, db = _epilogue_backward(ctx, dy, y, ep, has_bias and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[0] and native_input_gradients:
            dx = _input_gradient(dy, x.shape, weight, stride, padding, transposed, output_padding)
        want_w = ctx.needs_input_grad[1] and not weight_gradients_disabled
        want_b = has_bias and ctx.needs_input_grad[2]
        if want_w and native_weight_gradients and stride in (1, 2):
            if torch.is_grad_enabled() and (dy.requires_grad or x.requires_grad):
                # create_graph with dy / x carrying a graph: the weight gradient must itself be differentiable
                try:
                    dw = _WeightGradient.apply(dy, x, tuple(weight.shape), stride, padding, transposed, output_padding)
                except nat.NativeNotCovered:
                    dw = None
            else:
                dw = _weight_gradient(dy, x, weight.shape, stride, padding, transposed)
        if want_b and db is None and (dw is not None or not want_w):
            db = bias_act.channel_sum(dy, 1)                 # one deterministic native pass (csrc/bias_act.hip)
        mask = [dx is None and ctx.needs_input_grad[0], want_w and dw is None, want_b and db is None]
        if any(mask):
            gx, gw, gb = torch.ops.aten.convolution_backward(
                dy, x, weight, [weight.shape[1 if transposed else 0]] if has_bias else None,
                [stride, stride], list(padding), [1, 1], transposed, list(output_padding), 1, mask)
            dx = gx if mask[0] else dx
            dw = gw if mask[1] else dw
            db = gb if mask[2] else db
        return dx, dw, db, None, None, None, None, None


def _weight_gradient(dy, x, weight_shape, stride, padding, transposed):
    """Native fp32 weight gradient (a GEMM over pixels, csrc/conv2d_wgrad.hip); None = geometry not covered."""
    if not transposed:
        return conv2d_mfma.weight_gradient(x, dy, weight_shape, padding, stride=stride)
    # y = conv_transpose2d(x, w[Cin, Cout]):  dw[ci, co, ky, kx] = sum x[ci, iy, ix] dy[co, s iy + ky - p, s ix + kx - p] -- the weight
    # gradient of the strided convolution dy -> x, whose 'OIHW' kernel has O = Cin, I = Cout: the same kernel with the roles swapped
    return conv2d_mfma.weight_gradient(dy, x, weight_shape, padding, stride=stride)


class _WeightGradient(torch.autograd.Function):
    """The weight gradient as a differentiable op (the role of the reference's Conv2dGradWeight, conv2d_gradfix.py:139-168): dw is bilinear
    in (dy, x), so for an incoming gradient g of the weight's shape  d/d(dy) = the forward convolution of x with g in the weight's place and
    d/dx = the input-gradient form of dy with g -- both native again, to any order."""

    @staticmethod
    def forward(ctx, dy, x, weight_shape, stride, padding, transposed, output_padding):
        dw = _weight_gradient(dy.contiguous(), x.contiguous(), weight_shape, stride, padding, transposed)
        if dw is None:
            raise nat.NativeNotCovered('conv2d_gradfix: weight gradient geometry not covered')
        ctx.save_for_backward(dy, x)
        ctx.cfg = (stride, padding, transposed, output_padding)
        return dw

    @staticmethod
    def backward(ctx, g):
        dy, x = ctx.saved_tensors
        stride, padding, transposed, output_padding = ctx.cfg
        d_dy = d_x = None
        if ctx.needs_input_grad[0]:
            d_dy = _Conv2dMfma.apply(x, g, None, stride, padding, transposed, output_padding)
        if ctx.needs_input_grad[1]:
            d_x = _input_gradient(dy, x.shape, g, stride, padding, transposed, output_padding)
            if d_x is None:
                d_x = torch.ops.aten.convolution_backward(dy, x, g, None, [stride, stride], list(padding), [1, 1], transposed, list(output_padding), 1, [True, False, False])[0]
        return d_dy, d_x, None, None, None, None, None


class _Conv2dMfma16(torch.autograd.Function):
    """bf16 / fp16 convolution on the 16-bit MFMA kernel.  Channels are zero-padded to a multiple of 16 (the K of one
    MFMA) when needed -- the fromrgb layers: 6 / 10 image channels.  Output: channels-last storage, x's dtype."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, transposed, output_padding, ep=None):
        n, cin, h, w = x.shape
        kh, kw = int(weight.shape[2]), int(weight.shape[3])
        xp, wf = x, weight.detach().float()
        if cin % 16 != 0:
            padc = 16 - cin % 16
            xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, padc))
            wf = torch.nn.functional.pad(wf, (0, 0, 0, 0, 0, 0, 0, padc) if transposed else (0, 0, 0, 0, 0, padc))
        b32 = bias.detach().float() if bias is not None else None
        if not transposed:
            cout = int(weight.shape[0])
            packed, _, _ = conv2d_mfma16.pack_weight(wf, x.dtype)
            fz = dict(act=ep[0], alpha=ep[1], gain=ep[2], clamp=ep[3] if ep[3] >= 0 else None) if ep is not None else {}
            y = conv2d_mfma16.conv2d_forward(xp, packed, cout, kh, kw, stride=stride, pad=padding, bias=b32, **fz)
        else:
            assert ep is None
            cout = int(weight.shape[1])
            out_hw = ((h - 1) * stride - 2 * padding[0] + kh + output_padding[0], (w - 1) * stride - 2 * padding[1] + kw + output_padding[1])
            phases = conv2d_mfma16.pack_transposed(wf, x.dtype, stride, padding, (h, w), out_hw)
            y = conv2d_mfma16.conv_transpose2d_forward(xp, phases, cout, out_hw, stride=stride, bias=b32)
        ctx.save_for_backward(x, weight, y if ep is not None else None)
        ctx.cfg = (stride, padding, transposed, output_padding, bias is not None, ep)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        stride, padding, transposed, output_padding, has_bias, ep = ctx.cfg
        dx = dw = db = None
        if ep is not None:
            dy, db = _epilogue_backward(ctx, dy, y, ep, has_bias and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[0]:
            dx = _input_gradient(dy, x.shape, weight, stride, padding, transposed, output_padding, fn=_Conv2dMfma16, mod=conv2d_mfma16)
        want_w = ctx.needs_input_grad[1] and not weight_gradients_disabled
        want_b = has_bias and ctx.needs_input_grad[2]
        if want_w and native_weight_gradients16 and not (torch.is_grad_enabled() and (dy.requires_grad or x.requires_grad)):
            if not transposed:
                g = conv2d_mfma16.weight_gradient(x, dy, weight.shape, padding, stride=stride)    # float32 [Cout, Cin, kh, kw]; None = not covered
            else:
                # y = conv_transpose2d(x, w[Cin, Cout]): dw[ci, co] = the weight gradient of the strided convolution dy -> x, whose OIHW kernel has O = Cin, I = Cout --
                # the same kernel with the roles swapped (as `_weight_gradient` does in float32).  Round 5: this case went to aten (MIOpen), whose stride-2 16-bit
                # weight gradient is not run-to-run reproducible -- it is the input-gradient node of the half-precision down-sampling convolutions under R1's double
                # backward (tools/probes/d_fp16_determinism.py: `bNN.conv1.weight` differed between identical runs).
                g = conv2d_mfma16.weight_gradient(dy, x, weight.shape, padding, stride=stride)
            dw = g.to(weight.dtype) if g is not None else None
        if want_b and db is None and (dw is not None or not want_w):
            db = bias_act.channel_sum(dy, 1)
        need_x = dx is None and ctx.needs_input_grad[0]
        need_w = want_w and dw is None
        need_b = want_b and db is None
        if need_x or need_w or need_b:
            gx, gw, gb = torch.ops.aten.convolution_backward(
                dy, x, weight.to(x.dtype), [weight.shape[1 if transposed else 0]] if has_bias else None,
                [stride, stride], list(padding), [1, 1], transposed, list(output_padding), 1, [need_x, need_w, need_b])
            dx = gx if need_x else dx
            dw = gw.to(weight.dtype) if need_w else dw
            db = gb if need_b else db
        return dx, dw, db, None, None, None, None, None


def _input_gradient(dy, x_shape, weight, stride, padding, transposed, output_padding, fn=None, mod=None):
    """d(loss)/dx of y = conv(x, w) (or conv_transpose) as another native convolution; None if that geometry is not covered."""
    _Conv2dMfma, conv2d_mfma = (fn or globals()['_Conv2dMfma']), (mod or globals()['conv2d_mfma'])
    kh, kw = int(weight.shape[2]), int(weight.shape[3])
    _, _, h, w = x_shape
    if not transposed:
        if stride == 1:        # dx = correlate(dy, w^T flipped) with padding k-1-p
            py, px = kh - 1 - padding[0], kw - 1 - padding[1]
            if min(py, px) < 0 or not conv2d_mfma.supported(kh, kw, 1):
                return None
            if fn is None and not (torch.is_grad_enabled() and (dy.requires_grad or weight.requires_grad)):
                # plain first-order backward: the flipped / transposed pack comes straight from the parameter (cached per version),
                # no transposed copy of the weight tensor is made
                cin_f = int(weight.shape[1])
                wg = globals()['conv2d_mfma'].use_winograd(kh, kw, 1, cin_f, int(weight.shape[0]), pad=(py, px), hw=dy.shape[2:])
                pk = _packed(weight, wg, flip=True, transpose_oi=True)
                return globals()['conv2d_mfma'].conv2d_forward(dy.contiguous(), pk, cin_f, kh, kw, stride=1, pad=(py, px), winograd=wg)
            return _Conv2dMfma.apply(dy, weight.transpose(0, 1).flip([2, 3]), None, 1, (py, px), False, (0, 0))
        # strided conv: dx = conv_transpose(dy, w, stride) with the output padding that restores x's size
        opad = (h - ((dy.shape[2] - 1) * stride - 2 * padding[0] + kh), w - ((dy.shape[3] - 1) * stride - 2 * padding[1] + kw))
        if min(opad) < 0 or max(opad) >= stride or kh < stride or kw < stride:
            return None
        if not all(conv2d_mfma.supported(-(-(kh - a) // stride), -(-(kw - b) // stride), 1) for a in range(stride) for b in range(stride)):
            return None
        return _Conv2dMfma.apply(dy, weight, None, stride, padding, True, opad)
    # forward was conv_transpose(x, w[Cin, Cout]): dx = conv(dy, w, stride) -- w read as OIHW with O = Cin
    if not conv2d_mfma.supported(kh, kw, stride) or min(padding) < 0:
        return None
    dx = _Conv2dMfma.apply(dy, weight, None, stride, padding, False, (0, 0))
    return dx if dx.shape[2:] == tuple(x_shape[2:]) else None
