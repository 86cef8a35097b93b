"""The two operators of the VGG19 perceptual loss (training/vgg_loss.py) that are not convolutions, on MI355X.

``maxpool2x2(x)`` is ``nn.MaxPool2d(2, 2)`` (floor semantics: a trailing odd row or column is dropped).  ``l1_mean(x, y, groups)`` is
``nn.L1Loss()`` between each of the `groups` tensors stacked on `x`'s batch axis and the one `y`: ``[G]`` means.  `y` carries no gradient
(the reference detaches the target's features, loss_fullbody.py:347).

Dispatch follows the other ops: a GPU tensor runs ``csrc/vgg_loss.hip`` (``pg_maxpool2x2`` / ``pg_maxpool2x2_backward`` /
``pg_l1_pair_sum`` / ``pg_l1_pair_grad``), never reads a value to the host and uses no atomics; a CPU tensor runs ``F.max_pool2d`` or the
``(x - y).abs().mean()`` composition.  Both are first-order: the term lives in Gmain only, which takes no second derivative, and the
native backwards are marked ``once_differentiable`` so that a double backward raises instead of returning a wrong zero.
"""

import ctypes

import torch
from torch.autograd.function import once_differentiable

from .. import custom_ops
from . import _native as nat

_plugin = None
MAX_GROUPS = 8          # PG_L1_PAIR_MAX_GROUPS


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('vgg_loss_plugin')
        p, i, l, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        plugin.lib.pg_maxpool2x2.argtypes = [p, p, l, i, i, p]
        plugin.lib.pg_maxpool2x2_backward.argtypes = [p, p, p, l, i, i, p]
        plugin.lib.pg_l1_pair_blocks.argtypes = [l]
        plugin.lib.pg_l1_pair_sum.argtypes = [p, p, p, p, i, l, d, p]
        plugin.lib.pg_l1_pair_grad.argtypes = [p, p, p, p, i, l, d, p]
        for fn in (plugin.lib.pg_maxpool2x2, plugin.lib.pg_maxpool2x2_backward, plugin.lib.pg_l1_pair_blocks, plugin.lib.pg_l1_pair_sum,
                   plugin.lib.pg_l1_pair_grad):
            fn.restype = ctypes.c_int
        _plugin = plugin
    return True


def _check_feature(x, what):
    if x.dtype != torch.float32:
        raise nat.NativeOpError(f'{what}: float32 tensors only, got {x.dtype}')
    if x.ndim != 4:
        raise nat.NativeOpError(f'{what}: tensors must be NCHW (rank 4)')
    return x.contiguous()


class _MaxPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _init()
        n, c, h, w = x.shape
        y = torch.empty([n, c, h // 2, w // 2], dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            st = _plugin.lib.pg_maxpool2x2(nat.ptr(x), nat.ptr(y), n * c, h, w, nat.stream_of(x))
        nat.check(st, 'pg_maxpool2x2')
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        n, c, h, w = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)                       # every element is written by the kernel
        with torch.cuda.device(x.device):
            st = _plugin.lib.pg_maxpool2x2_backward(nat.ptr(x), nat.ptr(dy), nat.ptr(dx), n * c, h, w, nat.stream_of(x))
        nat.check(st, 'pg_maxpool2x2_backward')
        return dx


class _L1Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, groups):
        _init()
        m = y.numel()
        out = torch.empty([groups], dtype=torch.float32, device=x.device)
        partials = torch.empty([groups * _plugin.lib.pg_l1_pair_blocks(m)], dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            st = _plugin.lib.pg_l1_pair_sum(nat.ptr(x), nat.ptr(y), nat.ptr(partials), nat.ptr(out), groups, m, 1.0 / m, nat.stream_of(x))
        nat.check(st, 'pg_l1_pair_sum')
        ctx.save_for_backward(x, y)
        ctx.groups = groups
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, y = ctx.saved_tensors
        dout = dout.contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            st = _plugin.lib.pg_l1_pair_grad(nat.ptr(x), nat.ptr(y), nat.ptr(dout), nat.ptr(dx), ctx.groups, y.numel(), float(y.numel()), nat.stream_of(x))
        nat.check(st, 'pg_l1_pair_grad')
        return dx, None, None


# ---------------------------------------------------------------------------- public ops

def maxpool2x2(x):
    """``F.max_pool2d(x, 2, 2)`` of an NCHW tensor, with aten's tie rule in the backward (first maximum in row-major order; a NaN wins)."""
    assert isinstance(x, torch.Tensor)
    if x.device.type != 'cuda':
        return torch.nn.functional.max_pool2d(x, kernel_size=2, stride=2)
    x = _check_feature(x, 'maxpool2x2')
    if x.shape[2] < 2 or x.shape[3] < 2 or x.shape[0] * x.shape[1] == 0:
        raise nat.NativeOpError(f'maxpool2x2: needs a non-empty batch with H, W >= 2, got {list(x.shape)}')
    return _MaxPool2x2.apply(x)


def l1_mean(x, y, groups=1):
    """`x` = [G * N, C, H, W] (G groups stacked on the batch axis), `y` = [N, C, H, W]: the G means of |x_g - y|, shape [G].  No gradient
    reaches `y`."""
    assert isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)
    groups = int(groups)
    if groups < 1 or x.ndim != y.ndim or x.ndim < 1 or tuple(x.shape) != (groups * y.shape[0],) + tuple(y.shape[1:]) or y.numel() == 0:
        raise (nat.NativeOpError if x.device.type == 'cuda' else ValueError)(
            f'l1_mean: x must stack {groups} group(s) of y\'s shape {list(y.shape)} on the batch axis, got {list(x.shape)}')
    y = y.detach()
    if x.device.type != 'cuda':
        return (x.reshape([groups, -1]) - y.reshape([1, -1])).abs().mean(dim=1)
    x, y = _check_feature(x, 'l1_mean'), _check_feature(y, 'l1_mean')
    if y.device != x.device:
        raise nat.NativeOpError('l1_mean: x and y must be on the same device')
    if groups > MAX_GROUPS:
        raise nat.NativeOpError(f'l1_mean: at most {MAX_GROUPS} groups')
    return _L1Mean.apply(x, y, groups)
