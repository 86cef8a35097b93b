"""The contextual loss of the reference's ``ContextualLoss_forward`` (training/loss_fullbody.py:564-618, PONO centring) on MI355X.

``contextual_loss(x, y, h=0.1, groups=1)``: `x` = [G * N, C, H, W] (G groups stacked on the batch axis), `y` = [N, C, H, W]; sample `s` of `x`
meets sample ``s % N`` of `y`; the result is the [G * N] per-sample losses, as the reference's class returns them.  `y` carries no gradient.

For one sample, P = H * W positions, ``mu_p = mean_c y[c, p]``, ``xn_p = (x_p - mu_p) / (|x_p - mu_p| + eps)``, `yn` likewise:
``d_ij = 1 - xn_i . yn_j``, ``w_ij = exp((1 - d_ij / (min_j d_ij + 1e-3)) / h)``, ``A_ij = w_ij / sum_j w_ij``, ``CX = mean_i max_j A_ij``,
``loss = -log CX``.

A GPU tensor runs ``csrc/contextual.hip``: the P x P affinity is streamed through the float32 matrix instruction twice forward and once
backward and never stored; no atomics, no value read to the host.  A CPU tensor runs the literal torch composition of the reference.  First
order only: the native backward is ``once_differentiable``.
"""

import ctypes
import sys

import torch
from torch.autograd.function import once_differentiable

from .. import custom_ops
from . import _native as nat

_plugin = None
MAX_GROUPS = 8          # PG_CX_MAX_GROUPS
EPS = sys.float_info.epsilon


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('contextual_plugin')
        p, i, l, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        lib = plugin.lib
        lib.pg_cx_padded_channels.argtypes = [i]
        lib.pg_cx_prepare.argtypes = [p, p, p, p, p, i, i, i, l, p]
        lib.pg_cx_prepare_backward.argtypes = [p, p, p, p, i, i, l, p]
        lib.pg_cx_forward.argtypes = [p] * 9 + [i, i, i, l, d, p]
        lib.pg_cx_backward.argtypes = [p] * 10 + [i, i, i, l, d, p]
        for fn in (lib.pg_cx_padded_channels, lib.pg_cx_prepare, lib.pg_cx_prepare_backward, lib.pg_cx_forward, lib.pg_cx_backward):
            fn.restype = ctypes.c_int
        _plugin = plugin
    return True


# ---------------------------------------------------------------------------- the native pieces (GPU tensors, already checked)

def prepare(x, y):
    """`x` [S, C, H, W], `y` [N, C, H, W] (S a multiple of N) -> ``xn`` [S, P, Cp], ``yn`` [N, P, Cp] (centred, normalised, position-major, Cp = C
    rounded up to 32 with zero padding) and ``rx`` [S, P] = the norms of the centred `x`."""
    _init()
    s, c, h, w = x.shape
    n, pos = y.shape[0], h * w
    cp = _plugin.lib.pg_cx_padded_channels(c)
    xn = torch.empty([s, pos, cp], dtype=torch.float32, device=x.device)
    yn = torch.empty([n, pos, cp], dtype=torch.float32, device=x.device)
    rx = torch.empty([s, pos], dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = _plugin.lib.pg_cx_prepare(nat.ptr(x), nat.ptr(y), nat.ptr(xn), nat.ptr(yn), nat.ptr(rx), s, n, c, pos, nat.stream_of(x))
    nat.check(st, 'pg_cx_prepare')
    return xn, yn, rx


def prepare_backward(dxn, xn, rx, shape):
    """The gradient with respect to `x` ([S, C, H, W] = `shape`) of ``prepare`` from `dxn` [S, P, Cp]."""
    _init()
    s, c, h, w = shape
    dx = torch.empty(list(shape), dtype=torch.float32, device=dxn.device)          # every element is written by the kernel
    with torch.cuda.device(dxn.device):
        st = _plugin.lib.pg_cx_prepare_backward(nat.ptr(dxn), nat.ptr(xn), nat.ptr(rx), nat.ptr(dx), s, c, h * w, nat.stream_of(dxn))
    nat.check(st, 'pg_cx_prepare_backward')
    return dx


def forward_sweeps(xn, yn, channels, h):
    """``pg_cx_forward`` on prepared operands -> (loss [S], stats): `stats` = the row statistics (m, jmin, S', T', a; [S, P] each) and CX [S], what
    ``backward_sweep`` takes."""
    _init()
    s, pos = xn.shape[0], xn.shape[1]
    new = lambda dtype=torch.float32, shape=(s, pos): torch.empty(list(shape), dtype=dtype, device=xn.device)      # noqa: E731
    m, jmin, others, tsum, a = new(), new(torch.int32), new(), new(), new()
    cx, loss = new(shape=(s,)), new(shape=(s,))
    with torch.cuda.device(xn.device):
        st = _plugin.lib.pg_cx_forward(nat.ptr(xn), nat.ptr(yn), nat.ptr(m), nat.ptr(jmin), nat.ptr(others), nat.ptr(tsum), nat.ptr(a), nat.ptr(cx),
                                       nat.ptr(loss), s, yn.shape[0], channels, pos, h, nat.stream_of(xn))
    nat.check(st, 'pg_cx_forward')
    return loss, (m, jmin, others, tsum, a, cx)


def backward_sweep(xn, yn, stats, gout, channels, h):
    """``pg_cx_backward``: dxn [S, P, Cp] from the forward's statistics and `gout` [S]."""
    _init()
    dxn = torch.empty_like(xn)                              # every element is written by the kernel
    with torch.cuda.device(xn.device):
        st = _plugin.lib.pg_cx_backward(nat.ptr(xn), nat.ptr(yn), *[nat.ptr(t) for t in stats], nat.ptr(gout), nat.ptr(dxn), xn.shape[0], yn.shape[0],
                                        channels, xn.shape[1], h, nat.stream_of(xn))
    nat.check(st, 'pg_cx_backward')
    return dxn


class _Contextual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, h):
        xn, yn, rx = prepare(x, y)
        loss, stats = forward_sweeps(xn, yn, x.shape[1], h)
        ctx.save_for_backward(xn, yn, rx, *stats)
        ctx.h, ctx.shape = h, tuple(x.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        xn, yn, rx, *stats = ctx.saved_tensors
        dxn = backward_sweep(xn, yn, stats, gout.to(torch.float32).contiguous(), ctx.shape[1], ctx.h)
        return prepare_backward(dxn, xn, rx, ctx.shape), None, None


# ---------------------------------------------------------------------------- the torch composition (CPU route; the reference's own lines)

def contextual_loss_composition(x, y, h=0.1):
    """``ContextualLoss_forward(PONO=True).forward(x, y, h)`` restated line by line; `x` and `y` of one shape, any float dtype and device."""
    b, c = x.shape[0], x.shape[1]
    mu = y.mean(dim=1).unsqueeze(dim=1)
    x, y = x - mu, y - mu
    x = (x / (torch.norm(x, p=2, dim=1, keepdim=True) + EPS)).view(b, c, -1)
    y = (y / (torch.norm(y, p=2, dim=1, keepdim=True) + EPS)).view(b, c, -1)
    d = 1 - torch.matmul(x.permute(0, 2, 1), y)
    d_norm = d / (torch.min(d, dim=-1, keepdim=True)[0] + 1e-3)
    w = torch.exp((1 - d_norm) / h)
    a_ij = w / torch.sum(w, dim=-1, keepdim=True)
    cx = torch.mean(torch.max(a_ij, dim=-1)[0], dim=1)
    return -torch.log(cx)


# ---------------------------------------------------------------------------- public op

def _fail(x, msg):
    raise (nat.NativeOpError if x.device.type == 'cuda' else ValueError)(msg)


def contextual_loss(x, y, h=0.1, groups=1):
    """[G * N] per-sample contextual losses of `x` = [G * N, C, H, W] against `y` = [N, C, H, W]; no gradient reaches `y`."""
    assert isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)
    groups, h = int(groups), float(h)
    if x.ndim != 4 or y.ndim != 4:
        _fail(x, 'contextual_loss: tensors must be NCHW (rank 4)')
    if groups < 1 or tuple(x.shape) != (groups * y.shape[0],) + tuple(y.shape[1:]) or y.numel() == 0:
        _fail(x, f'contextual_loss: x must stack {groups} group(s) of y\'s shape {list(y.shape)} on the batch axis, got {list(x.shape)}')
    if not h > 0:
        _fail(x, f'contextual_loss: the bandwidth h must be positive, got {h}')
    y = y.detach()
    if x.device.type != 'cuda':
        return contextual_loss_composition(x, y.repeat([groups, 1, 1, 1]) if groups > 1 else y, h)
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise nat.NativeOpError(f'contextual_loss: float32 tensors only, got {x.dtype} and {y.dtype}')
    if y.device != x.device:
        raise nat.NativeOpError('contextual_loss: x and y must be on the same device')
    if groups > MAX_GROUPS:
        raise nat.NativeOpError(f'contextual_loss: at most {MAX_GROUPS} groups')
    return _Contextual.apply(x.contiguous(), y.contiguous(), h)
