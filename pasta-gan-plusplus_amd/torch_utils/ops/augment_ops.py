"""The two image operators of ADA's AugmentPipe (training/augment.py), on MI355X.

``geometric(x, g_inv, margins, f)`` is the reference's "Execute geometric transformations" block (augment.py:270-301): reflect-pad
by the per-sample-derived margin, 2x upsample with the sym6 filter `f`, per-sample affine bilinear resampling, 2x downsample.
``color(x, C)`` is its "Execute color transformations" block (augment.py:356-366).  Both are linear in the image; the sampling
matrices, margins and colour matrices carry no gradient (AugmentPipe is ``requires_grad_(False)``).

Dispatch follows the other ops: a GPU tensor runs ``csrc/augment.hip`` (``pg_augment_warp`` / ``pg_augment_warp_adjoint`` /
``pg_augment_color``) with the downsample on ``pg_upfirdn2d``, and never reads a value to the host; a CPU tensor runs the
reference composition in plain torch.  The backward of each native op is its transpose, whose backward is the op's linear part
(the warp itself; the colour matrix without its offset), so R1's double backward (training/loss.py) stays on the native kernels.
"""

import ctypes

import torch

from .. import custom_ops
from . import _native as nat
from . import upfirdn2d

_plugin = None
HZ_PAD = 3          # Hz_geom.shape[0] // 4 (augment.py:276) for the 12-tap sym6 filter


def _init():
    global _plugin
    if _plugin is None:
        plugin = custom_ops.get_plugin('augment_plugin')
        p, i = ctypes.c_void_p, ctypes.c_int
        plugin.lib.pg_augment_warp.argtypes = [p, p, p, p, p, i, i, i, i, p]
        plugin.lib.pg_augment_warp_adjoint.argtypes = [p, p, p, p, p, p, i, i, i, i, p]
        plugin.lib.pg_augment_color.argtypes = [p, p, p, i, i, i, i, p]
        for fn in (plugin.lib.pg_augment_warp, plugin.lib.pg_augment_warp_adjoint, plugin.lib.pg_augment_color):
            fn.restype = ctypes.c_int
        _plugin = plugin
    return True


def _check_image(x, what):
    if x.dtype != torch.float32:
        raise nat.NativeOpError(f'{what}: float32 images only, got {x.dtype}')
    if x.ndim != 4:
        raise nat.NativeOpError(f'{what}: images must be NCHW (rank 4)')
    return x.contiguous()


def _check_params(x, g_inv, margins, f):
    n, _, h, w = x.shape
    if g_inv.dtype != torch.float32 or tuple(g_inv.shape) != (n, 3, 3) or g_inv.device != x.device:
        raise nat.NativeOpError('augment warp: g_inv must be float32 [N, 3, 3] on the images\' device')
    if margins.dtype != torch.int32 or margins.numel() != 4 or margins.device != x.device:
        raise nat.NativeOpError('augment warp: margins must be int32 [4] on the images\' device')
    if f.dtype != torch.float32 or f.numel() != 4 * HZ_PAD or f.device != x.device:
        raise nat.NativeOpError('augment warp: f must be the 12 float32 taps of Hz_geom on the images\' device')
    if h < 2 or w < 2:
        raise nat.NativeOpError('augment warp: reflect padding needs H, W >= 2')
    return g_inv.contiguous(), margins.contiguous(), f.contiguous()


def _warp_native(x, g_inv, margins, f):
    _init()
    n, c, h, w = x.shape
    y = torch.empty([n, c, 2 * (h + 2 * HZ_PAD), 2 * (w + 2 * HZ_PAD)], dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        st = _plugin.lib.pg_augment_warp(nat.ptr(x), nat.ptr(y), nat.ptr(g_inv), nat.ptr(margins), nat.ptr(f), n, c, h, w, nat.stream_of(x))
    nat.check(st, 'pg_augment_warp')
    return y


def _warp_adjoint_native(dy, g_inv, margins, f, h, w):
    _init()
    n, c = dy.shape[:2]
    assert tuple(dy.shape[2:]) == (2 * (h + 2 * HZ_PAD), 2 * (w + 2 * HZ_PAD))
    ws = torch.empty([n, c, 2 * (3 * h - 2), 2 * (3 * w - 2)], dtype=dy.dtype, device=dy.device)   # only the live corner is written and read
    dx = torch.empty([n, c, h, w], dtype=dy.dtype, device=dy.device)
    with torch.cuda.device(dy.device):
        st = _plugin.lib.pg_augment_warp_adjoint(nat.ptr(dy), nat.ptr(ws), nat.ptr(dx), nat.ptr(g_inv), nat.ptr(margins), nat.ptr(f), n, c, h, w, nat.stream_of(dy))
    nat.check(st, 'pg_augment_warp_adjoint')
    return dx


class _Warp(torch.autograd.Function):
    """x [N, C, H, W] -> the grid-sampled, up-sampled padded image [N, C, 2(H+6), 2(W+6)] (before the downsample)."""
    @staticmethod
    def forward(ctx, x, g_inv, margins, f):
        ctx.save_for_backward(g_inv, margins, f)
        ctx.hw = x.shape[2:]
        return _warp_native(x, g_inv, margins, f)

    @staticmethod
    def backward(ctx, dy):
        g_inv, margins, f = ctx.saved_tensors
        return _WarpT.apply(dy.contiguous(), g_inv, margins, f, ctx.hw[0], ctx.hw[1]), None, None, None


class _WarpT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, g_inv, margins, f, h, w):
        ctx.save_for_backward(g_inv, margins, f)
        return _warp_adjoint_native(dy, g_inv, margins, f, h, w)

    @staticmethod
    def backward(ctx, ddx):
        g_inv, margins, f = ctx.saved_tensors
        return _Warp.apply(ddx.contiguous(), g_inv, margins, f), None, None, None, None, None


_COLOR_AFFINE, _COLOR_TRANSPOSE, _COLOR_LINEAR = 0, 1, 2      # pg_augment_color modes


def _color_native(x, mat, mode):
    _init()
    n, c, h, w = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = _plugin.lib.pg_augment_color(nat.ptr(x), nat.ptr(y), nat.ptr(mat), n, c, h * w, mode, nat.stream_of(x))
    nat.check(st, 'pg_augment_color')
    return y


class _Color(torch.autograd.Function):
    """mode AFFINE: y = M x + t per sample; TRANSPOSE: y = M^T x; LINEAR: y = M x (mat = [N, C, C + 1]).  Backward: AFFINE and LINEAR -> TRANSPOSE,
    TRANSPOSE -> LINEAR (the offset drops out of every derivative)."""
    @staticmethod
    def forward(ctx, x, mat, mode):
        ctx.save_for_backward(mat)
        ctx.mode = mode
        return _color_native(x, mat, mode)

    @staticmethod
    def backward(ctx, dy):
        mat, = ctx.saved_tensors
        return _Color.apply(dy.contiguous(), mat, _COLOR_LINEAR if ctx.mode == _COLOR_TRANSPOSE else _COLOR_TRANSPOSE), None, None


# ---------------------------------------------------------------------------- public ops

def _translate2d(tx, ty, like):
    m = torch.eye(3, dtype=like.dtype, device=like.device)
    m[0, 2], m[1, 2] = tx, ty
    return m


def _scale2d(sx, sy, like):
    return torch.diag(torch.tensor([sx, sy, 1.0], dtype=like.dtype, device=like.device))


class _GridSample(torch.autograd.Function):
    """F.grid_sample(x, grid, 'bilinear', 'zeros', align_corners=False), differentiable to any order in `x` (aten's grid_sampler_2d_backward
    has no derivative; R1's double backward on the CPU route needs one -- the reference's grid_sample_gradfix fills the same gap on its GPU
    route).  The backward is aten's own input gradient, whose backward is the sampling again; `grid` carries no gradient."""
    @staticmethod
    def forward(ctx, x, grid):
        ctx.save_for_backward(grid)
        ctx.x_shape = x.shape
        return torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)

    @staticmethod
    def backward(ctx, dy):
        grid, = ctx.saved_tensors
        return _GridSampleT.apply(dy, grid, ctx.x_shape), None


class _GridSampleT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, grid, x_shape):
        ctx.save_for_backward(grid)
        x = dy.new_empty([]).expand(x_shape)
        return torch.ops.aten.grid_sampler_2d_backward(dy, x, grid, 0, 0, False, [True, False])[0]

    @staticmethod
    def backward(ctx, ddx):
        grid, = ctx.saved_tensors
        return _GridSample.apply(ddx, grid), None, None


def _geometric_torch(x, g_inv, margins, f):
    """The reference composition (augment.py:270-301) in plain torch: reads the margins to the host (CPU tensors only)."""
    n, c, h, w = x.shape
    mx0, my0, mx1, my1 = [int(v) for v in margins.cpu()]
    g_inv = g_inv.to(x.dtype)
    x = torch.nn.functional.pad(input=x, pad=[mx0, mx1, my0, my1], mode='reflect')
    g_inv = _translate2d((mx0 - mx1) / 2, (my0 - my1) / 2, g_inv) @ g_inv
    x = upfirdn2d.upsample2d(x=x, f=f, up=2, impl='ref')
    g_inv = _scale2d(2, 2, g_inv) @ g_inv @ _scale2d(1 / 2, 1 / 2, g_inv)
    g_inv = _translate2d(-0.5, -0.5, g_inv) @ g_inv @ _translate2d(0.5, 0.5, g_inv)
    shape = [n, c, (h + HZ_PAD * 2) * 2, (w + HZ_PAD * 2) * 2]
    g_inv = _scale2d(2 / x.shape[3], 2 / x.shape[2], g_inv) @ g_inv @ _scale2d(shape[3] / 2, shape[2] / 2, g_inv)
    grid = torch.nn.functional.affine_grid(theta=g_inv[:, :2, :], size=shape, align_corners=False)
    x = _GridSample.apply(x, grid.detach())
    return upfirdn2d.downsample2d(x=x, f=f, down=2, padding=-HZ_PAD * 2, flip_filter=True, impl='ref')


def geometric(x, g_inv, margins, f):
    """AugmentPipe's geometric block: `g_inv` = per-sample pixel_out -> pixel_in matrices [N, 3, 3] (before padding), `margins` =
    int32 [mx0, my0, mx1, my1] (clamped, ceiled; augment.py:277-283), `f` = Hz_geom.  Output has the input's shape."""
    assert isinstance(x, torch.Tensor)
    if x.device.type != 'cuda':
        return _geometric_torch(x, g_inv, margins.to(x.device), f.to(x.device, torch.float32))
    x = _check_image(x, 'augment warp')
    g_inv, margins, f = _check_params(x, g_inv, margins, f)
    y = _Warp.apply(x, g_inv.detach(), margins, f.detach())
    return upfirdn2d.downsample2d(x=y, f=f.detach(), down=2, padding=-HZ_PAD * 2, flip_filter=True)


def color(x, C):
    """AugmentPipe's colour block: `C` = per-sample homogeneous colour matrices [N, 4, 4]; 3 channels: C[:, :3, :3] @ x + C[:, :3, 3];
    1 channel: the reference's mean-collapsed form.  Any other channel count raises ValueError."""
    n, c, h, w = x.shape
    if c not in (1, 3):
        raise ValueError('Image must be RGB (3 channels) or L (1 channel)')
    C = C.detach()
    if x.device.type != 'cuda':
        C = C.to(x.dtype)
        x = x.reshape([n, c, h * w])
        if c == 3:
            x = C[:, :3, :3] @ x + C[:, :3, 3:]
        else:
            C = C[:, :3, :].mean(dim=1, keepdims=True)
            x = x * C[:, :, :3].sum(dim=2, keepdims=True) + C[:, :, 3:]
        return x.reshape([n, c, h, w])
    x = _check_image(x, 'augment color')
    if C.dtype != torch.float32 or tuple(C.shape) != (n, 4, 4) or C.device != x.device:
        raise nat.NativeOpError('augment color: C must be float32 [N, 4, 4] on the images\' device')
    if c == 3:
        mat = C[:, :3, :].contiguous()
    else:
        Cm = C[:, :3, :].mean(dim=1, keepdims=True)
        mat = torch.cat([Cm[:, :, :3].sum(dim=2, keepdims=True), Cm[:, :, 3:]], dim=2).contiguous()
    return _Color.apply(x, mat, _COLOR_AFFINE)
