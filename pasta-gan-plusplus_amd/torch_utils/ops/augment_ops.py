"""The image operators of ADA's AugmentPipe (training/augment.py), on MI355X.

``geometric(x, g_inv, margins, f)`` is the reference's "Execute geometric transformations" block (augment.py:270-301): reflect-pad
by the per-sample-derived margin, 2x upsample with the sym6 filter `f`, per-sample affine bilinear resampling, 2x downsample.
``color(x, C)`` is its "Execute color transformations" block (augment.py:356-366).  ``late(x, taps, noise, sigma, cut)`` is the rest
of the pipe (augment.py:372-431): the per-sample separable image filter behind its reflect pad, additive noise and cutout, one
``pg_augment_late`` launch.  All are affine in the image; the sampling matrices, margins, colour matrices and late parameters carry
no gradient (AugmentPipe is ``requires_grad_(False)``).

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
        plugin.lib.pg_augment_late.argtypes = [p, p, p, i, p, p, p, i, i, i, i, i, p]
        for fn in (plugin.lib.pg_augment_warp, plugin.lib.pg_augment_warp_adjoint, plugin.lib.pg_augment_color, plugin.lib.pg_augment_late):
            fn.restype = ctypes.c_int
        plugin.late = plugin.lib.pg_augment_late          # bound once: the late stages' host path is as long as their kernels
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


_LATE_AFFINE, _LATE_LINEAR, _LATE_ADJOINT = 0, 1, 2           # pg_augment_late modes
MAX_LATE_TAPS = 43      # Hz_fbank.shape[1]: what csrc/augment.hip is built for


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _late_native(x, taps, noise, sigma, cut, mode):
    """One pg_augment_late launch on checked, contiguous tensors (a None: that stage is off).  These stages are short next to their host work, so the
    call is kept lean: raw addresses, and no device guard where the image's device is already current."""
    if _plugin is None:
        _init()
    n, c, h, w = x.shape
    y = torch.empty_like(x)
    index = x.device.index
    guard = None
    if index != torch.cuda.current_device():
        guard = torch.cuda.device(index)
        guard.__enter__()
    try:
        stream = _raw_stream(index) if _raw_stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        st = _plugin.late(x.data_ptr(), y.data_ptr(), taps.data_ptr() if taps is not None else None, taps.shape[1] if taps is not None else 0,
                          noise.data_ptr() if noise is not None else None, sigma.data_ptr() if sigma is not None else None,
                          cut.data_ptr() if cut is not None else None, n, c, h, w, mode, stream)
    finally:
        if guard is not None:
            guard.__exit__(None, None, None)
    if st != 0:
        nat.check(st, 'pg_augment_late')
    return y


class _Late(torch.autograd.Function):
    """mode AFFINE: y = M (F x + noise sigma); LINEAR: y = M F x; ADJOINT: y = F^T (M x) (F = the reflect-padded separable filter, M = the cutout mask).
    Backward: AFFINE and LINEAR -> ADJOINT, ADJOINT -> LINEAR (the noise drops out of every derivative; with neither F nor M it is the identity)."""
    @staticmethod
    def forward(ctx, x, taps, noise, sigma, cut, mode):
        ctx.params = (taps, cut)
        ctx.mode = mode
        return _late_native(x, taps, noise, sigma, cut, mode)

    @staticmethod
    def backward(ctx, dy):
        taps, cut = ctx.params
        if taps is None and cut is None:
            return dy, None, None, None, None, None
        mode = _LATE_LINEAR if ctx.mode == _LATE_ADJOINT else _LATE_ADJOINT
        return _late_apply(dy.contiguous(), taps, None, None, cut, mode), None, None, None, None, None


def _late_apply(x, taps, noise, sigma, cut, mode):
    """Through autograd only where a gradient is being recorded."""
    if x.requires_grad and torch.is_grad_enabled():
        return _Late.apply(x, taps, noise, sigma, cut, mode)
    return _late_native(x, taps, noise, sigma, cut, mode)


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



def late_reference(x, taps, noise, sigma, cut):
    """The reference composition (augment.py:397-431) in plain torch, in the image's dtype."""
    n, c, h, w = x.shape
    if taps is not None:
        f = taps.to(x.dtype).unsqueeze(1).repeat([1, c, 1]).reshape([n * c, 1, -1])
        p = taps.shape[1] // 2
        x = x.reshape([1, n * c, h, w])
        x = torch.nn.functional.pad(input=x, pad=[p, p, p, p], mode='reflect')
        x = torch.nn.functional.conv2d(x, f.unsqueeze(2), groups=n * c)
        x = torch.nn.functional.conv2d(x, f.unsqueeze(3), groups=n * c)
        x = x.reshape([n, c, h, w])
    if noise is not None:
        x = x + noise.to(x.dtype) * sigma.to(x.dtype).reshape([n, 1, 1, 1])
    if cut is not None:
        cut = cut.to(x.dtype)
        center, size = cut[:, :2].reshape([n, 2, 1, 1, 1]), cut[:, 2:].reshape([n, 2, 1, 1, 1])
        coord_x = torch.arange(w, device=x.device).reshape([1, 1, 1, -1])
        coord_y = torch.arange(h, device=x.device).reshape([1, 1, -1, 1])
        mask_x = (((coord_x + 0.5) / w - center[:, 0]).abs() >= size[:, 0] / 2)
        mask_y = (((coord_y + 0.5) / h - center[:, 1]).abs() >= size[:, 1] / 2)
        x = x * torch.logical_or(mask_x, mask_y).to(x.dtype)
    return x


def _check_late(x, taps, noise, sigma, cut):
    n, c, h, w = x.shape
    dev, f32, T = x.device, torch.float32, torch.Tensor
    if taps is not None:
        if not (isinstance(taps, T) and taps.ndim == 2 and taps.dtype == f32 and taps.shape[0] == n and taps.device == dev):
            raise nat.NativeOpError('augment late: taps must be float32 [N, K] on the images\' device')
        k = taps.shape[1]
        if k % 2 == 0 or k > MAX_LATE_TAPS:
            raise nat.NativeOpError(f'augment late: the filter must have an odd number of taps, at most {MAX_LATE_TAPS}; got {k}')
        if h <= k // 2 or w <= k // 2:
            raise nat.NativeOpError(f'augment late: reflect padding by {k // 2} needs H, W >= {k // 2 + 1}')
        if taps.requires_grad or not taps.is_contiguous():
            taps = taps.detach().contiguous()
    if (noise is None) != (sigma is None):
        raise nat.NativeOpError('augment late: noise and sigma come together')
    if noise is not None:
        if not (isinstance(noise, T) and isinstance(sigma, T) and noise.dtype == f32 and sigma.dtype == f32 and noise.shape == x.shape
                and sigma.numel() == n and noise.device == dev and sigma.device == dev):
            raise nat.NativeOpError('augment late: noise must be float32 [N, C, H, W] and sigma float32 [N] on the images\' device')
        if noise.requires_grad or not noise.is_contiguous():
            noise = noise.detach().contiguous()
        if sigma.requires_grad or not sigma.is_contiguous():
            sigma = sigma.detach().contiguous()
    if cut is not None:
        if not (isinstance(cut, T) and cut.dtype == f32 and cut.shape == (n, 4) and cut.device == dev):
            raise nat.NativeOpError('augment late: cut must be float32 [N, 4] (centre x, centre y, size x, size y) on the images\' device')
        if cut.requires_grad or not cut.is_contiguous():
            cut = cut.detach().contiguous()
    return taps, noise, sigma, cut


def late(x, taps=None, noise=None, sigma=None, cut=None):
    """AugmentPipe's late stages in the reference's order: `taps` = per-sample 1-D filters [N, K] (K odd; rows, then columns, behind a reflect pad of
    K // 2), `noise` [N, C, H, W] scaled by `sigma` [N] and added, `cut` = [N, 4] (centre x, centre y, size x, size y in units of the image) zeroed.
    None switches a stage off.  Output has the input's shape; the parameters carry no gradient."""
    assert isinstance(x, torch.Tensor)
    if taps is None and noise is None and sigma is None and cut is None:
        return x
    if x.device.type != 'cuda':
        det = lambda t: None if t is None else t.detach()
        return late_reference(x, det(taps), det(noise), det(sigma), det(cut))
    x = _check_image(x, 'augment late')
    taps, noise, sigma, cut = _check_late(x, taps, noise, sigma, cut)
    return _late_apply(x, taps, noise, sigma, cut, _LATE_AFFINE)
