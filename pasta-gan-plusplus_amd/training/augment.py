"""ADA's augmentation pipeline for the discriminator's image input: ``AugmentPipe``, restated from the reference's
``training/augment.py`` (the paper "Training Generative Adversarial Networks with Limited Data").

Same constructor keywords and defaults (augment.py:117-160), the same buffers (``p``, ``Hz_geom``, ``Hz_fbank``: a reference
snapshot's ``augment_pipe`` loads with ``checkpoint.load_into(pipe, snapshot, key='augment_pipe')``), and the same sequence of
``torch.rand`` / ``torch.randn`` calls, so that on one device and seed the same augmentation is drawn.  ``forward`` is split into
``sample_params`` (plain torch on [N, 3, 3] / [N, 4, 4] matrices; nothing is read to the host -- the margins are clamped and
ceiled on the device) and ``apply``, whose geometric and colour blocks are ``torch_utils.ops.augment_ops`` (HIP kernels on a GPU
tensor, the reference composition on a CPU tensor).  The late stages (``imgfilter``, ``noise``, ``cutout``) are split the same way
into ``sample_late`` and ``apply_late``; ``set_native_late(True)`` (the training driver does it) runs them on a GPU tensor as one
``pg_augment_late`` launch.  Without that switch a GPU tensor takes the torch composition, and ``imgfilter`` raises
NotImplementedError there.
"""

import itertools
import math

import numpy as np
import torch

from torch_utils.ops import augment_ops

# Named pipelines of the reference's train.py (:293-305); 'bgc' is its default.
AUGPIPE_SPECS = {
    'blit':   dict(xflip=1, rotate90=1, xint=1),
    'geom':   dict(scale=1, rotate=1, aniso=1, xfrac=1),
    'color':  dict(brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1),
    'filter': dict(imgfilter=1),
    'noise':  dict(noise=1),
    'cutout': dict(cutout=1),
    'bg':     dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1),
    'bgc':    dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1),
    'bgcf':   dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1, imgfilter=1),
    'bgcfn':  dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1, imgfilter=1, noise=1),
    'bgcfnc': dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1, imgfilter=1, noise=1,
                   cutout=1),
}

# ---------------------------------------------------------------------------- wavelet low-pass filters


def daubechies_symlet(n):
    """Low-pass decomposition filter of the Symlet with `n` vanishing moments (2n taps, sum sqrt(2)), by spectral factorisation:
    H(z) = ((1 + z^-1) / 2)^n Q(z) with |Q|^2 = P(sin^2(w/2)), P(y) = sum_k C(n-1+k, k) y^k; every root y of P contributes one of
    the reciprocal pair z + 1/z = 2 - 4y, and the Symlet is the choice whose phase is closest to linear."""
    ys = np.roots([math.comb(n - 1 + k, k) for k in range(n)][::-1])
    reps = [(y.real, False) for y in ys if abs(y.imag) < 1e-12] + [(y, True) for y in ys if y.imag >= 1e-12]
    w = np.linspace(0, np.pi, 512, endpoint=False)[1:]
    basis = np.stack([w, np.ones_like(w)], 1)
    best = None
    for choice in itertools.product([0, 1], repeat=len(reps)):
        zs = []
        for (y, pair), ch in zip(reps, choice):
            r = np.roots([1, -(2 - 4 * y), 1])
            z = r[np.argsort(np.abs(r))][ch]
            zs += [z, np.conj(z)] if pair else [z]
        h = np.real(np.poly(zs + [-1.0] * n))
        h = h / h.sum() * np.sqrt(2)
        phase = np.unwrap(np.angle(np.polyval(h[::-1], np.exp(-1j * w))))
        err = np.sum((phase - basis @ np.linalg.lstsq(basis, phase, rcond=None)[0]) ** 2)
        if best is None or err < best[0] - 1e-12:
            best = (err, h)
    return best[1]


def daubechies2():
    """db2 = sym2 low-pass taps as tabulated by PyWavelets ('db2' / 'sym2'), in the reference's tap order.  The tabulated values differ
    from the closed form (1 -+ sqrt 3, 3 -+ sqrt 3) / (4 sqrt 2) by ~3e-13, which moves the near-zero entries of the filter bank; the
    reference's Hz_fbank is built from the tabulated ones, so those are used."""
    return np.array([-0.12940952255092145, 0.22414386804185735, 0.836516303737469, 0.48296291314469025])


def _filter_bank(Hz_lo):
    """The four-band filter bank of augment.py:150-159 (np.convolve in place of scipy.signal.convolve: same full 1-D convolution per row)."""
    Hz_hi = Hz_lo * ((-1) ** np.arange(Hz_lo.size))         # H(-z)
    Hz_lo2 = np.convolve(Hz_lo, Hz_lo[::-1]) / 2            # H(z) * H(z^-1) / 2
    Hz_hi2 = np.convolve(Hz_hi, Hz_hi[::-1]) / 2            # H(-z) * H(-z^-1) / 2
    Hz_fbank = np.eye(4, 1)
    for i in range(1, Hz_fbank.shape[0]):
        Hz_fbank = np.dstack([Hz_fbank, np.zeros_like(Hz_fbank)]).reshape(Hz_fbank.shape[0], -1)[:, :-1]
        Hz_fbank = np.stack([np.convolve(row, Hz_lo2) for row in Hz_fbank])
        Hz_fbank[i, (Hz_fbank.shape[1] - Hz_hi2.size) // 2: (Hz_fbank.shape[1] + Hz_hi2.size) // 2] += Hz_hi2
    return Hz_fbank


# ---------------------------------------------------------------------------- transformation matrices

_constants = {}


def _constant(value, device):
    """A cached constant tensor (float32): built, and copied to the device, once per value and device."""
    value = np.asarray(value, dtype=np.float64)
    key = (value.shape, value.tobytes(), str(device))
    t = _constants.get(key)
    if t is None:
        t = _constants[key] = torch.as_tensor(value.copy(), dtype=torch.float32, device=device)
    return t


def matrix(*rows, device=None):
    elems = [x for row in rows for x in row]
    ref = [x for x in elems if isinstance(x, torch.Tensor)]
    if not ref:
        return _constant(rows, device)
    elems = [x if isinstance(x, torch.Tensor) else torch.full(ref[0].shape, float(x), dtype=torch.float32, device=ref[0].device) for x in elems]
    return torch.stack(elems, dim=-1).reshape(ref[0].shape + (len(rows), -1))


def translate2d(tx, ty, **kw):
    return matrix([1, 0, tx], [0, 1, ty], [0, 0, 1], **kw)


def translate3d(tx, ty, tz, **kw):
    return matrix([1, 0, 0, tx], [0, 1, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1], **kw)


def scale2d(sx, sy, **kw):
    return matrix([sx, 0, 0], [0, sy, 0], [0, 0, 1], **kw)


def scale3d(sx, sy, sz, **kw):
    return matrix([sx, 0, 0, 0], [0, sy, 0, 0], [0, 0, sz, 0], [0, 0, 0, 1], **kw)


def rotate2d(theta, **kw):
    return matrix([torch.cos(theta), torch.sin(-theta), 0], [torch.sin(theta), torch.cos(theta), 0], [0, 0, 1], **kw)


def rotate3d(v, theta, **kw):
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    s, c = torch.sin(theta), torch.cos(theta)
    cc = 1 - c
    return matrix([vx * vx * cc + c, vx * vy * cc - vz * s, vx * vz * cc + vy * s, 0],
                  [vy * vx * cc + vz * s, vy * vy * cc + c, vy * vz * cc - vx * s, 0],
                  [vz * vx * cc - vy * s, vz * vy * cc + vx * s, vz * vz * cc + c, 0],
                  [0, 0, 0, 1], **kw)


def translate2d_inv(tx, ty, **kw):
    return translate2d(-tx, -ty, **kw)


def scale2d_inv(sx, sy, **kw):
    return scale2d(1 / sx, 1 / sy, **kw)


def rotate2d_inv(theta, **kw):
    return rotate2d(-theta, **kw)


# ---------------------------------------------------------------------------- the pipeline

class AugmentPipe(torch.nn.Module):
    def __init__(self,
                 xflip=0, rotate90=0, xint=0, xint_max=0.125,
                 scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2, xfrac_std=0.125,
                 brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1, saturation_std=1,
                 imgfilter=0, imgfilter_bands=[1, 1, 1, 1], imgfilter_std=1,
                 noise=0, cutout=0, noise_std=0.1, cutout_size=0.5):
        super().__init__()
        self.register_buffer('p', torch.ones([]))        # overall multiplier for augmentation probability (ADA adjusts it)
        # pixel blitting
        self.xflip, self.rotate90, self.xint, self.xint_max = float(xflip), float(rotate90), float(xint), float(xint_max)
        # general geometric transformations
        self.scale, self.rotate, self.aniso, self.xfrac = float(scale), float(rotate), float(aniso), float(xfrac)
        self.scale_std, self.rotate_max, self.aniso_std, self.xfrac_std = float(scale_std), float(rotate_max), float(aniso_std), float(xfrac_std)
        # colour transformations
        self.brightness, self.contrast, self.lumaflip, self.hue, self.saturation = float(brightness), float(contrast), float(lumaflip), float(hue), float(saturation)
        self.brightness_std, self.contrast_std, self.hue_max, self.saturation_std = float(brightness_std), float(contrast_std), float(hue_max), float(saturation_std)
        # image-space filtering
        self.imgfilter, self.imgfilter_bands, self.imgfilter_std = float(imgfilter), list(imgfilter_bands), float(imgfilter_std)
        # image-space corruptions
        self.noise, self.cutout, self.noise_std, self.cutout_size = float(noise), float(cutout), float(noise_std), float(cutout_size)

        self.native_late = False                         # set_native_late(): a plain attribute, not a buffer

        sym6 = torch.as_tensor(daubechies_symlet(6), dtype=torch.float32)
        self.register_buffer('Hz_geom', sym6 / sym6.sum())  # upfirdn2d.setup_filter(sym6): 12 taps -> separable, normalised
        self.register_buffer('Hz_fbank', torch.as_tensor(_filter_bank(daubechies2()), dtype=torch.float32))

    def _geom_enabled(self):
        return any(v > 0 for v in (self.xflip, self.rotate90, self.xint, self.scale, self.rotate, self.aniso, self.xfrac))

    def sample_params(self, batch_size, height, width, device, debug_percentile=None, num_channels=3):
        """Draw one augmentation per sample: (G_inv [N, 3, 3] or None, margins int32 [4] or None, C [N, 4, 4] or None); None = the
        reference's identity object, whose block it skips (``G_inv is not I_3``, augment.py:271).  No value is read to the host."""
        if debug_percentile is not None:
            debug_percentile = torch.as_tensor(debug_percentile, dtype=torch.float32, device=device)
        rand = lambda *shape: torch.rand(list(shape), device=device)
        randn = lambda *shape: torch.randn(list(shape), device=device)
        n = batch_size

        # pixel blitting (augment.py:194-222)
        I_3 = torch.eye(3, device=device)
        G_inv = I_3
        if self.xflip > 0:
            i = torch.floor(rand(n) * 2)
            i = torch.where(rand(n) < self.xflip * self.p, i, torch.zeros_like(i))
            if debug_percentile is not None:
                i = torch.full_like(i, torch.floor(debug_percentile * 2))
            G_inv = G_inv @ scale2d_inv(1 - 2 * i, 1)
        if self.rotate90 > 0:
            i = torch.floor(rand(n) * 4)
            i = torch.where(rand(n) < self.rotate90 * self.p, i, torch.zeros_like(i))
            if debug_percentile is not None:
                i = torch.full_like(i, torch.floor(debug_percentile * 4))
            G_inv = G_inv @ rotate2d_inv(-np.pi / 2 * i)
        if self.xint > 0:
            t = (rand(n, 2) * 2 - 1) * self.xint_max
            t = torch.where(rand(n, 1) < self.xint * self.p, t, torch.zeros_like(t))
            if debug_percentile is not None:
                t = torch.full_like(t, (debug_percentile * 2 - 1) * self.xint_max)
            G_inv = G_inv @ translate2d_inv(torch.round(t[:, 0] * width), torch.round(t[:, 1] * height))

        # general geometric transformations (augment.py:224-264)
        if self.scale > 0:
            s = torch.exp2(randn(n) * self.scale_std)
            s = torch.where(rand(n) < self.scale * self.p, s, torch.ones_like(s))
            if debug_percentile is not None:
                s = torch.full_like(s, torch.exp2(torch.erfinv(debug_percentile * 2 - 1) * self.scale_std))
            G_inv = G_inv @ scale2d_inv(s, s)
        p_rot = 1 - torch.sqrt((1 - self.rotate * self.p).clamp(0, 1))      # P(pre OR post) = p
        if self.rotate > 0:
            theta = (rand(n) * 2 - 1) * np.pi * self.rotate_max
            theta = torch.where(rand(n) < p_rot, theta, torch.zeros_like(theta))
            if debug_percentile is not None:
                theta = torch.full_like(theta, (debug_percentile * 2 - 1) * np.pi * self.rotate_max)
            G_inv = G_inv @ rotate2d_inv(-theta)
        if self.aniso > 0:
            s = torch.exp2(randn(n) * self.aniso_std)
            s = torch.where(rand(n) < self.aniso * self.p, s, torch.ones_like(s))
            if debug_percentile is not None:
                s = torch.full_like(s, torch.exp2(torch.erfinv(debug_percentile * 2 - 1) * self.aniso_std))
            G_inv = G_inv @ scale2d_inv(s, 1 / s)
        if self.rotate > 0:
            theta = (rand(n) * 2 - 1) * np.pi * self.rotate_max
            theta = torch.where(rand(n) < p_rot, theta, torch.zeros_like(theta))
            if debug_percentile is not None:
                theta = torch.zeros_like(theta)
            G_inv = G_inv @ rotate2d_inv(-theta)
        if self.xfrac > 0:
            t = randn(n, 2) * self.xfrac_std
            t = torch.where(rand(n, 1) < self.xfrac * self.p, t, torch.zeros_like(t))
            if debug_percentile is not None:
                t = torch.full_like(t, torch.erfinv(debug_percentile * 2 - 1) * self.xfrac_std)
            G_inv = G_inv @ translate2d_inv(t[:, 0] * width, t[:, 1] * height)

        margins = None
        if G_inv is I_3:
            G_inv = None
        else:   # padding of augment.py:273-283, kept on the device
            cx, cy = (width - 1) / 2, (height - 1) / 2
            cp = matrix([-cx, -cy, 1], [cx, -cy, 1], [cx, cy, 1], [-cx, cy, 1], device=device)
            cp = G_inv @ cp.t()
            hz_pad = self.Hz_geom.shape[0] // 4
            margin = cp[:, :2, :].permute(1, 0, 2).flatten(1)
            margin = torch.cat([-margin, margin]).max(dim=1).values
            margin = margin + _constant([hz_pad * 2 - cx, hz_pad * 2 - cy] * 2, device)
            margin = margin.max(_constant([0, 0] * 2, device))
            margin = margin.min(_constant([width - 1, height - 1] * 2, device))
            margins = margin.ceil().to(torch.int32)

        # colour transformations (augment.py:304-350)
        I_4 = torch.eye(4, device=device)
        C = I_4
        if self.brightness > 0:
            b = randn(n) * self.brightness_std
            b = torch.where(rand(n) < self.brightness * self.p, b, torch.zeros_like(b))
            if debug_percentile is not None:
                b = torch.full_like(b, torch.erfinv(debug_percentile * 2 - 1) * self.brightness_std)
            C = translate3d(b, b, b) @ C
        if self.contrast > 0:
            c = torch.exp2(randn(n) * self.contrast_std)
            c = torch.where(rand(n) < self.contrast * self.p, c, torch.ones_like(c))
            if debug_percentile is not None:
                c = torch.full_like(c, torch.exp2(torch.erfinv(debug_percentile * 2 - 1) * self.contrast_std))
            C = scale3d(c, c, c) @ C
        v = _constant(np.asarray([1, 1, 1, 0]) / np.sqrt(3), device)            # luma axis
        if self.lumaflip > 0:
            i = torch.floor(rand(n, 1, 1) * 2)
            i = torch.where(rand(n, 1, 1) < self.lumaflip * self.p, i, torch.zeros_like(i))
            if debug_percentile is not None:
                i = torch.full_like(i, torch.floor(debug_percentile * 2))
            C = (I_4 - 2 * v.ger(v) * i) @ C                                     # Householder reflection
        if self.hue > 0 and num_channels > 1:
            theta = (rand(n) * 2 - 1) * np.pi * self.hue_max
            theta = torch.where(rand(n) < self.hue * self.p, theta, torch.zeros_like(theta))
            if debug_percentile is not None:
                theta = torch.full_like(theta, (debug_percentile * 2 - 1) * np.pi * self.hue_max)
            C = rotate3d(v, theta) @ C                                           # rotate around v
        if self.saturation > 0 and num_channels > 1:
            s = torch.exp2(randn(n, 1, 1) * self.saturation_std)
            s = torch.where(rand(n, 1, 1) < self.saturation * self.p, s, torch.ones_like(s))
            if debug_percentile is not None:
                s = torch.full_like(s, torch.exp2(torch.erfinv(debug_percentile * 2 - 1) * self.saturation_std))
            C = (v.ger(v) + (I_4 - v.ger(v)) * s) @ C
        if C is I_4:
            C = None
        return G_inv, margins, C

    def apply(self, images, params, debug_percentile=None):
        """Run a drawn augmentation (`params` from sample_params) on `images`; the later stages (imgfilter, noise, cutout) are drawn here
        (sample_late), in the reference's order, and run by apply_late."""
        assert isinstance(images, torch.Tensor) and images.ndim == 4
        batch_size, num_channels, height, width = images.shape
        device = images.device
        G_inv, margins, C = params
        if G_inv is not None:
            images = augment_ops.geometric(images, G_inv, margins, self.Hz_geom)
        if C is not None:
            images = augment_ops.color(images, C)

        if self.imgfilter > 0 and images.device.type == 'cuda' and not self.native_late:
            raise NotImplementedError('AugmentPipe: the imgfilter stage runs on the GPU only on the native route (set_native_late(True)); '
                                      'without it use a pipe without imgfilter (e.g. "bgc") on the GPU')
        late = self.sample_late(batch_size, num_channels, height, width, device, debug_percentile=debug_percentile)
        return self.apply_late(images, late)

    def set_native_late(self, native=True):
        """Run the late stages (imgfilter, noise, cutout) of a GPU tensor as one ``pg_augment_late`` launch instead of the torch composition (which has no
        imgfilter on the GPU).  A plain attribute, not a buffer: ``state_dict()`` is unchanged.  CPU tensors are unaffected.  Returns self."""
        self.native_late = bool(native)
        return self

    def sample_late(self, batch_size, num_channels, height, width, device, debug_percentile=None):
        """Draw the late stages in the reference's order (augment.py:372-431): per band randn then rand; the noise's randn, rand and the [N, C, H, W]
        randn; the cutout's rand, rand.  Returns (taps [N, K] or None, noise [N, C, H, W] or None, sigma [N] or None, cut [N, 4] = centre x, centre y,
        size x, size y, or None); None = the stage is off.  Nothing is read to the host."""
        if debug_percentile is not None:
            debug_percentile = torch.as_tensor(debug_percentile, dtype=torch.float32, device=device)
        taps = noise = sigma = cut = None
        if self.imgfilter > 0:   # augment.py:372-395
            num_bands = self.Hz_fbank.shape[0]
            assert len(self.imgfilter_bands) == num_bands
            expected_power = _constant(np.array([10, 1, 1, 1]) / 13, device)
            g = torch.ones([batch_size, num_bands], device=device)
            for i, band_strength in enumerate(self.imgfilter_bands):
                t_i = torch.exp2(torch.randn([batch_size], device=device) * self.imgfilter_std)
                t_i = torch.where(torch.rand([batch_size], device=device) < self.imgfilter * self.p * band_strength, t_i, torch.ones_like(t_i))
                if debug_percentile is not None:
                    t_i = torch.full_like(t_i, torch.exp2(torch.erfinv(debug_percentile * 2 - 1) * self.imgfilter_std)) if band_strength > 0 else torch.ones_like(t_i)
                t = torch.ones([batch_size, num_bands], device=device)
                t[:, i] = t_i
                t = t / (expected_power * t.square()).sum(dim=-1, keepdims=True).sqrt()
                g = g * t
            taps = g @ self.Hz_fbank

        if self.noise > 0:   # augment.py:410-416
            sigma = torch.randn([batch_size, 1, 1, 1], device=device).abs() * self.noise_std
            sigma = torch.where(torch.rand([batch_size, 1, 1, 1], device=device) < self.noise * self.p, sigma, torch.zeros_like(sigma))
            if debug_percentile is not None:
                sigma = torch.full_like(sigma, torch.erfinv(debug_percentile) * self.noise_std)
            sigma = sigma.reshape([batch_size])
            noise = torch.randn([batch_size, num_channels, height, width], device=device)

        if self.cutout > 0:  # augment.py:419-426
            size = torch.full([batch_size, 2, 1, 1, 1], self.cutout_size, device=device)
            size = torch.where(torch.rand([batch_size, 1, 1, 1, 1], device=device) < self.cutout * self.p, size, torch.zeros_like(size))
            center = torch.rand([batch_size, 2, 1, 1, 1], device=device)
            if debug_percentile is not None:
                size = torch.full_like(size, self.cutout_size)
                center = torch.full_like(center, debug_percentile)
            cut = torch.cat([center.reshape([batch_size, 2]), size.reshape([batch_size, 2])], dim=1)
        return taps, noise, sigma, cut

    def apply_late(self, images, late):
        """Run drawn late stages (`late` from sample_late): the filter behind its reflect pad (augment.py:397-404), then the noise, then the cutout.
        A GPU tensor takes ``pg_augment_late`` when ``native_late`` is set, else the torch composition; a CPU tensor always the composition."""
        taps, noise, sigma, cut = late
        if images.device.type == 'cuda' and not self.native_late:
            return augment_ops.late_reference(images, taps, noise, sigma, cut)
        return augment_ops.late(images, taps, noise, sigma, cut)

    def forward(self, images, debug_percentile=None):
        assert isinstance(images, torch.Tensor) and images.ndim == 4
        n, c, h, w = images.shape
        params = self.sample_params(n, h, w, images.device, debug_percentile=debug_percentile, num_channels=c)
        return self.apply(images, params, debug_percentile=debug_percentile)
