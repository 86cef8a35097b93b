"""The VGG19 perceptual term of the reference's G loss (training/loss_fullbody.py:336-386): L1 between the ``relu{1..5}_1`` features of a
generated and a real image, weighted 1/32, 1/16, 1/8, 1/4, 1.

The trunk is torchvision's ``vgg19().features[0:30]``: thirteen 3x3 convolutions with bias and ReLU and four 2x2 max-pools.  The images
enter as they are, in [-1, 1]: the reference applies no ImageNet normalisation.  On a GPU every convolution runs on this package's native
kernels through ``conv2d_gradfix.conv2d`` with ReLU as the fused epilogue, the pools and the feature-space L1 means on
``torch_utils/ops/vgg_ops.py``; on the CPU the same calls are the aten composition.

The weights are BUFFERS of a module that no network owns: they reach no optimizer, EMA, gradient bucket or snapshot.  They come from a
torchvision-format checkpoint (``load_vgg19``; the pretrained ``vgg19-dcbb9e9d.pth`` is not shipped) or, for tests and tools, from
``training.synthetic.vgg19_state_dict``.
"""

import torch

from torch_utils.ops import conv2d_gradfix, conv2d_mfma, vgg_ops

# torchvision's `features` indices of the thirteen convolutions up to relu5_1 with their (Cin, Cout); a tap follows TAPS' convolutions, a pool POOL_BEFORE's
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (16, 256, 256), (19, 256, 512),
         (21, 512, 512), (23, 512, 512), (25, 512, 512), (28, 512, 512))
TAPS = (0, 5, 10, 19, 28)             # relu1_1, relu2_1, relu3_1, relu4_1, relu5_1: the ends of the reference's slices [0:2], [2:7], [7:12], [12:21], [21:30]
POOL_BEFORE = (5, 10, 19, 28)         # features[4], [9], [18], [27]
_RELU = dict(act='relu', gain=1)      # nn.ReLU: bias_act's own default gain for 'relu' is sqrt(2)


def load_vgg19(path):
    """The thirteen (weight, bias) pairs of a torchvision-format VGG19 state dict at `path`, as {key: float32 CPU tensor}; ``features.30+`` and
    ``classifier.*`` are ignored.  KeyError names a missing key, ValueError a mis-shaped one."""
    sd = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f'{path}: expected a state dict, got {type(sd).__name__}')
    out = {}
    for idx, cin, cout in CONVS:
        for leaf, shape in (('weight', (cout, cin, 3, 3)), ('bias', (cout,))):
            key = f'features.{idx}.{leaf}'
            if key not in sd:
                raise KeyError(f'{path}: missing "{key}"')
            t = sd[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError(f'{path}: "{key}" has shape {list(getattr(t, "shape", []))}, expected {list(shape)}')
            out[key] = t.detach().to(torch.float32).contiguous()
    return out


class VGG19Features(torch.nn.Module):
    """`state_dict` = torchvision-format entries (``load_vgg19``'s result or a superset of it).  forward(x) -> [relu1_1, ..., relu5_1].

    `forward_algo` = the launch policy of the FORWARD convolutions on a GPU (``conv2d_mfma.algo``); the input gradients always run under the
    package's own policy (Winograd F(4x4) where it pays).  The default is the direct implicit-GEMM form: every ReLU mask, pool arg-max and
    L1 sign of the backward pass is decided by a forward value, and the Winograd forms' larger rounding error (F(4x4): ~2e-5 of the
    feature scale against ~2e-6 direct) decides enough of them the other way to move dx by 1e-2 of its maximum, against 6e-7 with the direct
    form.  The backward's own rounding is linear in dy and needs no such care.  'auto' trades that for speed."""
    def __init__(self, state_dict, forward_algo='direct'):
        super().__init__()
        self.forward_algo = forward_algo
        for idx, cin, cout in CONVS:
            w, b = state_dict[f'features.{idx}.weight'], state_dict[f'features.{idx}.bias']
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f'features.{idx}: shapes {list(w.shape)} / {list(b.shape)}, expected {[cout, cin, 3, 3]} / {[cout]}')
            self.register_buffer(f'weight{idx}', w.detach().clone().contiguous(), persistent=False)
            self.register_buffer(f'bias{idx}', b.detach().clone().contiguous(), persistent=False)

    def forward(self, x):
        taps = []
        for idx, _, _ in CONVS:
            if idx in POOL_BEFORE:
                x = vgg_ops.maxpool2x2(x)
            with conv2d_mfma.algo(self.forward_algo if x.is_cuda else None):
                x = conv2d_gradfix.conv2d(x, getattr(self, f'weight{idx}'), getattr(self, f'bias{idx}'), padding=1, _epilogue=_RELU)
            if idx in TAPS:
                taps.append(x)
        return taps


class VGGLoss(torch.nn.Module):
    """forward(xs, y): `xs` = a list of G image batches shaped like `y` -> the G scalars  sum_i w_i * mean|f_i(x_g) - f_i(y)|  as a [G] tensor.
    The features of `y` are computed once, without a graph (the reference recomputes them per call and detaches them: the same values); the G
    batches go through the trunk stacked on the batch axis."""
    def __init__(self, features, weights=(1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)):
        super().__init__()
        assert len(weights) == len(TAPS)
        self.features = features
        self.weights = tuple(float(w) for w in weights)

    def forward(self, xs, y):
        if isinstance(xs, torch.Tensor):
            xs = [xs]
        groups = len(xs)
        for x in xs:
            if x.shape != y.shape:
                raise ValueError(f'VGGLoss: every batch of xs must have y\'s shape {list(y.shape)}, got {list(x.shape)}')
        with torch.no_grad():
            fy = self.features(y.detach())
        fx = self.features(xs[0] if groups == 1 else torch.cat(list(xs), dim=0))
        loss = 0
        for w, a, b in zip(self.weights, fx, fy):
            loss = loss + w * vgg_ops.l1_mean(a, b, groups=groups)
        return loss
