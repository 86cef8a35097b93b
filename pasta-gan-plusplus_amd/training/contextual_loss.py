"""The contextual term of the reference's loss options (training/loss_fullbody.py:481-618): ``ContextualLoss_forward`` on the features of
``VGG19_feature_color_torchversion``.

The reference constructs both classes with ``contextual_weight > 0`` (:64-73) and never calls them in ``accumulate_gradients``.  What is pinned
here is therefore the reference's own two classes: the op (``torch_utils/ops/contextual_ops.py``) to ``ContextualLoss_forward`` and the trunk
to ``VGG19_feature_color_torchversion``.  The COMBINATION of levels is this package's choice, documented as such: the one
of the code those classes were taken from, CoCosNet's ``get_ctx_loss``:
    8 cx(r52) + 4 cx(r42) + 2 cx(avg_pool2(r32))  [+ 1 cx(avg_pool4(r22)) with use_22],  cx = the batch mean of the per-sample loss.
Nothing is claimed about reproducing a reference training run with it.

The trunk: ``vgg_preprocess`` with ``vgg_normal_correct=True`` ((x + 1) / 2, RGB -> BGR, minus the BGR means, times 255), then fourteen 3x3
convolutions with bias and ReLU up to ``conv5_2`` and four 2x2 max-pools.  On a GPU every convolution runs on this package's native kernels
through ``conv2d_gradfix.conv2d`` with ReLU as the fused epilogue and the pools on ``vgg_ops.maxpool2x2``; on the CPU the same calls are the
aten composition.  The weights are BUFFERS of a module that no network owns: they reach no optimizer, EMA, gradient bucket or snapshot.  They
come from a checkpoint with the reference's key names (``load_vgg19_conv``; ``./checkpoints/vgg19_conv.pth`` is not shipped) or, for tests and
tools, from ``training.synthetic.vgg19_conv_state_dict``.
"""

import torch

from torch_utils.ops import contextual_ops, conv2d_gradfix, conv2d_mfma, vgg_ops

# the fourteen convolutions up to conv5_2 with their (Cin, Cout); a tap follows TAPS' convolutions, a pool precedes POOL_BEFORE's
CONVS = (('conv1_1', 3, 64), ('conv1_2', 64, 64), ('conv2_1', 64, 128), ('conv2_2', 128, 128), ('conv3_1', 128, 256), ('conv3_2', 256, 256),
         ('conv3_3', 256, 256), ('conv3_4', 256, 256), ('conv4_1', 256, 512), ('conv4_2', 512, 512), ('conv4_3', 512, 512), ('conv4_4', 512, 512),
         ('conv5_1', 512, 512), ('conv5_2', 512, 512))
TAPS = {'conv1_2': 'r12', 'conv2_2': 'r22', 'conv3_2': 'r32', 'conv4_2': 'r42', 'conv5_2': 'r52'}
TAP_NAMES = ('r12', 'r22', 'r32', 'r42', 'r52')
POOL_BEFORE = ('conv2_1', 'conv3_1', 'conv4_1', 'conv5_1')
BGR_MEAN = (0.40760392, 0.45795686, 0.48501961)
_RELU = dict(act='relu', gain=1)      # nn.ReLU: bias_act's own default gain for 'relu' is sqrt(2)


def load_vgg19_conv(path):
    """The fourteen (weight, bias) pairs ``conv1_1 ... conv5_2`` of a state dict with the reference's key names at `path`, as {key: float32 CPU
    tensor}; later layers are ignored.  KeyError names a missing key, ValueError a mis-shaped one."""
    sd = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f'{path}: expected a state dict, got {type(sd).__name__}')
    out = {}
    for name, cin, cout in CONVS:
        for leaf, shape in (('weight', (cout, cin, 3, 3)), ('bias', (cout,))):
            key = f'{name}.{leaf}'
            if key not in sd:
                raise KeyError(f'{path}: missing "{key}"')
            t = sd[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError(f'{path}: "{key}" has shape {list(getattr(t, "shape", []))}, expected {list(shape)}')
            out[key] = t.detach().to(torch.float32).contiguous()
    return out


def vgg_preprocess(x):
    """The reference's ``vgg_preprocess(x, vgg_normal_correct=True)``: [-1, 1] RGB -> mean-subtracted BGR in [0, 255] units."""
    x = (x + 1) / 2
    bgr = torch.cat((x[:, 2:3], x[:, 1:2], x[:, 0:1]), dim=1)
    return (bgr - torch.tensor(BGR_MEAN, dtype=bgr.dtype, device=bgr.device).view(1, 3, 1, 1)) * 255


class VGG19ConvFeatures(torch.nn.Module):
    """`state_dict` = entries under the reference's key names (``load_vgg19_conv``'s result or a superset).  forward(x) -> [r12, r22, r32, r42, r52].
    `forward_algo` as in ``vgg_loss.VGG19Features``: the direct form by default, because every ReLU mask, pool arg-max and row arg-min of the
    backward pass is decided by a forward value."""
    def __init__(self, state_dict, forward_algo='direct'):
        super().__init__()
        self.forward_algo = forward_algo
        for name, cin, cout in CONVS:
            w, b = state_dict[f'{name}.weight'], state_dict[f'{name}.bias']
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f'{name}: shapes {list(w.shape)} / {list(b.shape)}, expected {[cout, cin, 3, 3]} / {[cout]}')
            self.register_buffer(f'{name}_weight', w.detach().clone().contiguous(), persistent=False)
            self.register_buffer(f'{name}_bias', b.detach().clone().contiguous(), persistent=False)

    def forward(self, x):
        x = vgg_preprocess(x)
        taps = []
        for name, _, _ in CONVS:
            if name in POOL_BEFORE:
                x = vgg_ops.maxpool2x2(x)
            with conv2d_mfma.algo(self.forward_algo if x.is_cuda else None):
                x = conv2d_gradfix.conv2d(x, getattr(self, f'{name}_weight'), getattr(self, f'{name}_bias'), padding=1, _epilogue=_RELU)
            if name in TAPS:
                taps.append(x)
        return taps


class ContextualLoss(torch.nn.Module):
    """forward(xs, y): `xs` = a list of G image batches shaped like `y` -> [G]: per group
    ``8 mean_n cx(r52) + 4 mean_n cx(r42) + 2 mean_n cx(avg_pool2(r32))`` (``+ 1 mean_n cx(avg_pool4(r22))`` with `use_22`).  The features of `y`
    are computed once, without a graph; the G batches go through the trunk stacked on the batch axis."""
    def __init__(self, features, use_22=False, h=0.1):
        super().__init__()
        self.features = features
        self.use_22 = bool(use_22)
        self.h = float(h)

    def levels(self, taps):
        """(weight, features) of every level of the combination, from the five taps."""
        _, r22, r32, r42, r52 = taps
        out = [(8.0, r52), (4.0, r42), (2.0, torch.nn.functional.avg_pool2d(r32, 2))]
        if self.use_22:
            out.append((1.0, torch.nn.functional.avg_pool2d(r22, 4)))
        return out

    def forward(self, xs, y):
        if isinstance(xs, torch.Tensor):
            xs = [xs]
        groups = len(xs)
        for x in xs:
            if x.shape != y.shape:
                raise ValueError(f'ContextualLoss: every batch of xs must have y\'s shape {list(y.shape)}, got {list(x.shape)}')
        with torch.no_grad():
            fy = self.levels(self.features(y.detach()))
        fx = self.levels(self.features(xs[0] if groups == 1 else torch.cat(list(xs), dim=0)))
        loss = 0
        for (w, a), (_, b) in zip(fx, fy):
            loss = loss + w * contextual_ops.contextual_loss(a, b, h=self.h, groups=groups).reshape(groups, -1).mean(dim=1)
        return loss
