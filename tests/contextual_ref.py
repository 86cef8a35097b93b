"""Float64 restatement of the contextual loss (the formula of DESIGN section 6o) and of the level combination, written from the formula -- not
from the code under test: the yardstick of test_contextual_cpu.py / test_contextual_gpu.py and of make_golden_contextual.py.  Gradients come
from autograd on these float64 expressions."""

import torch

EPS = 2.220446049250313e-16


def prepare(x, y):
    """x, y [B, C, H, W] (float64) -> xn, yn [B, P, C] and the norms of the centred x [B, P]."""
    b, c = x.shape[0], x.shape[1]
    mu = y.mean(dim=1, keepdim=True)
    xc, yc = (x - mu).reshape(b, c, -1), (y - mu).reshape(b, c, -1)
    rx, ry = xc.pow(2).sum(dim=1).sqrt(), yc.pow(2).sum(dim=1).sqrt()
    return (xc / (rx.unsqueeze(1) + EPS)).permute(0, 2, 1), (yc / (ry.unsqueeze(1) + EPS)).permute(0, 2, 1), rx


def affinity(x, y, h=0.1):
    """d, A [B, P, P] of x, y [B, C, H, W]."""
    xn, yn, _ = prepare(x, y)
    d = 1 - xn @ yn.transpose(1, 2)
    e = d.min(dim=-1, keepdim=True)[0] + 1e-3
    w = torch.exp((1 - d / e) / h)
    return d, w / w.sum(dim=-1, keepdim=True)


def contextual_loss(x, y, h=0.1, groups=1):
    """[G * N] per-sample losses in float64; x [G * N, C, H, W] against y [N, C, H, W] (sample s meets s % N)."""
    x, y = x.double(), y.double().detach()
    if groups > 1:
        y = y.repeat([groups, 1, 1, 1])
    _, a = affinity(x, y, h)
    return -torch.log(a.max(dim=-1)[0].mean(dim=1))


def loss_and_grad(x, y, h=0.1, groups=1, weights=None):
    """(per-sample losses, d(sum_s weights_s loss_s)/dx) in float64; weights default to ones."""
    x = x.detach().double().requires_grad_(True)
    loss = contextual_loss(x, y, h, groups)
    w = torch.ones_like(loss) if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    dx, = torch.autograd.grad((loss * w).sum(), x)
    return loss.detach(), dx


def gaps(x, y, h=0.1):
    """(smallest gap between the two smallest d of a row, smallest relative gap between the two largest A of a row) over all rows and samples
    (inf for P == 1): how far the inputs are from an arg-min / arg-max tie."""
    d, a = affinity(x.double(), y.double(), h)
    if d.shape[-1] < 2:
        return float('inf'), float('inf')
    d2 = d.topk(2, dim=-1, largest=False)[0]
    a2 = a.topk(2, dim=-1, largest=True)[0]
    return float((d2[..., 1] - d2[..., 0]).min()), float(((a2[..., 0] - a2[..., 1]) / a2[..., 0]).min())


TRUNK = ('conv1_1', 'conv1_2', 'P', 'conv2_1', 'conv2_2', 'P', 'conv3_1', 'conv3_2', 'conv3_3', 'conv3_4', 'P', 'conv4_1', 'conv4_2', 'conv4_3',
         'conv4_4', 'P', 'conv5_1', 'conv5_2')
BGR_MEAN = (0.40760392, 0.45795686, 0.48501961)


def trunk_margins(state_dict, x):
    """The float64 trunk up to conv5_2 on images x in [-1, 1]: (the smallest |pre-activation| of a ReLU, the smallest gap between the two largest
    values of a pool window whose maximum is positive), each as a fraction of its layer's largest |value|.  A float32 trunk whose features are
    within that fraction of these decides every ReLU mask and pool arg-max as float64 does; inside it, a gradient differs by a discrete amount."""
    F = torch.nn.functional
    x = (x.double() + 1) / 2
    x = (torch.cat((x[:, 2:3], x[:, 1:2], x[:, 0:1]), dim=1) - torch.tensor(BGR_MEAN, dtype=torch.float64).view(1, 3, 1, 1)) * 255
    relu_margin, pool_margin = float('inf'), float('inf')
    for name in TRUNK:
        if name == 'P':
            win = F.unfold(x.reshape(-1, 1, *x.shape[2:]), 2, stride=2)          # [planes, 4, windows]
            top = win.topk(2, dim=1)[0]
            live = top[:, 0] > 0
            if bool(live.any()):
                pool_margin = min(pool_margin, float((top[:, 0] - top[:, 1])[live].min() / x.abs().max()))
            x = F.max_pool2d(x, 2, 2)
        else:
            pre = F.conv2d(x, state_dict[f'{name}.weight'].double(), state_dict[f'{name}.bias'].double(), padding=1)
            relu_margin = min(relu_margin, float(pre.abs().min() / pre.abs().max()))
            x = pre.relu()
    return relu_margin, pool_margin


def combine(taps_x, taps_y, groups=1, use_22=False, h=0.1):
    """[G]: 8 mean_n cx(r52) + 4 mean_n cx(r42) + 2 mean_n cx(avg_pool2(r32)) (+ 1 mean_n cx(avg_pool4(r22))) from the five taps r12 ... r52."""
    pool = torch.nn.functional.avg_pool2d
    levels = [(8.0, taps_x[4], taps_y[4]), (4.0, taps_x[3], taps_y[3]), (2.0, pool(taps_x[2].double(), 2), pool(taps_y[2].double(), 2))]
    if use_22:
        levels.append((1.0, pool(taps_x[1].double(), 4), pool(taps_y[1].double(), 4)))
    return sum(w * contextual_loss(a, b, h, groups).reshape(groups, -1).mean(dim=1) for w, a, b in levels)
