"""Child process of tests/test_head_fold.py (not a test): one forward of the reduced-width SynthesisNetworkFull_v18 (cases.G6_KW, N = 1, the labelled
parsing map given) on cuda:0 under the PG_HEAD_FOLD setting of its environment, run twice.

    python head_fold_worker.py OUT.npz

Writes img / finetune_img / pred_parsing of the first run, whether the second run reproduced them bit for bit, how many times the last style block took
the folded route, and the float64 composition (merge_conv 1x1 -> modulated heads -> bias, clamp, skip image) of that block's heads from the very tensors the
block received -- the anchor both settings are measured against (everything in front of the block is the same computation under both)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, 'pasta-gan-plusplus_amd'), os.path.join(HERE, 'golden'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def heads_f64(block, x, feat, styles, img):
    """merge_conv over [x ; feat], then the block's ToRGB (+ parsing) heads, composed layer by layer in float64."""
    import torch
    mc, tr = block.merge_conv, block.torgb
    d = lambda t: t.detach().double()
    cm = mc.weight.shape[0]
    m = torch.einsum('oc,nchw->nohw', d(mc.weight).reshape(cm, -1) * mc.weight_gain, torch.cat([d(x), d(feat)], 1)) + d(mc.bias)[None, :, None, None]
    cl = float(tr.conv_clamp) if tr.conv_clamp is not None else float('inf')

    def head(w, b):
        return torch.einsum('noc,nchw->nohw', d(w).reshape(1, w.shape[0], cm) * d(styles)[:, None, :], m).add(d(b)[None, :, None, None]).clamp(-cl, cl)
    rgb = head(tr.weight, tr.bias)
    if img is not None:
        rgb = rgb + d(img)
    return rgb, (head(tr.m_weight1, tr.m_bias1) if tr.is_last and tr.is_style else None)


def main():
    import numpy as np
    import torch
    from torch_utils import custom_ops
    custom_ops.verbosity = 'none'
    import cases as C
    from detgen import fill_module_, synthesis_inputs
    from training import networks as PN

    dev = torch.device('cuda', 0)
    net = fill_module_(PN.SynthesisNetworkFull_v18(**C.G6_KW), 'g6.').to(dev).eval()
    inp = synthesis_inputs(1, w_dim=C.G6_KW['w_dim'], num_ws=net.num_ws, feat_ch=C.G6_FEAT_CH, seed_tag='g6', labels=True)
    to = lambda t: t.to(dev) if t is not None else None
    args = (to(inp['ws']), to(inp['pose_feat']), {k: v.to(dev) for k, v in inp['cat_feat'].items()}, to(inp['denorm_upper_input']),
            to(inp['denorm_lower_input']), to(inp['denorm_upper_mask']), to(inp['denorm_lower_mask']), to(inp['gt_parsing']))

    block = net.b512
    seen, folded = [], [0]
    inner_merge, inner_fold = block._merge_heads, block._heads_folded

    def merge_heads(x, feat, w, styles, img, fused_modconv, feat_unused=False):
        seen.append((x, feat, styles, img))
        return inner_merge(x, feat, w, styles, img, fused_modconv, feat_unused=feat_unused)

    def heads_folded(*a):
        r = inner_fold(*a)
        folded[0] += r is not None
        return r
    block._merge_heads, block._heads_folded = merge_heads, heads_folded
    with torch.no_grad():
        first = net(*args, noise_mode='const')
        again = net(*args, noise_mode='const')
        assert len(seen) == 2 and all(t is not None for t in seen[0])
        ref_rgb, ref_pp = heads_f64(block, *seen[0])
    torch.cuda.synchronize()
    names = ('img', 'finetune_img', 'pred_parsing')
    np.savez(sys.argv[1], **{n: t.cpu().numpy() for n, t in zip(names, first)}, ref_img=ref_rgb.cpu().numpy(), ref_pred_parsing=ref_pp.cpu().numpy(),
             repeat_identical=np.array([bool(torch.equal(a, b)) for a, b in zip(first, again)]), folded_calls=np.int64(folded[0]))


if __name__ == '__main__':
    main()
