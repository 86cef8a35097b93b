"""GPU box: the stride-2 3x3 convolution after the FIR pass of a `down = 2` layer -- conv2d_s2x3 (bf16 pipe, three-term split, csrc/conv2d_s2x3.h) against
conv2d_mfma<3,3,2> (fp32 MFMA), alternating in one process: per round one timing of each (4 launches between two events), error against float64 on one image.
A shape belongs to the policy (conv2d_mfma.s2x3_wanted) only where EVERY timing of the new kernel is below EVERY timing of the fp32 kernel of the same run.
    python tools/s2x3_probe.py [out.txt]      (default profiles/s2x3_probe.txt)"""
import math
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))
import torch
from torch_utils import custom_ops
custom_ops.verbosity = 'none'
from torch_utils.ops import conv2d_mfma

SHAPES = [(8, 64, 128, 513), (8, 128, 256, 257)]      # (N, Cin, Cout, H = W): the config-2 layer and config 3's encoder layer
ROUNDS, REPS = 8, 4


def main(out_path):
    lines = ['# tools/s2x3_probe.py on ' + torch.cuda.get_device_name(0) + f': {ROUNDS} alternating rounds, {REPS} launches per timing, us per launch; bias + lrelu + gain + clamp in the epilogue']
    torch.set_grad_enabled(False)
    for n, cin, cout, h in SHAPES:
        x = torch.randn(n, cin, h, h, device='cuda')
        w = torch.randn(cout, cin, 3, 3, device='cuda') / (3 * math.sqrt(cin))
        b = torch.randn(cout, device='cuda')
        packed = conv2d_mfma.pack_weight(w)
        ep = dict(bias=b, act='lrelu', alpha=0.2, gain=math.sqrt(2), clamp=256.0)

        def run(new):
            os.environ['PG_S2_X3'] = '1' if new else '0'
            return conv2d_mfma.conv2d_forward(x, packed, cout, 3, 3, stride=2, **ep)
        tl = conv2d_mfma.start_timeline()
        y_new, y_old = run(True), run(False)
        conv2d_mfma.stop_timeline()
        assert tl[0][0][4].endswith(' s2x3') and ' s2x3' not in tl[1][0][4], [t[0] for t in tl]
        ts = {True: [], False: []}
        for r in range(ROUNDS + 1):
            for new in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    run(new)
                e1.record()
                torch.cuda.synchronize()
                if r:                                   # (round 0 warms both up)
                    ts[new].append(e0.elapsed_time(e1) / REPS * 1e3)
        pre = torch.nn.functional.conv2d(x[:1].double(), w.double(), stride=2) + b.double()[None, :, None, None]
        ref = (torch.where(pre > 0, pre, pre * 0.2) * math.sqrt(2)).clamp(-256, 256)
        sc = float(ref.abs().max())
        e_new, e_old = float((y_new[:1].double() - ref).abs().max()), float((y_old[:1].double() - ref).abs().max())
        oh = (h - 3) // 2 + 1
        fl = 2.0 * n * cout * oh * oh * cin * 9
        faster = max(ts[True]) < min(ts[False])
        lines.append(f'N{n} {cin}->{cout} {h}^2')
        lines.append('  s2x3 ' + ' '.join(f'{t:7.1f}' for t in ts[True]) + f'   min {min(ts[True]):.1f} max {max(ts[True]):.1f}  ({fl / min(ts[True]) / 1e6:.1f} fp32-equivalent TFLOP/s)')
        lines.append('  fp32 ' + ' '.join(f'{t:7.1f}' for t in ts[False]) + f'   min {min(ts[False]):.1f} max {max(ts[False]):.1f}  ({fl / min(ts[False]) / 1e6:.1f} TFLOP/s)')
        lines.append(f'  every s2x3 timing below every fp32 timing: {faster}   error / scale vs float64: s2x3 {e_new / sc:.2e}, fp32 {e_old / sc:.2e}')
        print('\n'.join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 's2x3_probe.txt'))
