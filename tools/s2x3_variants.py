"""Dev tool: build (here) and time (GPU box) variants of csrc/conv2d_s2x3.h compiled with -DSX_EXP=<mask> (1 no MFMAs, 2 no operand split, 4 no halo loads,
8 no weight loads, 16 no output stores; results wrong by design), and print the cycle stamps of the variant built with 32 (per round the cycles of the multiplying
waves in operand reads + MFMAs and at the barrier, per tile in the epilogue).    SX_VARIANTS=0,1,6,16,32 python tools/s2x3_variants.py build|run"""
import math
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pasta-gan-plusplus_amd'))
from torch_utils import custom_ops
custom_ops.verbosity = 'none'
VARIANTS = os.environ.get('SX_VARIANTS', '0,1,6,16,32').split(',')


def flags_of(v):
    return [f'-DSX_EXP={int(v)}']


def name_of(v):
    return 'sx_exp' + v


SRC = custom_ops.PLUGIN_SOURCES['conv2d_plugin']
for v in VARIANTS:
    custom_ops.get_plugin(name_of(v), sources=SRC, extra_hipcc_flags=flags_of(v), build_only=True)
if sys.argv[1] == 'build':
    sys.exit(0)
import torch
from torch_utils.ops import conv2d_mfma
torch.set_grad_enabled(False)
libs = {}
for v in VARIANTS:
    conv2d_mfma._plugin = None
    custom_ops.PLUGIN_SOURCES[name_of(v)] = SRC
    _orig = custom_ops.get_plugin
    custom_ops.get_plugin = lambda name, _v=v, **kw: _orig(name, extra_hipcc_flags=flags_of(_v), abi_name='conv2d_plugin', **kw)
    libs[v] = conv2d_mfma._init(name_of(v))
    custom_ops.get_plugin = _orig
for (N, cin, cout, H) in [(8, 64, 128, 513), (8, 128, 256, 257)]:
    x = torch.randn(N, cin, H, H, device='cuda')
    w = torch.randn(cout, cin, 3, 3, device='cuda') / (3 * cin ** 0.5)
    b = torch.randn(cout, device='cuda')
    ep = dict(bias=b, act='lrelu', alpha=0.2, gain=math.sqrt(2), clamp=256.0)
    times = {v: [] for v in VARIANTS}
    packs, last = {}, {}
    for v in VARIANTS:
        conv2d_mfma._plugin = libs[v]
        conv2d_mfma._x3_planes.clear()
        packs[v] = conv2d_mfma.pack_weight(w)
        conv2d_mfma.pack_x3('s2', packs[v], cout, cin)
    for r in range(6):
        for v in VARIANTS:
            conv2d_mfma._plugin = libs[v]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(4):
                last[v] = conv2d_mfma.conv2d_forward(x, packs[v], cout, 3, 3, stride=2, **ep)
            e1.record(); torch.cuda.synchronize()
            if r > 0:
                times[v].append(e0.elapsed_time(e1) / 4 * 1e3)
    print(f'N{N} {cin}->{cout} {H}^2: ' + '  '.join(f'[{v}] {statistics.median(times[v]):6.1f}us' for v in VARIANTS), flush=True)
    if '32' in VARIANTS:
        raw = last['32'].flatten()[:32].contiguous().view(torch.int64).cpu()
        for wv in range(4):
            mm, bar, epi, rounds = (int(t) for t in raw[wv * 4: wv * 4 + 4])
            tiles = max(1, rounds // (cin // 16))
            print(f'  wave {wv}: {rounds} rounds, {tiles} tiles: operand reads + MFMAs {mm / max(rounds, 1):8.0f} cycles per round, barrier wait {bar / max(rounds, 1):8.0f} per round, epilogue {epi / tiles:8.0f} per tile')
