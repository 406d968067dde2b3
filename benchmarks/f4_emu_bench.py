"""Time the fused split-bf16 F(4x4) kernel (variant 24) against the exact fused variant that
``ops.conv.f4_variant`` picks at 'highest' for the same shape, interleaved.

    python benchmarks/f4_emu_bench.py --repeats 5 --out profiles/r11/f4_emu/per_shape.json

Shapes: the fused layers of U-Net(5,64) at micro-batch 40 (forward and backward-data: the
channel pair swapped) and ResNet's 64 / 128-channel 3x3s at 22 and 110 images.  Per shape:
median and (min, max) of each arm, whether 24's median beats the exact kernel's by more than
the spread of the exact kernel's own repetitions, the distance of the two results (the
levels are ~3e-5 apart) and whether two runs of 24 gave the same bits.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.wino_variants import UNET_SHAPES  # noqa: E402
from torchgpipe_amd.ops import _ext, conv  # noqa: E402

RESNET_SHAPES = [(n, c, c, h) for n in (22, 110) for c, h in ((64, 56), (128, 28))]
EMU = conv.F4_EMU_VARIANT


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--splits', type=int, nargs='+', default=[0],
                   help='split-K counts of variant 24 to time (0: the planner picks)')
    p.add_argument('--shape', type=int, nargs=4, action='append', default=None,
                   help='N C K H (repeatable; default: the U-Net and ResNet tables)')
    p.add_argument('--out', default=None)
    a = p.parse_args()
    ops = _ext.require()
    shapes = a.shape or [s for s in UNET_SHAPES + RESNET_SHAPES if s[2] < 512]
    rows = []
    for n, c, k, h in shapes:
        exact = conv.f4_variant((n, c, h, h), k, 'highest')
        torch.manual_seed(0)
        x = torch.randn(n, c, h, h, device='cuda')
        w = torch.randn(k, c, 3, 3, device='cuda') / (3 * c ** 0.5)
        images = {exact: ops.wino4_weight(w, False), EMU: ops.wino4_weight_emu(w, False)}
        arms = [(exact, 0)] + [(EMU, sp) for sp in a.splits]
        times = {arm: [] for arm in arms}
        for v, sp in arms:
            for _ in range(3):
                ops.wino4_conv(x, images[v], None, k, v, sp)
        for _ in range(a.repeats):
            for v, sp in arms:
                s, e = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                s.record()
                for _ in range(a.iters):
                    ops.wino4_conv(x, images[v], None, k, v, sp)
                e.record()
                e.synchronize()
                times[v, sp].append(s.elapsed_time(e) / a.iters)
        y_exact = ops.wino4_conv(x, images[exact], None, k, exact, 0)
        row = {'shape': [n, c, k, h], 'exact': exact}
        for (v, sp), ts in times.items():
            ts.sort()
            entry = {'ms': round(ts[len(ts) // 2], 4), 'min': round(ts[0], 4),
                     'max': round(ts[-1], 4),
                     'splits': ops.wino4_plan_info(n, c, k, h, h, v, sp)[2]}
            if v == EMU:
                y = ops.wino4_conv(x, images[v], None, k, v, sp)
                again = ops.wino4_conv(x, images[v], None, k, v, sp)
                entry['vs_exact'] = ((y.double() - y_exact.double()).norm()
                                     / y_exact.double().norm()).item()
                entry['same_bits_twice'] = bool(torch.equal(y, again))
            row[f'v{v}' + (f's{sp}' if sp else '')] = entry
        base, emu = row[f'v{exact}'], row[f'v{EMU}' + (f's{a.splits[0]}' if a.splits[0] else '')]
        row['speedup'] = round(base['ms'] / emu['ms'], 3)
        row['qualifies'] = bool(base['ms'] - emu['ms'] > base['max'] - base['min'])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        json.dump(rows, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
