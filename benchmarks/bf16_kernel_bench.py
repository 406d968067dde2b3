"""bf16 against fp32 instances of the U-Net epilogue and resampling kernels, per kernel, at
the shapes of U-Net(5,64) with micro-batches of 40: DropNormAct forward / backward,
MaxPool2x2 forward / backward, up2x_cat forward / backward.

Each figure is the median of ``--iters`` event-timed launches after ``--warmup`` untimed
ones, the two dtypes alternating shape by shape; ``gb_s`` counts the bytes the kernel has to
move (reads + writes of its operands), so the two dtypes can be compared with the HBM rate.
Each timed call allocates its output, and repeats on the same buffers: operands that fit
the 256 MB Infinity Cache (the bf16 ones at every level, the fp32 ones from 96^2 down) can
be served from it, so a bf16 / fp32 ratio at 192^2 also compares cached with uncached.

    python benchmarks/bf16_kernel_bench.py --out profiles/r12/amp/kernels.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchgpipe_amd.ops import _ext  # noqa: E402

# (channels, plane side) of the encoder levels and the bottleneck at 192^2 input
LEVELS = [(64, 192), (128, 96), (256, 48), (512, 24), (1024, 12), (1024, 6)]


def timed(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--images', type=int, default=40)
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    ops = torch.ops.tgpipe
    dev = torch.device('cuda', 0)
    rows = []
    for c, side in LEVELS:
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn(a.images, c, side, side, device=dev).to(dtype)
            dy = torch.randn_like(x)
            size = x.numel() * x.element_size()
            y, mean, rstd, scale = ops.dna_forward(x, 0.1, 1e-5, 1e-2, 1, 2, True, None)
            cases = [('dna_forward', 2 * size,
                      lambda: ops.dna_forward(x, 0.1, 1e-5, 1e-2, 1, 2, True, None)),
                     ('dna_backward', 3 * size,
                      lambda: ops.dna_backward(dy, x, mean, rstd, scale, 1e-2))]
            if side % 2 == 0 and side > 6:
                pooled = ops.maxpool2x2_forward(x, None)
                dp = torch.randn_like(pooled)
                half = x[:, :c // 2].contiguous()
                small = pooled[:, :c // 2].contiguous()   # (dense: no copy inside the op)
                cat = ops.up2x_cat_forward(small, half)
                dcat = torch.randn_like(cat)
                cases += [
                    ('maxpool2x2_forward', size + size // 4,
                     lambda: ops.maxpool2x2_forward(x, None)),
                    ('maxpool2x2_backward', 2 * size + size // 4,
                     lambda: ops.maxpool2x2_backward(x, dp)),
                    ('up2x_cat_forward', size // 8 + size // 2 + size,
                     lambda: ops.up2x_cat_forward(small, half)),
                    ('up2x_backward', size // 2 + size // 8,
                     lambda: ops.up2x_backward(dcat, c // 2)),
                ]
            for name, nbytes, fn in cases:
                us = timed(fn, a.warmup, a.iters)
                row = {'kernel': name, 'dtype': str(dtype).replace('torch.', ''),
                       'shape': [a.images, c, side, side], 'us': round(us, 1),
                       'gb_s': round(nbytes / us / 1e3, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del x, dy, y, cases
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        json.dump(rows, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
