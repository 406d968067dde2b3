"""The three GEMMs of a Linear layer: the native split-bf16 kernels (``csrc/linear.hip``) at
each precision level against the library path ``gradacc._Linear`` takes (``F.linear``,
``dy.matmul(weight)``, ``grad.addmm_(dy.t(), x)``).

Shapes ``(R, I, O)``: VGG-16's three classifier layers at R = 32, 64 and 256 rows, ResNet-101's
2048 -> 1000 at R = 110, and a square 4096^3.  The weight gradient accumulates into an
existing gradient in both versions (beta = 1).

The implementations alternate window by window in one process; a window is ``--calls``
back-to-back calls between two device events, and each figure is the median over
``--windows`` windows with the min-max spread beside it.  Beside the time: the FLOPs
(2 R I O) and the bytes each pass has to move at least (every operand once, the result once,
the accumulated gradient read and written), both from the shapes; ``t_mfma_us`` = the bf16
MFMA products of the level (6 / 3 / 1 per fp32 product) over the 2.5 PFLOP/s dense bf16 rate
of the chip (for the library row: the FLOPs over its 157 TFLOP/s fp32 matrix rate),
``t_bytes_us`` = the bytes over the 6.29 TB/s measured float4 copy rate; ``bound`` names the
larger and ``share`` is it over the time.

    python benchmarks/linear_bench.py --out profiles/r16/linear/linear.json
"""
import argparse
import json
import os
import statistics
import sys
from typing import Callable, Dict, List, Tuple

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.gradclip_bench import COPY_RATE, window  # noqa: E402
from torchgpipe_amd.ops import _ext, precision  # noqa: E402

BF16_RATE = 2.5e15   # dense bf16 MFMA, FLOP/s
F32_RATE = 157.3e12  # fp32 matrix, FLOP/s
PRODUCTS = {'highest': 6, 'high': 3, 'medium': 1}

SHAPES: List[Tuple[str, int, int, int]] = (
    [(f'vgg_fc{i + 1}', r, fan_in, fan_out)
     for i, (fan_in, fan_out) in enumerate([(25088, 4096), (4096, 4096), (4096, 1000)])
     for r in (32, 64, 256)]
    + [('resnet101_fc', 110, 2048, 1000), ('square', 4096, 4096, 4096)])


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=50)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    ops = torch.ops.tgpipe
    dev = torch.device('cuda', 0)
    rows: List[Dict[str, object]] = []
    for name, r, fan_in, fan_out in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(r, fan_in, device=dev, generator=gen)
        w = torch.randn(fan_out, fan_in, device=dev, generator=gen) / fan_in ** 0.5
        b = torch.randn(fan_out, device=dev, generator=gen)
        dy = torch.randn(r, fan_out, device=dev, generator=gen)
        grad = torch.zeros_like(w)
        flops = 2 * r * fan_in * fan_out
        io = 4 * (r * fan_in + fan_out * fan_in + r * fan_out)
        passes: Dict[str, Tuple[int, Callable[[], object], Callable[[], object]]] = {
            'forward': (io + 4 * fan_out, lambda: F.linear(x, w, b),
                        lambda: ops.linear_forward(x, w, b)),
            'backward_data': (io, lambda: dy.matmul(w),
                              lambda: ops.linear_backward_data(dy, w)),
            'weight_grad': (io + 4 * fan_out * fan_in, lambda: grad.addmm_(dy.t(), x),
                            lambda: ops.linear_backward_weight(dy, x, grad, True)),
        }
        for pass_name, (nbytes, lib, native) in passes.items():
            def at(level: str, fn: Callable[[], object] = native) -> Callable[[], object]:
                def run() -> None:
                    with precision.conv_precision(level):
                        for _ in range(a.calls):
                            fn()
                return run

            def lib_run(fn: Callable[[], object] = lib) -> None:
                for _ in range(a.calls):
                    fn()

            impls: Dict[str, Callable[[], object]] = {'library': lib_run}
            impls.update({f'native_{level}': at(level) for level in precision.LEVELS})
            times: Dict[str, List[float]] = {impl: [] for impl in impls}
            for i in range(a.warmup + a.windows):
                for impl, fn in impls.items():
                    grad.zero_()
                    ms = window(fn, 1) / a.calls
                    if i >= a.warmup:
                        times[impl].append(ms)
            lib_ms = statistics.median(times['library'])
            for impl, ts in times.items():
                med = statistics.median(ts)
                t_mfma = (flops / F32_RATE if impl == 'library'
                          else flops * PRODUCTS[impl[len('native_'):]] / BF16_RATE)
                t_bytes = nbytes / COPY_RATE
                row = {'shape': name, 'R': r, 'I': fan_in, 'O': fan_out, 'pass': pass_name,
                       'impl': impl, 'us': round(med * 1e3, 2),
                       'us_min': round(min(ts) * 1e3, 2), 'us_max': round(max(ts) * 1e3, 2),
                       'vs_library': round(med / lib_ms, 3), 'gflop': round(flops / 1e9, 3),
                       'mbytes': round(nbytes / 1e6, 2), 't_mfma_us': round(t_mfma * 1e6, 2),
                       't_bytes_us': round(t_bytes * 1e6, 2),
                       'bound': 'mfma' if t_mfma > t_bytes else 'bytes',
                       'share': round(max(t_mfma, t_bytes) / (med * 1e-3), 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del x, w, b, dy, grad, passes
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
