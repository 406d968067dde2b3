"""Global-norm gradient clipping: ``ops.gradclip.clip_grad_norm_`` (native kernels) against
``torch.nn.utils.clip_grad_norm_(foreach=True)`` on the gradient lists of U-Net(5,64) and
ResNet-101 -- random tensors of the parameters' shapes, no training.

Two cases per model: the clip active (``max_norm`` half the norm: one read pass and one
rewrite, 12 B per fp32 element) and inactive (twice the norm: the native path only reads,
4 B per element; torch multiplies by 1.0 all the same).  The two implementations alternate
window by window in one process; a window is ``--calls`` back-to-back calls between two
device events (sized well above a few milliseconds), and each figure is the median over
``--windows`` windows with the min-max spread beside it.  ``gb_s`` is the bytes the native
path has to move over the time, ``share`` that rate over the 6.29 TB/s float4 copy rate of
the chip; torch's rows use the same byte counts so the two can be compared directly.

    python benchmarks/gradclip_bench.py --out profiles/r12/gradclip/gradclip.json
"""
import argparse
import json
import os
import statistics
import sys
from typing import Callable, Dict, List

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchgpipe_amd.ops import _ext, gradclip  # noqa: E402

COPY_RATE = 6.29e12  # measured float4 copy, bytes/s


def shapes(name: str) -> List[torch.Size]:
    with torch.device('meta'):
        if name == 'unet':
            from torchgpipe_amd.models import unet
            model = unet(depth=5, num_convs=5, base_channels=64, input_channels=3,
                         output_channels=1)
        else:
            from torchgpipe_amd.models import resnet101
            model = resnet101(num_classes=1000)
    return [p.shape for p in model.parameters()]


def window(fn: Callable[[], object], calls: int) -> float:
    """Milliseconds per call over ``calls`` back-to-back calls."""
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--models', default='unet,resnet101')
    p.add_argument('--dtype', default='float32', choices=['float32', 'bfloat16'])
    p.add_argument('--calls', type=int, default=50)
    p.add_argument('--windows', type=int, default=9)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    dev = torch.device('cuda', 0)
    dtype = getattr(torch, a.dtype)
    rows: List[Dict[str, object]] = []
    for name in a.models.split(','):
        gen = torch.Generator(device=dev).manual_seed(0)
        source = [torch.randn(s, device=dev, generator=gen).to(dtype) for s in shapes(name)]
        numel = sum(g.numel() for g in source)
        norm = float(gradclip.grad_sumsq(source).sqrt())
        params = [nn.Parameter(torch.empty_like(g)) for g in source]
        for q, g in zip(params, source):
            q.grad = g.clone()
        esize = source[0].element_size()
        for case, bound, nbytes in (('active', 0.5 * norm, 3 * esize * numel),
                                    ('inactive', 2.0 * norm, esize * numel)):
            def restore() -> None:  # an active clip shrinks the gradients: start alike
                torch._foreach_copy_([q.grad for q in params], source)

            # an active bound must stay active over a window: clip towards a norm that
            # every call undershoots by the same factor (the bound follows the gradients)
            state = {'bound': bound}

            def native() -> None:
                gradclip.clip_grad_norm_(params, state['bound'])
                if case == 'active':
                    state['bound'] *= 0.8

            def foreach() -> None:
                torch.nn.utils.clip_grad_norm_(params, state['bound'], foreach=True)
                if case == 'active':
                    state['bound'] *= 0.8

            times: Dict[str, List[float]] = {'native': [], 'torch_foreach': []}
            for i in range(a.warmup + a.windows):
                for impl, fn in (('native', native), ('torch_foreach', foreach)):
                    restore()
                    state['bound'] = bound
                    ms = window(fn, a.calls)
                    if i >= a.warmup:
                        times[impl].append(ms)
            for impl, ts in times.items():
                med = statistics.median(ts)
                row = {'model': name, 'dtype': a.dtype, 'tensors': len(source),
                       'elements': numel, 'case': case, 'impl': impl,
                       'ms': round(med, 4), 'ms_min': round(min(ts), 4),
                       'ms_max': round(max(ts), 4), 'window_ms': round(med * a.calls, 2),
                       'gb_s': round(nbytes / med / 1e6, 1),
                       'share': round(nbytes / (med * 1e-3) / COPY_RATE, 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del source, params
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
