"""Softmax cross-entropy over logit rows: the native kernels (``csrc/cross_entropy.hip``)
against the library (``F.cross_entropy`` and its autograd backward), ``mean`` reduction, fp32.

Rows ``(R, V)``: the LM shapes 8192 x 32000, 16384 x 32000, 8192 x 50257 (dword path),
8192 x 50304, 4096 x 128256, the classifier batches 220 x 1000 and 118 x 1000, and 8192 and
1024 rows of 1024 to 16384 columns for the switch-over between the instances.
``forward`` is one call on logits that require a gradient (so the library saves what its
backward needs); ``backward`` is ``torch.autograd.grad`` of that loss, the same host path both
ways.  Rows up to ``--force-up-to`` columns are also timed with each instance forced
(``native_wave``, ``native_workgroup``; forcing costs two more host calls per call, so these
rows compare with each other), and the wide backward past 8192 columns with 4096 and 8192
columns per workgroup (``native_chunk4096``, ``native_chunk8192``): the switch-over width and
the chunk are read off those rows.  ``peak_mib`` is the peak of allocated device memory over
one forward plus backward, above the logits and targets.

The implementations alternate window by window in one process; a window is ``--calls``
back-to-back calls between two device events, each figure the median over ``--windows``
windows with the min-max spread beside it.  ``gbs`` = the bytes the algorithm has to move
(forward ``4RV``, backward ``8RV``) over the time; ``share`` = that over the 6.29 TB/s measured
float4 copy rate.

    python benchmarks/cross_entropy_bench.py --out profiles/r21/cross_entropy/run1.json
"""
import argparse
import json
import os
import statistics
import sys
from typing import Callable, Dict, List

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.gradclip_bench import COPY_RATE, window  # noqa: E402
from torchgpipe_amd.ops import _ext  # noqa: E402
from torchgpipe_amd.ops.loss import _force_instance, _limits, native_cross_entropy  # noqa: E402

SHAPES = ((8192, 32000), (16384, 32000), (8192, 50257), (8192, 50304), (4096, 128256),
          (220, 1000), (118, 1000), (8192, 1024), (8192, 2048), (8192, 4096), (8192, 8192),
          (8192, 16384), (1024, 2048), (1024, 4096), (1024, 8192))
Loss = Callable[[torch.Tensor, torch.Tensor], torch.Tensor]


def forced(wide: int, chunk: int, fn: Callable[[], object]) -> Callable[[], object]:
    def run() -> None:
        _force_instance(wide, chunk)
        try:
            fn()
        finally:
            _force_instance(-1, 0)
    return run


def peak_mib(loss_fn: Loss, x: torch.Tensor, t: torch.Tensor) -> float:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.autograd.grad(loss_fn(x, t), x)
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--force-up-to', type=int, default=32768)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    dev = torch.device('cuda', 0)
    wave_row_max, chunk, dword_chunk = _limits()
    rows: List[Dict[str, object]] = [{'wave_row_max': wave_row_max, 'backward_chunk': chunk,
                                      'backward_dword_chunk': dword_chunk}]
    print(json.dumps(rows[0]), flush=True)
    losses: Dict[str, Loss] = {'library': F.cross_entropy, 'native': native_cross_entropy}
    for r, v in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = (4 * torch.randn(r, v, device=dev, generator=gen) + 30).requires_grad_()
        t = torch.randint(v, (r,), device=dev, generator=gen)
        peaks = {impl: peak_mib(fn, x, t) for impl, fn in losses.items()}
        for pass_name, factor in (('forward', 1), ('backward', 2)):
            impls: Dict[str, Callable[[], object]] = {}
            for impl, fn in losses.items():
                if pass_name == 'forward':
                    impls[impl] = lambda fn=fn: fn(x, t)  # type: ignore[misc]
                else:
                    loss = fn(x, t)
                    impls[impl] = lambda loss=loss: torch.autograd.grad(  # type: ignore[misc]
                        loss, x, retain_graph=True)
            if v <= a.force_up_to:
                impls['native_wave'] = forced(0, 0, impls['native'])
                impls['native_workgroup'] = forced(1, 0, impls['native'])
            if v > 8192 and pass_name == 'backward':
                impls['native_chunk4096'] = forced(-1, 4096, impls['native'])
                impls['native_chunk8192'] = forced(-1, 8192, impls['native'])
            times: Dict[str, List[float]] = {impl: [] for impl in impls}
            for i in range(a.warmup + a.windows):
                for impl, call in impls.items():
                    ms = window(call, a.calls)
                    if i >= a.warmup:
                        times[impl].append(ms)
            lib_ms = statistics.median(times['library'])
            nbytes = factor * 4 * r * v
            for impl, ts in times.items():
                med = statistics.median(ts)
                row = {'R': r, 'V': v, 'pass': pass_name, 'impl': impl,
                       'us': round(med * 1e3, 2), 'us_min': round(min(ts) * 1e3, 2),
                       'us_max': round(max(ts) * 1e3, 2), 'vs_library': round(med / lib_ms, 3),
                       'mbytes': round(nbytes / 1e6, 2),
                       'gbs': round(nbytes / (med * 1e-3) / 1e9, 1),
                       'share': round(nbytes / COPY_RATE / (med * 1e-3), 3),
                       'peak_mib': peaks.get(impl)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del impls
        del x, t
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
