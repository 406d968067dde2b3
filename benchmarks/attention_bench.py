"""Fused fp32 attention (``csrc/attention.hip``, ``csrc/attention128.hip``) at each precision
level against ``F.scaled_dot_product_attention`` on the same fp32 tensors, forward and
backward.

Grid: ``B * H`` in {16, 96} (B = 1), ``T`` in {512, 2048, 8192}, head dim 64 or, with
``--head-dim 128``, 128, causal and not.
Both implementations get the same contiguous ``[1, H, T, D]`` inputs in one process and
alternate window by window; a window is ``calls`` back-to-back calls between two device events
(20 / 5 / 1 calls by ``T``), each figure the median over ``--windows`` windows with the
min-max spread beside it.  The library's forward runs with autograd recording, as in
training (it keeps its ``T x T`` tensors for the backward).  The backward rows time the
backward alone: the native ``attention_backward`` op on the forward's saved ``o`` and
``lse``, the library's autograd over a retained graph.  ``peak_mb`` is the allocator's peak
over one forward plus backward, above what the inputs hold.  ``t_mfma_us`` = the pass's GEMM
units (2 forward, 7 native backward -- 8 at head dim 128, where dV and dK are two kernels --,
5 library backward; half of each when causal) times the
level's bf16 products over the 2.5 PFLOP/s dense bf16 rate (library: over its 157 TFLOP/s
fp32 matrix rate); ``share`` is it over the time.

    python benchmarks/attention_bench.py --out profiles/r17/attention/attention.json
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
from benchmarks.gradclip_bench import window  # noqa: E402
from benchmarks.linear_bench import BF16_RATE, F32_RATE, PRODUCTS  # noqa: E402
from torchgpipe_amd.ops import _ext, precision  # noqa: E402
from torchgpipe_amd.ops.attention import native_attention  # noqa: E402

CALLS = {512: 20, 2048: 5, 8192: 1}


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--heads', default='16,96')
    p.add_argument('--lengths', default='512,2048,8192')
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--head-dim', type=int, default=64, choices=(64, 128))
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    ops = torch.ops.tgpipe
    d, scale = a.head_dim, a.head_dim ** -0.5
    dev = torch.device('cuda', 0)
    rows: List[Dict[str, object]] = []
    for h in map(int, a.heads.split(',')):
        for t in map(int, a.lengths.split(',')):
            gen = torch.Generator(device=dev).manual_seed(0)
            q, k, v, do = (torch.randn(1, h, t, d, device=dev, generator=gen) for _ in range(4))
            leaves = [x.requires_grad_() for x in (q, k, v)]
            calls = CALLS.get(t, 1)
            for causal in (False, True):
                def peak(fn: Callable[[], torch.Tensor]) -> float:
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    torch.autograd.grad(fn(), leaves, do)
                    torch.cuda.synchronize()
                    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

                def lib_fwd() -> torch.Tensor:
                    return F.scaled_dot_product_attention(q, k, v, is_causal=causal)

                impls: Dict[str, Dict[str, Callable[[], object]]] = {}
                peaks = {'library': peak(lib_fwd)}
                out = lib_fwd()
                impls['library'] = {
                    'forward': lib_fwd,
                    'backward': lambda out=out: torch.autograd.grad(out, leaves, do,
                                                                    retain_graph=True)}
                for level in precision.LEVELS:
                    def at(fn: Callable[[], object], level: str = level) -> Callable[[], object]:
                        def run() -> None:
                            with precision.conv_precision(level):
                                fn()
                        return run
                    with precision.conv_precision(level):
                        peaks[f'native_{level}'] = peak(lambda: native_attention(q, k, v, causal))
                        o, lse = ops.attention_forward(q.detach(), k.detach(), v.detach(), causal,
                                                       scale)
                    impls[f'native_{level}'] = {
                        'forward': at(lambda: ops.attention_forward(q.detach(), k.detach(),
                                                                    v.detach(), causal, scale)),
                        'backward': at(lambda o=o, lse=lse: ops.attention_backward(
                            do, q.detach(), k.detach(), v.detach(), o, lse, causal, scale))}
                for pass_name in ('forward', 'backward'):
                    times: Dict[str, List[float]] = {impl: [] for impl in impls}
                    for i in range(a.warmup + a.windows):
                        for impl, fns in impls.items():
                            ms = window(fns[pass_name], calls)
                            if i >= a.warmup:
                                times[impl].append(ms)
                    lib_ms = statistics.median(times['library'])
                    unit = 2 * h * t * t * d * (0.5 if causal else 1.0)  # FLOPs of one GEMM
                    for impl, ts in times.items():
                        med = statistics.median(ts)
                        native = impl != 'library'
                        bwd_units = (7 if d == 64 else 8) if native else 5
                        units = 2 if pass_name == 'forward' else bwd_units
                        t_mfma = (units * unit * PRODUCTS[impl[len('native_'):]] / BF16_RATE
                                  if native else units * unit / F32_RATE)
                        row = {'BH': h, 'T': t, 'causal': causal, 'pass': pass_name, 'impl': impl,
                               'us': round(med * 1e3, 1), 'us_min': round(min(ts) * 1e3, 1),
                               'us_max': round(max(ts) * 1e3, 1),
                               'vs_library': round(med / lib_ms, 3),
                               'peak_mb': round(peaks[impl], 1),
                               't_mfma_us': round(t_mfma * 1e6, 1),
                               'share': round(t_mfma / (med * 1e-3), 3)}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                del impls, out, o, lse
            del q, k, v, do, leaves
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('[\n' + ',\n'.join(json.dumps(r) for r in rows) + '\n]\n')


if __name__ == '__main__':
    main()
