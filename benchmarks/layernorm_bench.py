"""LayerNorm / RMSNorm over the last dimension: the native kernels (``csrc/layernorm.hip``)
against the library (``F.layer_norm`` / ``F.rms_norm`` and their autograd backward).

Rows ``B*T`` in {4096, 16384, 65536} by widths ``N`` in {768, 1024, 2048, 4096, 8192}, fp32,
with weight (and, for LayerNorm, bias); 65536 x 8192 is 2 GiB per tensor, past what the native
ops take, and is left out.  ``forward`` is one call; ``backward`` is everything a training step
pays after it: for the library the autograd backward (``dx``, ``dweight``, ``dbias``) plus the
two adds of ``AccumulateGrad`` into existing gradients, for the native op the one call that
adds into the gradients itself.  The two do not share a host path: the library row goes
through ``torch.autograd.grad`` in Python, the ``native`` row is the bare op.  The
``native_autograd`` row closes that gap: the native kernels behind the same
``torch.autograd.grad`` call and the same two adds (no fused accumulation), so at the small
shapes, where the host is the limit, compare ``library`` with ``native_autograd``.  Up to the
widest row of the wave-per-row instance's registers
(2048) both instances are timed, forced through ``_force_instance``: the switch-over width is
read off those rows.

The implementations alternate window by window in one process; a window is ``--calls``
back-to-back calls between two device events, each figure the median over ``--windows``
windows with the min-max spread beside it.  ``gbs`` = the bytes the pass has to move at least
(forward: x and y; backward: dy, x and dx) over the time; ``share`` = that over the 6.29 TB/s
measured float4 copy rate.

    python benchmarks/layernorm_bench.py --out profiles/r20/layernorm/layernorm.json
"""
import argparse
import json
import os
import statistics
import sys
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.gradclip_bench import COPY_RATE, window  # noqa: E402
from torchgpipe_amd.ops import _ext  # noqa: E402
from torchgpipe_amd.ops.layernorm import (MAX_WIDTH, _force_instance, eligible,  # noqa: E402
                                          native_layer_norm, native_rms_norm)

ROWS = (4096, 16384, 65536)
WIDTHS = (768, 1024, 2048, 4096, MAX_WIDTH)
FORCE_UP_TO = 2048  # the wave-per-row instance has registers for rows up to here
EPS = 1e-5


def forced(wide: int, fn: Callable[[], object]) -> Callable[[], object]:
    def run() -> None:
        _force_instance(wide)
        try:
            fn()
        finally:
            _force_instance(-1)
    return run


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    ops = torch.ops.tgpipe
    dev = torch.device('cuda', 0)
    rows: List[Dict[str, object]] = []
    for r in ROWS:
        for n in WIDTHS:
            gen = torch.Generator(device=dev).manual_seed(0)
            x = torch.randn(r, n, device=dev, generator=gen).requires_grad_()
            if not eligible(x, (n,)):
                continue
            w = (1 + 0.1 * torch.randn(n, device=dev, generator=gen)).requires_grad_()
            b = (0.1 * torch.randn(n, device=dev, generator=gen)).requires_grad_()
            dy = torch.randn(r, n, device=dev, generator=gen)
            gw, gb = torch.zeros_like(w), torch.zeros_like(b)
            xd, wd, bd = x.detach(), w.detach(), b.detach()
            for rms in (False, True):
                bias: Optional[torch.Tensor] = None if rms else bd
                y = (F.rms_norm(x, (n,), w, EPS) if rms else F.layer_norm(x, (n,), w, b, EPS))
                _, mean, rstd = ops.layernorm_forward(xd, wd, bias, EPS, rms)

                def lib_forward(rms: bool = rms) -> None:
                    if rms:
                        F.rms_norm(xd, (n,), wd, EPS)
                    else:
                        F.layer_norm(xd, (n,), wd, bd, EPS)

                def lib_backward(rms: bool = rms, y: torch.Tensor = y) -> None:
                    if rms:
                        _, dw = torch.autograd.grad(y, [x, w], dy, retain_graph=True)
                        gw.add_(dw)
                    else:
                        _, dw, db = torch.autograd.grad(y, [x, w, b], dy, retain_graph=True)
                        gw.add_(dw)
                        gb.add_(db)

                def native_forward(rms: bool = rms, bias: Optional[torch.Tensor] = bias) -> None:
                    ops.layernorm_forward(xd, wd, bias, EPS, rms)

                def native_backward(rms: bool = rms, mean: torch.Tensor = mean,
                                    rstd: torch.Tensor = rstd) -> None:
                    ops.layernorm_backward(dy, xd, mean, rstd, wd, gw, None if rms else gb,
                                           True, True, rms)

                yn = (native_rms_norm(x, w, EPS) if rms else native_layer_norm(x, w, b, EPS))

                def native_autograd(rms: bool = rms, y: torch.Tensor = yn) -> None:
                    lib_backward(rms, y)  # the library's host path around the native kernels

                passes = {'forward': (2, lib_forward, native_forward),
                          'backward': (3, lib_backward, native_backward)}
                for pass_name, (tensors, lib, native) in passes.items():
                    impls: Dict[str, Callable[[], object]] = {'library': lib, 'native': native}
                    if pass_name == 'backward':
                        impls['native_autograd'] = native_autograd
                    if n <= FORCE_UP_TO:
                        impls['native_wave'] = forced(0, native)
                        impls['native_workgroup'] = forced(1, native)
                    times: Dict[str, List[float]] = {impl: [] for impl in impls}
                    for i in range(a.warmup + a.windows):
                        for impl, fn in impls.items():
                            ms = window(fn, a.calls)
                            if i >= a.warmup:
                                times[impl].append(ms)
                    lib_ms = statistics.median(times['library'])
                    nbytes = tensors * 4 * r * n
                    for impl, ts in times.items():
                        med = statistics.median(ts)
                        row = {'op': 'rmsnorm' if rms else 'layernorm', 'R': r, 'N': n,
                               'pass': pass_name, 'impl': impl, 'us': round(med * 1e3, 2),
                               'us_min': round(min(ts) * 1e3, 2),
                               'us_max': round(max(ts) * 1e3, 2),
                               'vs_library': round(med / lib_ms, 3),
                               'mbytes': round(nbytes / 1e6, 2),
                               'gbs': round(nbytes / (med * 1e-3) / 1e9, 1),
                               'share': round(nbytes / COPY_RATE / (med * 1e-3), 3)}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                del y, yn, mean, rstd
            del x, w, b, dy, gw, gb, xd, wd, bd
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
