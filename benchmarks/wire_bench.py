"""The bf16 wire format's two kernels (``ops.misc.pack_wire`` / ``unpack_wire``,
csrc/wire.hip) on one fp32 message of 1 MB, 16 MB and 283 MB (the U-Net pipeline-2 skip
of one micro-batch), against what they replace or compete with:

* ``encode``   fp32 -> bf16 wire buffer, one launch (reads 4 B, writes 2 B per element)
* ``decode``   wire buffer -> fp32 tensor, one launch (reads 2 B, writes 4 B per element)
* ``copy``     ``copy_segments`` of the same element count as fp32 (reads 4 B, writes 4 B):
               the pack pass an fp32 multi-tensor message pays today
* ``to+pack``  ``t.to(torch.bfloat16)`` followed by ``pack``: the two-pass route through
               torch (reads 4 B, writes 2 B, reads 2 B, writes 2 B per element)

``gb_s`` is the bytes each route has to move (as listed) over its time.  The routes
alternate window by window in one process; a window is ``calls`` back-to-back calls between
two device events, sized to a few tens of milliseconds, over a ring of source / destination
buffers larger than the 256 MiB Infinity Cache, so no call finds its data cached by the
one before.  Each figure is the median over ``--windows`` windows, the min-max beside it.
``link_ms`` columns are arithmetic, not measurements: the time the message's bytes take on
one link at the given rate, fp32 and bf16.

    python benchmarks/wire_bench.py --out profiles/r13/wire/wire_bench.json
"""
import argparse
import json
import os
import statistics
import sys
from typing import Callable, Dict, List

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchgpipe_amd.ops import _ext, misc  # noqa: E402

SIZES = {'1MB': 1 << 20, '16MB': 16 << 20, '283MB': 283_115_520}  # fp32 bytes
LINKS = (64e9, 50e9)  # bytes/s of one link: the README's two rates
CACHE = 256 << 20


def window(fn: Callable[[int], object], calls: int) -> float:
    """Milliseconds per call over ``calls`` back-to-back calls."""
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(calls):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--sizes', default=','.join(SIZES))
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--window-ms', type=float, default=40.0,
                   help='device time one window is sized to')
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    dev = torch.device('cuda', 0)
    bf16 = torch.bfloat16
    rows: List[Dict[str, object]] = []
    for name in a.sizes.split(','):
        nbytes = SIZES[name]
        n = nbytes // 4
        # a ring of buffers whose fp32 sides alone exceed twice the cache
        ring = max(2, -(-2 * CACHE // nbytes))
        gen = torch.Generator(device=dev).manual_seed(0)
        src = [torch.randn(n, device=dev, generator=gen) for _ in range(ring)]
        dst = [torch.empty(n, device=dev) for _ in range(ring)]
        wire = [torch.empty(misc.wire_nbytes([src[0]], bf16), dtype=torch.uint8, device=dev)
                for _ in range(ring)]
        flat = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(ring)]
        for k in range(ring):
            misc.pack_wire([src[k]], wire[k], bf16)
        routes: Dict[str, Callable[[int], object]] = {
            'encode': lambda k: misc.pack_wire([src[k % ring]], wire[k % ring], bf16),
            'decode': lambda k: misc.unpack_wire(wire[k % ring], [dst[k % ring]], bf16),
            'copy': lambda k: misc.pack([src[k % ring]], flat[k % ring]),
            'to+pack': lambda k: misc.pack([src[k % ring].to(bf16)], wire[k % ring]),
        }
        moved = {'encode': 6 * n, 'decode': 6 * n, 'copy': 8 * n, 'to+pack': 10 * n}
        calls = {}
        for route, fn in routes.items():  # warm up, and size the windows
            window(fn, 3)
            calls[route] = max(5, int(a.window_ms / window(fn, 5)))
        times: Dict[str, List[float]] = {route: [] for route in routes}
        for _ in range(a.windows):
            for route, fn in routes.items():
                times[route].append(window(fn, calls[route]))
        # the encode's bytes are the torch route's bytes
        check = torch.empty_like(wire[0])
        misc.pack([src[0].to(bf16)], check)
        misc.pack_wire([src[0]], wire[0], bf16)
        assert torch.equal(check, wire[0])
        for route in routes:
            ms = statistics.median(times[route])
            row = {'size': name, 'elements': n, 'route': route, 'calls': calls[route],
                   'ring': ring, 'ms': round(ms, 5), 'ms_min': round(min(times[route]), 5),
                   'ms_max': round(max(times[route]), 5),
                   'gb_s': round(moved[route] / ms / 1e6, 1)}
            for rate in LINKS:
                tag = f'link{int(rate / 1e9)}'
                row[f'{tag}_fp32_ms'] = round(nbytes / rate * 1e3, 4)
                row[f'{tag}_bf16_ms'] = round(nbytes / 2 / rate * 1e3, 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del src, dst, wire, flat, routes
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            # (the measurement's parameters; where the file lies is not one)
            args = {k: v for k, v in vars(a).items() if k != 'out'}
            json.dump({'args': args, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
