"""Clip-then-step: the native optimizers with the clip fused into the update
(``grad_sumsq`` + ``torchgpipe_amd.optim`` ``step(grad_sumsq=, max_norm=)``) against
``ops.gradclip.clip_grad_norm_`` + ``torch.optim`` (foreach; for SGD also ``fused=True``) on
the parameter lists of U-Net(5,64) and ResNet-101 -- random tensors of the parameters'
shapes, no training.

Configurations: SGD with momentum 0.9 and weight decay 1e-4, RMSprop plain, and RMSprop
centred with momentum 0.9.  The clip is active in every call (``max_norm`` below the norm).
The implementations alternate window by window in one process; a window is ``--calls``
back-to-back calls between two device events, and each figure is the median over
``--windows`` windows with the min-max spread beside it.  ``gb_s`` is the bytes the native
path has to move (one read of the gradients for the sum of squares, then one read of the
gradient and one read and one write of the parameter and of each state tensor) over the time,
``share`` that rate over the 6.29 TB/s float4 copy rate of the chip; the other rows use the
same byte counts so that all can be compared directly.

    python benchmarks/optim_bench.py --out profiles/r14/optim/optim.json
"""
import argparse
import json
import os
import statistics
import sys
from typing import Callable, Dict, List, Tuple

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.gradclip_bench import COPY_RATE, shapes, window  # noqa: E402
from torchgpipe_amd import optim  # noqa: E402
from torchgpipe_amd.ops import _ext, gradclip  # noqa: E402

LR = 1e-3
# name -> (kind, keyword arguments, state tensors per parameter)
CONFIGS: Dict[str, Tuple[str, Dict[str, object], int]] = {
    'sgd_momentum_wd': ('sgd', {'momentum': 0.9, 'weight_decay': 1e-4}, 1),
    'rmsprop': ('rmsprop', {}, 1),
    'rmsprop_centered_momentum': ('rmsprop', {'centered': True, 'momentum': 0.9}, 3),
}


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--models', default='unet,resnet101')
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--windows', type=int, default=9)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    dev = torch.device('cuda', 0)
    rows: List[Dict[str, object]] = []
    for name in a.models.split(','):
        gen = torch.Generator(device=dev).manual_seed(0)
        source = [torch.randn(s, device=dev, generator=gen) for s in shapes(name)]
        numel = sum(g.numel() for g in source)
        norm = float(gradclip.grad_sumsq(source).sqrt())
        bound = 0.5 * norm
        for config, (kind, kwargs, states) in CONFIGS.items():
            nbytes = 4 * numel * (1 + 1 + 2 * (1 + states))

            def fresh() -> List[nn.Parameter]:
                params = [nn.Parameter(torch.randn_like(g)) for g in source]
                for q, g in zip(params, source):
                    q.grad = g.clone()
                return params

            impls: Dict[str, Callable[[], None]] = {}
            restores: Dict[str, Callable[[], None]] = {}
            state = {'bound': bound}

            def add_native() -> None:
                params = fresh()
                cls = optim.SGD if kind == 'sgd' else optim.RMSprop
                opt = cls(params, lr=LR, **kwargs)
                grads = [q.grad for q in params]

                def step() -> None:  # .grad stays unscaled: the bound stays active
                    opt.step(grad_sumsq=gradclip.grad_sumsq(grads), max_norm=bound)

                impls['native_fused_clip'] = step
                restores['native_fused_clip'] = lambda: None

            def add_torch(label: str, **extra: object) -> None:
                params = fresh()
                cls = torch.optim.SGD if kind == 'sgd' else torch.optim.RMSprop
                opt = cls(params, lr=LR, **kwargs, **extra)

                def step() -> None:
                    # an active bound must stay active over a window: the clip shrinks the
                    # gradients in place, so the bound follows them
                    gradclip.clip_grad_norm_(params, state['bound'])
                    state['bound'] *= 0.8
                    opt.step()

                def restore() -> None:
                    torch._foreach_copy_([q.grad for q in params], source)
                    state['bound'] = bound

                impls[label] = step
                restores[label] = restore

            add_native()
            add_torch('clip_torch_foreach', foreach=True)
            if kind == 'sgd':
                add_torch('clip_torch_fused', fused=True)

            times: Dict[str, List[float]] = {impl: [] for impl in impls}
            for i in range(a.warmup + a.windows):
                for impl, fn in impls.items():
                    restores[impl]()
                    ms = window(fn, a.calls)
                    if i >= a.warmup:
                        times[impl].append(ms)
            for impl, ts in times.items():
                med = statistics.median(ts)
                row = {'model': name, 'tensors': len(source), 'elements': numel,
                       'config': config, 'impl': impl, 'ms': round(med, 4),
                       'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4),
                       'window_ms': round(med * a.calls, 2), 'bytes': nbytes,
                       'gb_s': round(nbytes / med / 1e6, 1),
                       'share': round(nbytes / (med * 1e-3) / COPY_RATE, 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del impls, restores
            torch.cuda.empty_cache()
        del source
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
