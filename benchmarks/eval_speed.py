"""Evaluation throughput: ResNet-101 and AmoebaNet-D(18, 256) in ``model.eval()`` under
``torch.no_grad()`` on one GPU, images / s.

    python benchmarks/eval_speed.py --batch 64

Public API only (the model constructors, ``eval()``, a forward), so the same file times any
commit.  Each model is warmed up (code objects, plans, MIOpen's find step), then ``--rounds``
windows of ``--iters`` forwards are each bracketed by device events on the same stream and
closed by a synchronise; the best and the median window are reported, one JSON line in all.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchgpipe_amd.models import amoebanetd  # noqa: E402
from torchgpipe_amd.models.resnet import build_resnet  # noqa: E402

MODELS = {
    'resnet101': lambda: build_resnet([3, 4, 23, 3], num_classes=1000),
    'amoebanetd_18_256': lambda: amoebanetd(num_classes=1000, num_layers=18, num_filters=256),
}


def measure(name: str, batch: int, warmup: int, iters: int, rounds: int) -> dict:
    torch.manual_seed(0)
    device = torch.device('cuda', 0)
    model = MODELS[name]().to(device).eval()
    x = torch.rand(batch, 3, 224, 224, device=device)
    windows = []
    with torch.no_grad():
        for _ in range(warmup):
            out = model(x)
        torch.cuda.synchronize(device)
        for _ in range(rounds):
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                out = model(x)
            stop.record()
            stop.synchronize()
            windows.append(start.elapsed_time(stop) / 1e3)
    assert torch.isfinite(out).all().item()
    rates = [batch * iters / t for t in windows]
    return {'images_per_s': round(max(rates), 2),
            'images_per_s_median': round(statistics.median(rates), 2),
            'window_s': round(min(windows), 4)}


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument('--batch', type=int, default=64, help='images per forward')
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--iters', type=int, default=20, help='forwards per timed window')
    p.add_argument('--rounds', type=int, default=5, help='timed windows')
    p.add_argument('--models', default=','.join(MODELS), help='comma-separated subset')
    p.add_argument('--label', default='', help='free text copied into the result')
    p.add_argument('--conv-precision', choices=['highest', 'high', 'medium'], default='highest',
                   help='fp32 precision of the split-bf16 convolution kernels '
                        '(torchgpipe_amd/ops/precision.py)')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_speed needs a GPU: a CPU run would time nothing of interest')
    result = {'benchmark': 'eval_speed', 'label': args.label, 'batch': args.batch,
              'iters': args.iters, 'rounds': args.rounds,
              'device': torch.cuda.get_device_name(0), 'conv_precision': args.conv_precision}
    if args.conv_precision != 'highest':
        from torchgpipe_amd.ops import precision
        precision.set_conv_precision(args.conv_precision)
    for name in args.models.split(','):
        result[name] = measure(name, args.batch, args.warmup, args.iters, args.rounds)
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
