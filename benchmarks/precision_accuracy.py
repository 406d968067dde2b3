"""Loss and gradient error of one training step at each conv precision level.

The tiny ResNet-50 and AmoebaNet-D(3, 64) of the model tests run one training step at
``highest``, ``high`` and ``medium`` (``torchgpipe_amd/ops/precision.py``) and are compared
with an fp64 eager copy of the same model: the relative error of the loss, and the median
and the worst relative error of the parameter gradients.  One JSON line per (model, level).

    python benchmarks/precision_accuracy.py --out profiles/r10/precision/accuracy.json
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def models():
    from torchgpipe_amd.models import amoebanetd
    from torchgpipe_amd.models.resnet import build_resnet
    # (name, the model, its eager twin for the fp64 copy, input, batch)
    yield ('resnet50_96px', lambda: build_resnet([3, 4, 6, 3], num_classes=10, fused=True),
           lambda: build_resnet([3, 4, 6, 3], num_classes=10, fused=False),
           lambda: torch.randn(16, 3, 96, 96, device='cuda'), 16)
    make = lambda: amoebanetd(num_classes=10, num_layers=3, num_filters=64)  # noqa: E731
    yield ('amoebanetd_3_64', make, make, lambda: torch.rand(8, 3, 224, 224, device='cuda'), 8)


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument('--out', default='')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('precision_accuracy needs a GPU')
    from torchgpipe_amd.ops import convbn, precision
    rows = []
    for name, build, build_eager, make_x, batch in models():
        torch.manual_seed(0)
        base = build().cuda()
        x = make_x()
        t = torch.randint(10, (batch,), device='cuda')
        ref = build_eager().cuda()
        ref.load_state_dict(base.state_dict())
        ref = ref.double()
        with convbn.disabled():
            loss64 = F.cross_entropy(ref(x.double()), t)
            loss64.backward()
        for level in precision.LEVELS:
            model = copy.deepcopy(base)
            with precision.conv_precision(level):
                loss = F.cross_entropy(model(x), t)
                loss.backward()
            errs = [rel_err(p.grad, r.grad) for p, r in zip(model.parameters(), ref.parameters())]
            row = {'model': name, 'conv_precision': level,
                   'loss_rel_err': abs(loss.item() - loss64.item()) / abs(loss64.item()),
                   'grad_rel_err_median': statistics.median(errs),
                   'grad_rel_err_worst': max(errs)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
