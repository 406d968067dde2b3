"""U-Net(5,64) pipeline-1 (B = 80, two micro-batches, one GPU) at the three conv precision
levels, the levels interleaved over ``--rounds`` rounds: samples/s per (round, level), and
the accuracy row of U-Net: the loss and the parameter gradients of one more step against
the same step of the same round at 'highest' (same seed, same dropout stream; relative
error of the loss, median and worst relative error of the gradients -- reported, not
asserted; benchmarks/precision_accuracy.py compares its models with fp64 eager twins,
which the U-Net's Philox dropout does not have).

    python benchmarks/unet_precision_speed.py --rounds 2 \\
        --out profiles/r11/f4_emu/unet_levels.json

``--autocast`` adds a ``bf16-autocast`` run to every round: the same stage at 'highest'
with every ``train_step`` under ``torch.autocast('cuda', dtype=torch.bfloat16)`` (library
bf16 convolutions between the bf16 DropNormAct / pool / upsample kernels), with the same
error report against the round's 'highest'.

The level is set before the stage is built (checkpoint recomputation must see the forward's
level), so every (round, level) builds its own stage from the same seed.
"""
import argparse
import contextlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchgpipe_amd.models import unet  # noqa: E402
from torchgpipe_amd.ops import _ext, precision  # noqa: E402
from torchgpipe_amd.parallel import PipelineStage  # noqa: E402


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


AUTOCAST = 'bf16-autocast'


def run(level: str, batch: int, chunks: int, steps: int, warmup: int, ref: dict) -> dict:
    amp = level == AUTOCAST
    precision.set_conv_precision('highest' if amp else level)
    device = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = unet(depth=5, num_convs=5, base_channels=64, input_channels=3, output_channels=1)
    stage = PipelineStage(model, [len(model)], device=device, chunks=chunks,
                          checkpoint='except_last')
    x = torch.rand(batch, 3, 192, 192, device=device)
    target = torch.ones(batch, 1, 192, 192, device=device)
    loss = None
    plain_step = stage.train_step

    def train_step(*args):  # type: ignore[no-untyped-def]
        with torch.autocast('cuda', dtype=torch.bfloat16) if amp else contextlib.nullcontext():
            return plain_step(*args)

    stage.train_step = train_step  # type: ignore[method-assign]
    for _ in range(warmup):
        loss = stage.train_step(x, target, F.binary_cross_entropy_with_logits)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = stage.train_step(x, target, F.binary_cross_entropy_with_logits)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {'level': level, 'step_ms': round(dt * 1e3, 2), 'samples_per_s': round(batch / dt, 2)}
    for q in stage.parameters():
        q.grad = None
    loss = stage.train_step(x, target, F.binary_cross_entropy_with_logits)
    torch.cuda.synchronize()
    grads = [q.grad.detach().clone() for q in stage.parameters()]
    out['loss'] = loss.item()
    if 'grads' not in ref:  # the round's first run: 'highest'
        ref['loss'], ref['grads'] = loss.item(), grads
    else:
        errs = sorted(rel_err(g, r) for g, r in zip(grads, ref['grads']))
        out['loss_rel_err_vs_highest'] = abs(loss.item() - ref['loss']) / abs(ref['loss'])
        out['grad_rel_err_median_vs_highest'] = errs[len(errs) // 2]
        out['grad_rel_err_worst_vs_highest'] = errs[-1]
    del stage, model
    torch.cuda.empty_cache()
    return out


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=2)
    p.add_argument('--steps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--batch', type=int, default=80)
    p.add_argument('--chunks', type=int, default=2)
    p.add_argument('--levels', nargs='+', default=list(precision.LEVELS),
                   help="the levels of a round, 'highest' first (a second 'highest' shows "
                        "what two runs of one level differ by)")
    p.add_argument('--exact-fused', action='store_true',
                   help='keep the fused F(4x4) layers on the exact kernels at every level '
                        '(what the reduced levels did before variant 24)')
    p.add_argument('--autocast', action='store_true',
                   help="add a 'bf16-autocast' run (torch.autocast around every step, conv "
                        "level 'highest') to every round")
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if not _ext.available():
        raise RuntimeError(f'HIP extension not loadable: {_ext.load_error()!r}')
    if a.exact_fused:
        from torchgpipe_amd.ops import conv
        conv.f4_emu_faster = lambda shape, out_channels: False
    rows = []
    try:
        for rnd in range(a.rounds):
            ref: dict = {}
            for level in list(a.levels) + ([AUTOCAST] if a.autocast else []):
                row = dict(run(level, a.batch, a.chunks, a.steps, a.warmup, ref), round=rnd)
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        precision.set_conv_precision('highest')
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        json.dump(rows, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
