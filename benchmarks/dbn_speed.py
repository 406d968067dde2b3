"""Training throughput with ``deferred_batch_norm`` off and on: ResNet-101 pipeline-1 and
AmoebaNet-D(18, 256) n1m32 as ``bench.py`` runs them on one GPU, samples / s.

    python benchmarks/dbn_speed.py --steps 5 --rounds 3

Public API only (the model constructors, ``PipelineStage`` and its ``train_step``, SGD), so
the same file times any commit.  Every row builds its stage from seed 0, runs ``--warmup``
steps (code objects, plans, MIOpen's find step, the cell captures), then ``--rounds`` windows
of ``--steps`` SGD steps, each window between two device synchronisations; the best and the
median window are reported, one JSON line per row.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchgpipe_amd.models import amoebanetd, resnet101  # noqa: E402
from torchgpipe_amd.models.amoebanet import set_cell_streams  # noqa: E402
from torchgpipe_amd.parallel import PipelineStage  # noqa: E402

# bench.py's one-GPU rows: batch, micro-batches, balance, checkpoint mode and the engine
# switches it turns on for each model (recompute / forward lanes for ResNet-101; cell
# streams and captured cells for AmoebaNet-D)
CONFIGS = {
    'resnet101_p1': dict(build=lambda: resnet101(num_classes=1000), batch=220, chunks=2,
                         balance=[370], checkpoint='except_last',
                         stage=dict(overlap_recompute=True, overlap_forward=True)),
    'amoebanetd_18_256_n1m32': dict(
        build=lambda: amoebanetd(num_classes=1000, num_layers=18, num_filters=256), batch=640,
        chunks=32, balance=[24], checkpoint='except_last', cell_streams=True,
        stage=dict(graph_cells=True)),
}


def measure(name: str, deferred: bool, warmup: int, steps: int, rounds: int,
            forward_lanes: bool = True) -> dict:
    cfg = CONFIGS[name]
    engine = dict(cfg['stage'])
    if not forward_lanes:  # (what a partition with deferred BatchNorms runs with anyway)
        engine.pop('overlap_forward', None)
    device = torch.device('cuda', 0)
    torch.manual_seed(0)
    stage = PipelineStage(cfg['build'](), cfg['balance'], device=device, chunks=cfg['chunks'],
                          checkpoint=cfg['checkpoint'], deferred_batch_norm=deferred,
                          **engine)
    if cfg.get('cell_streams'):
        set_cell_streams(stage.partition, True)
    optimizer = torch.optim.SGD(list(stage.parameters()), lr=0.1)
    x = torch.rand(cfg['batch'], 3, 224, 224, device=device)
    target = torch.randint(1000, (cfg['batch'],), device=device)

    def step() -> torch.Tensor:
        loss = stage.train_step(x, target, F.cross_entropy)
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        return loss

    for _ in range(warmup):
        loss = step()
    windows = []
    for _ in range(rounds):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize(device)
        windows.append(time.perf_counter() - t0)
    assert torch.isfinite(loss).item()
    rates = [cfg['batch'] * steps / t for t in windows]
    return {'samples_per_s': round(max(rates), 2),
            'samples_per_s_median': round(statistics.median(rates), 2),
            'window_s': round(min(windows), 4)}


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--steps', type=int, default=5, help='SGD steps per timed window')
    p.add_argument('--rounds', type=int, default=3, help='timed windows')
    p.add_argument('--models', default=','.join(CONFIGS), help='comma-separated subset')
    p.add_argument('--deferred', default='off,on', help="'off', 'on' or 'off,on'")
    p.add_argument('--forward-lanes', default='on', choices=['on', 'off'],
                   help="'off': no forward lanes for ResNet-101 with the option off either")
    p.add_argument('--label', default='', help='free text copied into every row')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dbn_speed needs a GPU: a CPU run would time nothing of interest')
    for name in args.models.split(','):
        for mode in args.deferred.split(','):
            row = {'benchmark': 'dbn_speed', 'label': args.label, 'model': name,
                   'deferred_batch_norm': mode == 'on', 'batch': CONFIGS[name]['batch'],
                   'chunks': CONFIGS[name]['chunks'], 'steps': args.steps,
                   'rounds': args.rounds, 'forward_lanes': args.forward_lanes,
                   'device': torch.cuda.get_device_name(0)}
            try:
                row.update(measure(name, mode == 'on', args.warmup, args.steps, args.rounds,
                                   args.forward_lanes == 'on'))
            except Exception as exc:  # (a commit on which the configuration does not run)
                row['error'] = f'{type(exc).__name__}: {exc}'
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
