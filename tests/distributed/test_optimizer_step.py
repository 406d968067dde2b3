"""``PipelineStage.optimizer_step`` over gloo CPU ranks: the clip fused into the native
optimizers' update uses the whole pipeline's norm, so the ranks' parameters afterwards are
those of the unpartitioned model after ``clip_grad_norm_`` + ``step()``."""
import pytest
import torch
from torch import nn
import torch.nn.functional as F

from tests.distributed.mp_util import run

CHUNKS = 2
X = torch.randn(6, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
T = torch.randn(6, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
LR = 0.0625  # exact in the fp32 LR tensor

# (world, balance); the last leaves rank 1 with parameterless layers only
CASES = {'two': (2, [2, 4]), 'bare_rank': (3, [1, 2, 3])}
RUNS = [('two', 'sgd'), ('two', 'rmsprop'), ('two', 'torch_sgd'), ('bare_rank', 'sgd')]


def build():
    torch.manual_seed(4321)
    model = nn.Sequential(nn.Linear(4, 8), nn.Tanh(), nn.Tanh(), nn.Linear(8, 8), nn.Tanh(),
                          nn.Linear(8, 2)).double()
    with torch.no_grad():  # unequal partition norms: the last layer's gradients dominate
        model[5].weight.mul_(3.0)
    return model


def optimizer(kind, params):
    from torchgpipe_amd import optim
    if kind == 'sgd':
        return optim.SGD(params, lr=LR, momentum=0.9, weight_decay=1e-4)
    if kind == 'rmsprop':
        return optim.RMSprop(params, lr=LR, centered=True, momentum=0.9)
    return torch.optim.SGD(params, lr=LR, momentum=0.9, weight_decay=1e-4)


def torch_optimizer(kind, params):
    if kind == 'rmsprop':
        return torch.optim.RMSprop(params, lr=LR, centered=True, momentum=0.9, foreach=False)
    return torch.optim.SGD(params, lr=LR, momentum=0.9, weight_decay=1e-4, foreach=False)


def reference(kind, scale):
    """The whole model in one process: (norm, parameters after the clipped step)."""
    model = build()
    for x, t in zip(X.chunk(CHUNKS), T.chunk(CHUNKS)):
        (F.mse_loss(model(x), t) * (x.size(0) / X.size(0))).backward()
    norm = float(torch.nn.utils.clip_grad_norm_(model.parameters(), float('inf')))
    torch.nn.utils.clip_grad_norm_(model.parameters(), scale * norm)
    torch_optimizer(kind, list(model.parameters())).step()
    return norm, [p.detach().clone() for p in model.parameters()]


def _worker(rank, world, balance, kind, bound):
    from torchgpipe_amd.parallel import PipelineStage
    stage = PipelineStage(build(), balance, chunks=CHUNKS, checkpoint='never')
    stage.train_step(X if rank == 0 else None, T if rank == world - 1 else None, F.mse_loss)
    params = list(stage.parameters())
    before = [p.grad.clone() for p in params]
    opt = optimizer(kind, params) if params else None
    norm = stage.optimizer_step(opt, bound)
    return {'norm': norm, 'params': [p.detach().clone() for p in params],
            'unscaled': all(torch.equal(p.grad, b) for p, b in zip(params, before))}


def _close(a, b, rel=1e-12):
    return float((a - b).abs().max()) <= rel * float(b.abs().max())


@pytest.mark.parametrize('case,kind', RUNS)
def test_parameters_match_the_clipped_step_of_the_whole_model(case, kind, tmp_path):
    world, balance = CASES[case]
    want_norm, want = reference(kind, 0.5)
    results = run(_worker, world, tmp_path, balance, kind, 0.5 * want_norm)
    norms = [r['norm'] for r in results]
    assert all(n.dtype == torch.float64 and n.dim() == 0 for n in norms)
    assert all(float(n) == float(norms[0]) for n in norms), norms
    assert abs(float(norms[0]) - want_norm) <= 1e-12 * want_norm
    got = [p for r in results for p in r['params']]
    assert len(got) == len(want)
    assert all(_close(a, b) for a, b in zip(got, want))
    initial = list(build().parameters())
    assert not any(torch.equal(a, b) for a, b in zip(got, initial))
    # the native optimizers leave .grad unscaled; torch's path clipped it in place
    assert all(r['unscaled'] == (kind != 'torch_sgd') for r in results if r['params'])
    if case == 'bare_rank':  # the rank without parameters took part
        assert results[1]['params'] == []
        assert float(results[1]['norm']) == float(results[0]['norm']) > 0
