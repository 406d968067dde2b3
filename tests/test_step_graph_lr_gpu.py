"""An LR schedule under ``StepGraph``: the native optimizers' learning rate is a device
tensor the captured update kernel reads, so ``StepLR`` takes effect between replays."""
import copy

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd import optim
from torchgpipe_amd.ops import _ext
from torchgpipe_amd.parallel import PipelineStage, StepGraph

pytestmark = pytest.mark.gpu

cuda = torch.device('cuda', 0)
LR, CLIP, WARMUP, STEPS = 0.1, 0.05, 2, 6  # warm-up, the capture and three replays


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


def _conv_stack() -> nn.Sequential:
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(),
                         nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(), nn.Conv2d(16, 2, 1))


def _batches():
    gen = torch.Generator().manual_seed(1)
    return [(torch.randn(4, 3, 16, 16, generator=gen).to(cuda),
             torch.randn(4, 2, 16, 16, generator=gen).to(cuda)) for _ in range(STEPS)]


def _stage(base):
    model = copy.deepcopy(base)
    return PipelineStage(model, [len(model)], device=cuda, chunks=2, checkpoint='except_last')


def _graphed(base, batches, scheduled):
    stage = _stage(base)
    opt = optim.SGD(stage.parameters(), lr=LR, momentum=0.9, weight_decay=1e-4)
    lr = opt.param_groups[0]['lr']
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    graph = StepGraph(stage, F.mse_loss, opt, warmup=WARMUP, max_grad_norm=CLIP)
    for x, y in batches:
        graph.step(x, y)
        if scheduled:
            sched.step()
    torch.cuda.synchronize()
    assert graph.captured and opt.param_groups[0]['lr'] is lr
    assert float(lr) == float(torch.tensor(LR)) * (0.5 ** STEPS if scheduled else 1.0)
    return [p.detach().clone() for p in stage.parameters()]


def _eager(base, batches):
    """The twin: torch.optim.SGD given the same LR sequence, and the stage's clip."""
    stage = _stage(base)
    opt = torch.optim.SGD(stage.parameters(), lr=LR, momentum=0.9, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for x, y in batches:
        opt.zero_grad(set_to_none=True)
        stage.train_step(x, y, F.mse_loss)
        norm = stage.clip_grad_norm_(CLIP)
        assert float(norm) > CLIP  # every step clips
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    return [p.detach().clone() for p in stage.parameters()]


def test_lr_schedule_takes_effect_between_replays():
    base, batches = _conv_stack(), _batches()
    scheduled = _graphed(base, batches, True)
    constant = _graphed(base, batches, False)
    eager = _eager(base, batches)
    for got, want, const in zip(scheduled, eager, constant):
        scale = want.abs().max().item() + 1e-12
        # test_step_graph.py's graph-against-eager tolerance
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5 * scale)
        # a kernel that ignored the LR tensor would give the constant-LR result: that one is
        # off by far more than the tolerance (77 to 1800 times it, per tensor, on the CPU)
        gap = (const - want).abs().max().item()
        assert gap > 20 * (1e-4 * scale + 1e-5 * scale), (gap, scale)


def test_torch_sgd_with_a_changed_float_lr_still_raises():
    base, batches = _conv_stack(), _batches()
    stage = _stage(base)
    opt = torch.optim.SGD(stage.parameters(), lr=LR, momentum=0.9)
    graph = StepGraph(stage, F.mse_loss, opt, warmup=1, max_grad_norm=CLIP)
    for x, y in batches[:3]:
        graph.step(x, y)
    assert graph.captured
    opt.param_groups[0]['lr'] = LR / 2
    with pytest.raises(RuntimeError, match='hyperparameters changed'):
        graph.step(*batches[3])
    torch.cuda.synchronize()


def test_native_optimizers_other_hyperparameters_are_still_checked():
    base, batches = _conv_stack(), _batches()
    stage = _stage(base)
    opt = optim.SGD(stage.parameters(), lr=LR, momentum=0.9)
    graph = StepGraph(stage, F.mse_loss, opt, warmup=1)
    for x, y in batches[:3]:
        graph.step(x, y)
    opt.param_groups[0]['momentum'] = 0.5
    with pytest.raises(RuntimeError, match='torchgpipe_amd.optim'):
        graph.step(*batches[3])
    torch.cuda.synchronize()
