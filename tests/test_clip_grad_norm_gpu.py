"""Global-norm gradient clipping through the public classes on a GPU: ``PipelineStage``,
``StepGraph(max_grad_norm=...)``, ``GPipe`` and two ranks sharing ``cuda:0`` over gloo."""
import copy
import time

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from tests.distributed import parity
from tests.distributed.mp_util import run
from torchgpipe_amd import GPipe
from torchgpipe_amd.ops import _ext, misc
from torchgpipe_amd.parallel import PipelineStage, StepGraph

pytestmark = pytest.mark.gpu

cuda = torch.device('cuda', 0)


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


def _conv_model() -> nn.Sequential:
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(),
                         nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 2, 1))


def _mlp() -> nn.Sequential:
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 16), nn.Tanh(),
                         nn.Linear(16, 4))


def _torch_clip(params, c):
    """torch's clip on clones of the gradients: (norm, clipped gradients)."""
    clones = [nn.Parameter(torch.zeros_like(p)) for p in params]
    for q, p in zip(clones, params):
        q.grad = p.grad.clone()
    norm = torch.nn.utils.clip_grad_norm_(clones, c)
    return norm, [q.grad for q in clones]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _conv_stage():
    model = _conv_model()
    stage = PipelineStage(model, [len(model)], device=cuda, chunks=2, checkpoint='except_last')
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 16, 16, generator=gen).to(cuda)
    t = torch.randn(4, 2, 16, 16, generator=gen).to(cuda)
    stage.train_step(x, t, F.mse_loss)
    return stage


def test_stage_clip_matches_torch():
    stage = _conv_stage()
    params = list(stage.parameters())
    only = stage.grad_norm()
    want_norm, _ = _torch_clip(params, 1.0)
    assert abs(float(only) - float(want_norm)) <= 1e-5 * float(want_norm)
    c = 0.5 * float(want_norm)
    want_norm, want = _torch_clip(params, c)
    norm = stage.clip_grad_norm_(c)
    assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.device == cuda
    assert abs(float(norm) - float(want_norm)) <= 1e-5 * float(want_norm)
    for p, w in zip(params, want):
        assert _rel(p.grad, w) <= 1e-5


def test_stage_clip_does_not_wait_on_the_host():
    stage = _conv_stage()
    stage.clip_grad_norm_(1e9)  # warm: extension, allocator, kernels loaded
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    misc.spin(0.2, cuda)
    done.record()
    start = time.perf_counter()
    stage.clip_grad_norm_(1e-3)
    elapsed = time.perf_counter() - start
    still_spinning = not done.query()
    torch.cuda.synchronize()
    assert still_spinning, 'the spin kernel ended before the call returned'
    assert elapsed < 0.1, elapsed


def _train(mode, c, steps=5):
    """Five SGD steps of the MLP: 'graph' (StepGraph clips), 'stage' (eager, the stage's
    clip) or 'torch' (eager, torch's clip); returns the parameters."""
    model = _mlp()
    stage = PipelineStage(model, [len(model)], device=cuda, chunks=2, checkpoint='except_last')
    opt = torch.optim.SGD(stage.parameters(), lr=0.1)
    graph = StepGraph(stage, F.mse_loss, opt, warmup=2, max_grad_norm=c) \
        if mode == 'graph' else None
    gen = torch.Generator().manual_seed(2)
    for _ in range(steps):
        x = torch.randn(8, 8, generator=gen).to(cuda)
        y = torch.randn(8, 4, generator=gen).to(cuda)
        if graph is not None:
            graph.step(x, y)
            continue
        opt.zero_grad(set_to_none=True)
        stage.train_step(x, y, F.mse_loss)
        if mode == 'stage':
            norm = stage.clip_grad_norm_(c)
        else:
            norm = torch.nn.utils.clip_grad_norm_(list(stage.parameters()), c)
        assert float(norm) > c  # every step clips
        opt.step()
    torch.cuda.synchronize()
    if graph is not None:
        assert graph.captured
    return [p.detach().clone() for p in stage.parameters()]


def test_step_graph_clips_inside_the_captured_step():
    c = 0.05
    graphed, staged, torched = _train('graph', c), _train('stage', c), _train('torch', c)
    initial = [p.detach().to(cuda) for p in _mlp().parameters()]
    assert not any(torch.equal(a, b) for a, b in zip(staged, initial))  # it trained
    for a, b in zip(graphed, staged):
        assert torch.equal(a, b)
    for a, b in zip(graphed, torched):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def test_step_graph_without_bound_is_unchanged():
    model = _mlp()
    stage = PipelineStage(model, [len(model)], device=cuda, chunks=2)
    assert StepGraph(stage, F.mse_loss).max_grad_norm is None


def test_gpipe_clip_matches_torch():
    model = _conv_model()
    pipe = GPipe(model, balance=[2, 3], devices=[0, 0], chunks=2)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 3, 16, 16, generator=gen).to(cuda)
    t = torch.randn(4, 2, 16, 16, generator=gen).to(cuda)
    F.mse_loss(pipe(x), t).backward()
    params = list(pipe.parameters())
    want_norm, _ = _torch_clip(params, 1.0)
    assert abs(float(pipe.grad_norm()) - float(want_norm)) <= 1e-5 * float(want_norm)
    c = 0.5 * float(want_norm)
    want_norm, want = _torch_clip(params, c)
    norm = pipe.clip_grad_norm_(c)
    assert abs(float(norm) - float(want_norm)) <= 1e-5 * float(want_norm)
    for p, w in zip(params, want):
        assert _rel(p.grad, w) <= 1e-5


def _shared_gpu_worker(rank, world, chunks, c):
    device = torch.device('cuda', 0)
    stage = PipelineStage(parity.build('unet'), parity.balance('unet', world), device=device,
                          chunks=chunks, checkpoint='except_last', timeout=60)
    x, t = parity.data('unet', device)
    loss = stage.train_step(x if stage.is_first else None, t if stage.is_last else None,
                            parity.loss_fn('unet'))
    norm = stage.clip_grad_norm_(c)
    torch.cuda.synchronize(device)
    return {'grads': [p.grad.detach().cpu().clone() for p in stage.parameters()],
            'loss': None if loss is None else loss.item(), 'norm': float(norm)}


def test_two_ranks_on_one_gpu_clip_to_the_global_norm(tmp_path):
    """Device -> pinned host -> gloo all-reduce -> device, against the whole model on one
    GPU with the same clip applied."""
    chunks = 3
    grads, loss = parity.reference('unet', cuda, chunks)
    want_norm = float(torch.cat([g.double().reshape(-1) for g in grads]).norm())
    c = 0.5 * want_norm
    results = run(_shared_gpu_worker, 2, tmp_path, chunks, c, backend='gloo', timeout=120)
    assert results[0]['norm'] == results[1]['norm']
    assert abs(results[0]['norm'] - want_norm) <= 1e-4 * want_norm
    refs = [nn.Parameter(g.clone()) for g in grads]
    for q, g in zip(refs, copy.deepcopy(grads)):
        q.grad = g
    torch.nn.utils.clip_grad_norm_(refs, c)
    parity.assert_parity(results, [q.grad for q in refs], loss, rel=1e-4)
