"""``optimizer_step`` on ``GPipe`` and a one-rank ``PipelineStage`` (CPU): with a native
optimizer the clip rides in the update and equals ``clip_grad_norm_`` + ``step()``; with a
``torch.optim`` optimizer it *is* those two calls."""
import copy

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd import GPipe, optim
from torchgpipe_amd.parallel import PipelineStage


def _mlp() -> nn.Sequential:
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 16), nn.Tanh(), nn.Linear(16, 16), nn.Tanh(),
                         nn.Linear(16, 4))


X = torch.randn(8, 8, generator=torch.Generator().manual_seed(1))
T = torch.randn(8, 4, generator=torch.Generator().manual_seed(2))


def _gpipe():
    pipe = GPipe(_mlp(), balance=[2, 3], devices=['cpu', 'cpu'], chunks=2)
    F.mse_loss(pipe(X), T).backward()
    return pipe


def _stage():
    model = _mlp()
    stage = PipelineStage(model, [len(model)], chunks=2, checkpoint='never')
    stage.train_step(X, T, F.mse_loss)
    return stage


OPTIMIZERS = {
    'native_sgd': lambda p: optim.SGD(p, lr=0.1, momentum=0.9, weight_decay=1e-4),
    'native_rmsprop': lambda p: optim.RMSprop(p, lr=0.01, centered=True, momentum=0.9),
    'torch_sgd': lambda p: torch.optim.SGD(p, lr=0.1, momentum=0.9, weight_decay=1e-4),
}


@pytest.mark.parametrize('make', [_gpipe, _stage], ids=['gpipe', 'stage'])
@pytest.mark.parametrize('optimizer', list(OPTIMIZERS))
@pytest.mark.parametrize('active', [True, False])
def test_optimizer_step_equals_clip_then_step(make, optimizer, active):
    fused, plain = make(), make()
    norm = float(plain.grad_norm())
    bound = norm * (0.5 if active else 2.0)
    a = OPTIMIZERS[optimizer](list(fused.parameters()))
    b = OPTIMIZERS[optimizer](list(plain.parameters()))
    before = [p.grad.clone() for p in fused.parameters()]
    for step in range(2):  # the second step has momentum / averages to carry
        for model in (fused, plain):  # the same gradients again: a clip in place scaled them
            for p, g in zip(model.parameters(), before):
                p.grad = g.clone()
        got = fused.optimizer_step(a, bound)
        want = plain.clip_grad_norm_(bound)
        b.step()
        assert torch.equal(got, want) and got.dtype == want.dtype and got.dim() == 0
        assert float(got) == norm  # what grad_norm() returned
    for p, q in zip(fused.parameters(), plain.parameters()):
        assert torch.equal(p, q)
    initial = list(_mlp().parameters())
    assert not any(torch.equal(p, q) for p, q in zip(fused.parameters(), initial))
    untouched = all(torch.equal(p.grad, g) for p, g in zip(fused.parameters(), before))
    # the native path leaves .grad unscaled; torch's path clips it in place when active
    assert untouched == (optim.is_native(a) or not active)


@pytest.mark.parametrize('make', [_gpipe, _stage], ids=['gpipe', 'stage'])
def test_without_a_bound_it_is_step(make):
    fused, plain = make(), make()
    a = OPTIMIZERS['native_sgd'](list(fused.parameters()))
    b = OPTIMIZERS['torch_sgd'](list(plain.parameters()))
    assert fused.optimizer_step(a) is None
    b.step()
    for p, q in zip(fused.parameters(), plain.parameters()):
        assert torch.equal(p, q)


def test_other_norms_take_the_two_calls():
    fused, plain = _stage(), _stage()
    a = OPTIMIZERS['native_sgd'](list(fused.parameters()))
    b = OPTIMIZERS['native_sgd'](list(plain.parameters()))
    bound = 0.5 * float(plain.grad_norm(float('inf')))
    got = fused.optimizer_step(a, bound, norm_type=float('inf'))
    want = plain.clip_grad_norm_(bound, float('inf'))
    b.step()
    assert torch.equal(got, want)
    for p, q in zip(fused.parameters(), plain.parameters()):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad)


def test_stage_without_optimizer_still_takes_part():
    stage = _stage()
    before = copy.deepcopy([p.detach() for p in stage.parameters()])
    norm = float(stage.grad_norm())
    assert float(stage.optimizer_step(None, 0.5 * norm)) == norm
    assert all(torch.equal(p, q) for p, q in zip(stage.parameters(), before))
    assert stage.optimizer_step(None) is None


def test_error_if_nonfinite_raises_before_the_update():
    stage = _stage()
    params = list(stage.parameters())
    params[0].grad[0, 0] = float('inf')
    before = [p.detach().clone() for p in params]
    opt = OPTIMIZERS['native_sgd'](params)
    with pytest.raises(RuntimeError, match='non-finite'):
        stage.optimizer_step(opt, 1.0, error_if_nonfinite=True)
    assert all(torch.equal(p, q) for p, q in zip(params, before))
