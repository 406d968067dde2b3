"""``torchgpipe_amd.optim`` on the CPU: the PyTorch-operation path, which is the oracle of the
kernels, is bitwise ``torch.optim``'s single-tensor loop; the classes keep torch's interface.
"""
import copy

import pytest
import torch
from torch import nn

from tests.ops import optim_cases as cases
from torchgpipe_amd import optim
from torchgpipe_amd.ops import gradclip

NUMELS = [1, 7, 64, 300]


def _assert_same(got, want):
    assert len(got) == len(want)
    for (gp, gs), (wp, ws) in zip(got, want):
        assert torch.equal(gp, wp)
        assert gs.keys() == ws.keys()
        for key in gs:
            assert torch.equal(gs[key], ws[key]), key


@pytest.mark.parametrize('config', list(cases.CONFIGS))
def test_bitwise_equal_to_torch_single_tensor(config):
    kind = cases.CONFIGS[config][0]
    inits, grads = cases.make_values(NUMELS)
    want, _, _ = cases.run(cases.TORCH[kind], config, inits, grads)
    got, opt, params = cases.run(cases.NATIVE[kind], config, inits, grads)
    for step in range(cases.STEPS):
        _assert_same(got[step], want[step])
    assert isinstance(opt, cases.TORCH[kind]) and optim.is_native(opt)
    if kind == 'rmsprop':
        assert all(float(opt.state[p]['step']) == cases.STEPS for p in params)


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop'])
def test_lr_is_a_tensor_the_scheduler_fills_in_place(kind):
    params = cases.as_params([torch.ones(3)])
    opt = cases.NATIVE[kind](params, lr=0.25)
    lr = opt.param_groups[0]['lr']
    assert isinstance(lr, torch.Tensor) and lr.dim() == 0 and lr.dtype == torch.float32
    assert lr.device == params[0].device and float(lr) == 0.25
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for step in range(3):
        params[0].grad = torch.ones(3)
        opt.step()
        sched.step()
        assert opt.param_groups[0]['lr'] is lr
        assert float(lr) == 0.25 * 0.5 ** (step + 1)
    # a group added later gets a tensor too
    extra = nn.Parameter(torch.zeros(2, dtype=torch.float64))
    opt.add_param_group({'params': [extra], 'lr': 0.5})
    assert isinstance(opt.param_groups[1]['lr'], torch.Tensor)
    assert opt.param_groups[1]['lr'].dtype == torch.float32
    assert opt.param_groups[0]['lr'] is lr


@pytest.mark.parametrize('config', ['sgd_weight_decay', 'rmsprop_all'])
def test_state_dict_round_trips_with_the_torch_class(config):
    kind = cases.CONFIGS[config][0]
    inits, grads = cases.make_values(NUMELS, seed=1)
    _, native, nparams = cases.run(cases.NATIVE[kind], config, inits, grads, steps=2)
    _, ref, rparams = cases.run(cases.TORCH[kind], config, inits, grads, steps=2)

    # native -> torch
    fresh = cases.as_params([p.detach() for p in nparams])
    into_torch = cases.build(cases.TORCH[kind], config, fresh)
    into_torch.load_state_dict(copy.deepcopy(native.state_dict()))
    # torch -> native: the LR tensor keeps its identity and takes the loaded value
    fresh_native = cases.as_params([p.detach() for p in rparams])
    into_native = cases.build(cases.NATIVE[kind], config, fresh_native)
    lr = into_native.param_groups[0]['lr']
    into_native.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert into_native.param_groups[0]['lr'] is lr
    assert float(lr) == float(torch.tensor(float(ref.param_groups[0]['lr'])))  # in fp32
    assert float(ref.param_groups[0]['lr']) == cases.LR[kind] / 4

    # all four continue alike
    for opt, params in ((native, nparams), (ref, rparams), (into_torch, fresh),
                        (into_native, fresh_native)):
        cases.set_grads(params, grads, 2)
        opt.step()
    want = cases.snapshot(ref, rparams)
    _assert_same(cases.snapshot(native, nparams), want)
    _assert_same(cases.snapshot(into_torch, fresh), want)
    _assert_same(cases.snapshot(into_native, fresh_native), want)
    # and back: what the native class saves, the native class loads
    again = cases.build(cases.NATIVE[kind], config, cases.as_params(inits))
    again.load_state_dict(copy.deepcopy(into_native.state_dict()))
    assert set(again.state_dict()['state'][0]) == set(ref.state_dict()['state'][0])


@pytest.mark.parametrize('config', ['sgd_weight_decay', 'rmsprop_all'])
@pytest.mark.parametrize('active', [True, False])
def test_fused_clip_equals_clip_then_step(config, active):
    kind = cases.CONFIGS[config][0]
    inits, grads = cases.make_values(NUMELS, seed=2)
    fused_params, plain_params = cases.as_params(inits), cases.as_params(inits)
    fused = cases.build(cases.NATIVE[kind], config, fused_params)
    plain = cases.build(cases.NATIVE[kind], config, plain_params)
    for step in range(3):
        cases.set_grads(fused_params, grads, step)
        cases.set_grads(plain_params, grads, step)
        before = [p.grad.clone() for p in fused_params]
        norm = float(gradclip.grad_norm(plain_params))
        bound = norm * (0.5 if active else 2.0)
        gradclip.clip_grad_norm_(plain_params, bound)
        plain.step()
        fused.step(grad_sumsq=gradclip.grad_sumsq(before), max_norm=bound)
        assert all(torch.equal(p.grad, b) for p, b in zip(fused_params, before))
        clipped = not all(torch.equal(p.grad, b) for p, b in zip(plain_params, before))
        assert clipped == active
        _assert_same(cases.snapshot(fused, fused_params), cases.snapshot(plain, plain_params))
    with pytest.raises(ValueError, match='go together'):
        fused.step(max_norm=1.0)


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop'])
def test_none_gradients_are_skipped_and_mixed_lists_work(kind):
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(6, 5, generator=gen)
    values = [torch.randn(9, generator=gen), torch.randn(4, dtype=torch.float64, generator=gen),
              base, torch.randn(3, generator=gen)]

    def params():
        out = cases.as_params(values)
        out[2] = nn.Parameter(base.clone().t())  # not contiguous
        assert not out[2].is_contiguous()
        return out

    ours, theirs = params(), params()
    kwargs = {'momentum': 0.9, 'weight_decay': 1e-3}
    a = cases.NATIVE[kind](ours, lr=0.0625, **kwargs)  # exact in fp32: the fp64 tensor
    b = cases.TORCH[kind](theirs, lr=0.0625, foreach=False, **kwargs)
    for step in range(3):
        for p, q in zip(ours[:3], theirs[:3]):
            g = torch.randn(p.shape, dtype=p.dtype, generator=gen)
            p.grad, q.grad = g.clone(), g.clone()
        a.step()
        b.step()
    for p, q in zip(ours, theirs):
        assert torch.equal(p, q)
    assert torch.equal(ours[3], values[3]) and len(a.state[ours[3]]) == 0


def test_sparse_gradients_raise():
    p = nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.zeros(4, 3).to_sparse()
    with pytest.raises(RuntimeError, match='sparse'):
        optim.SGD([p], lr=0.1).step()
    with pytest.raises(RuntimeError, match='sparse'):
        optim.RMSprop([p], lr=0.1).step()


def test_unsupported_options_are_refused():
    p = [nn.Parameter(torch.zeros(2))]
    for kwargs in ({'maximize': True}, {'differentiable': True}, {'fused': True}):
        with pytest.raises(ValueError, match=next(iter(kwargs))):
            optim.SGD(p, lr=0.1, **kwargs)
    for kwargs in ({'maximize': True}, {'differentiable': True}, {'capturable': True}):
        with pytest.raises(ValueError, match=next(iter(kwargs))):
            optim.RMSprop(p, lr=0.1, **kwargs)
    opt = optim.SGD(p, lr=0.1, foreach=True)  # accepted, ignored
    opt.param_groups[0]['maximize'] = True
    p[0].grad = torch.ones(2)
    with pytest.raises(ValueError, match='maximize'):
        opt.step()


def test_closure_runs_with_gradients_enabled():
    p = nn.Parameter(torch.tensor([2.0]))
    opt = optim.SGD([p], lr=0.5)

    def closure():
        opt.zero_grad()
        loss = (p * p).sum()
        loss.backward()
        return loss

    assert float(opt.step(closure).detach()) == 4.0
    assert float(p.detach()) == 0.0
