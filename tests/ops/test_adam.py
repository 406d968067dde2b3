"""``optim.Adam`` / ``optim.AdamW`` on the CPU: the PyTorch-operation path, the oracle of the
kernels, is bitwise ``torch.optim``'s single-tensor loop.  The learning rate is 2^-10, halved
after each step: the fp32 LR tensor and torch's host float then agree to the bit."""
import copy

import pytest
import torch

from tests.ops.optim_cases import STEPS, as_params, make_values, set_grads
from torchgpipe_amd import optim

LR = 2.0 ** -10
CONFIGS = {  # name -> (AdamW?, keyword arguments)
    'adam': (False, {}),
    'adam_wd': (False, {'weight_decay': 1e-4}),
    'adam_amsgrad': (False, {'amsgrad': True}),
    'adamw': (True, {'weight_decay': 1e-2}),
    'adamw_amsgrad': (True, {'weight_decay': 1e-2, 'amsgrad': True}),
}
STATE_KEYS = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


def numels(c=4096):
    """Where a kernel with chunks of ``c`` elements changes path (on the CPU: nine sizes)."""
    return [1, 3, 255, 256, 257, c - 1, c, c + 1, 2 * c + 5]


def build(native, config, params, lr=LR):
    decoupled, kwargs = CONFIGS[config]
    if native:
        return (optim.AdamW if decoupled else optim.Adam)(params, lr=lr, **kwargs)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    return cls(params, lr=lr, foreach=False, **kwargs)


def snapshot(opt, params):
    """[(param, {state key: tensor})] as CPU copies."""
    return [(p.detach().cpu().clone(), {k: v.detach().cpu().clone()
                                        for k, v in opt.state[p].items() if k in STATE_KEYS})
            for p in params]


def run(native, config, inits, grads, device='cpu', dtype=None, steps=STEPS, lr=LR,
        grouped=False, skip=lambda step, i: False):
    """The snapshots after each of ``steps`` updates, the LR halved after each.  ``grouped``:
    one group (launch) per tensor.  ``skip(step, i)``: no gradient for tensor ``i`` then."""
    params = as_params(inits, device, dtype)
    opt = build(native, config, [{'params': [p]} for p in params] if grouped else params, lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    history = []
    for step in range(steps):
        set_grads(params, grads, step)
        for i, p in enumerate(params):
            if skip(step, i):
                p.grad = None
        opt.step()
        sched.step()
        history.append(snapshot(opt, params))
    return history, opt, params


def assert_same(got, want):
    assert len(got) == len(want)
    for (gp, gs), (wp, ws) in zip(got, want):
        assert torch.equal(gp, wp)
        assert gs.keys() == ws.keys() and len(gs) >= 2
        assert all(torch.equal(gs[key], ws[key]) for key in gs)


@pytest.mark.parametrize('config', list(CONFIGS))
def test_bitwise_equal_to_torch_single_tensor(config):
    inits, grads = make_values(numels())
    want, ref, _ = run(False, config, inits, grads)
    got, opt, params = run(True, config, inits, grads)
    for step in range(STEPS):
        assert_same(got[step], want[step])
    assert isinstance(opt, type(ref)) and optim.is_native(opt)
    assert all(float(opt.state[p]['step']) == STEPS for p in params)


@pytest.mark.parametrize('config', ['adam_wd', 'adamw_amsgrad'])
def test_state_dicts_move_both_ways_and_unsupported_options_are_refused(config):
    inits, grads = make_values([1, 7, 300], seed=1)
    _, native, nparams = run(True, config, inits, grads, steps=2)
    _, ref, rparams = run(False, config, inits, grads, steps=2)
    into_torch = build(False, config, as_params([p.detach() for p in nparams]))
    into_torch.load_state_dict(copy.deepcopy(native.state_dict()))
    # torch -> native, saved with capturable=True: the LR tensor keeps its identity
    saved = copy.deepcopy(ref.state_dict())
    saved['param_groups'][0]['capturable'] = True
    into_native = build(True, config, as_params([p.detach() for p in rparams]))
    lr = into_native.param_groups[0]['lr']
    into_native.load_state_dict(saved)
    assert into_native.param_groups[0]['lr'] is lr and float(lr) == LR / 4
    ends = []
    for opt in (ref, native, into_torch, into_native):  # all four continue alike
        params = opt.param_groups[0]['params']
        set_grads(params, grads, 2)
        opt.step()
        assert all(float(opt.state[p]['step']) == 3 for p in params)
        ends.append(snapshot(opt, params))
        assert_same(ends[-1], ends[0])
    cls = type(native)
    for key in ('maximize', 'differentiable', 'capturable', 'fused'):
        with pytest.raises(ValueError, match=key):
            cls(nparams, **{key: True})
    with pytest.raises(ValueError, match='betas'):
        cls(nparams, betas=(torch.tensor(0.9), torch.tensor(0.999)))
    assert optim.Adam(nparams, foreach=True, decoupled_weight_decay=True) \
        .defaults['decoupled_weight_decay']  # foreach: accepted and ignored
