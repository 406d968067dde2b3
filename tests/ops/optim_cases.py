"""Shared cases of the optimizer tests: configurations, inputs and the runs they compare.

``torch.optim`` is the reference throughout: the same class, same hyperparameters, same
gradient sequence and same learning rates (``StepLR(gamma=0.5)``: halving is exact in fp32
and fp64, so the native fp32 LR tensor and torch's host float agree to the bit).
"""
import torch
from torch import nn

from torchgpipe_amd import optim

STEPS = 5
LR = {'sgd': 0.1, 'rmsprop': 0.01}

# name -> (kind, keyword arguments)
CONFIGS = {
    'sgd': ('sgd', {}),
    'sgd_momentum': ('sgd', {'momentum': 0.9}),
    'sgd_momentum_dampening': ('sgd', {'momentum': 0.9, 'dampening': 0.3}),
    'sgd_nesterov': ('sgd', {'momentum': 0.9, 'nesterov': True}),
    'sgd_weight_decay': ('sgd', {'momentum': 0.9, 'weight_decay': 1e-4}),
    'rmsprop': ('rmsprop', {}),
    'rmsprop_momentum': ('rmsprop', {'momentum': 0.9}),
    'rmsprop_centered': ('rmsprop', {'centered': True}),
    'rmsprop_all': ('rmsprop', {'centered': True, 'momentum': 0.9, 'weight_decay': 1e-4}),
}

NATIVE = {'sgd': optim.SGD, 'rmsprop': optim.RMSprop}
TORCH = {'sgd': torch.optim.SGD, 'rmsprop': torch.optim.RMSprop}
STATE_KEYS = ('momentum_buffer', 'square_avg', 'grad_avg')


def make_values(numels, seed=0, dtype=torch.float32):
    """Per tensor: initial values and ``STEPS`` gradients (CPU, ``dtype``), scales 1e-2..1e1."""
    gen = torch.Generator().manual_seed(seed)
    inits, grads = [], []
    for i, n in enumerate(numels):
        scale = 10.0 ** (-2 + 3 * (i % 4) / 3)
        inits.append(torch.randn(n, generator=gen, dtype=torch.float64).to(dtype))
        grads.append([(torch.randn(n, generator=gen, dtype=torch.float64) * scale).to(dtype)
                      for _ in range(STEPS)])
    return inits, grads


def as_params(inits, device='cpu', dtype=None):
    return [nn.Parameter(v.to(device=device, dtype=dtype or v.dtype).clone()) for v in inits]


def set_grads(params, grads, step):
    for p, g in zip(params, grads):
        p.grad = g[step].to(device=p.device, dtype=p.dtype).clone()


def build(cls, config, params, lr=None):
    kind, kwargs = CONFIGS[config]
    if cls in (torch.optim.SGD, torch.optim.RMSprop):
        kwargs = dict(kwargs, foreach=False)
    return cls(params, lr=LR[kind] if lr is None else lr, **kwargs)


def snapshot(opt, params):
    """[(param, {state key: tensor})] as CPU copies."""
    out = []
    for p in params:
        state = {k: v.detach().cpu().clone() for k, v in opt.state[p].items()
                 if k in STATE_KEYS}
        out.append((p.detach().cpu().clone(), state))
    return out


def run(cls, config, inits, grads, device='cpu', dtype=None, steps=STEPS, lr=None,
        grouped=False):
    """``steps`` updates with the LR halved after each; the snapshot after every step.
    ``grouped``: one parameter group (on the GPU: one launch) per tensor."""
    params = as_params(inits, device, dtype)
    opt = build(cls, config, [{'params': [p]} for p in params] if grouped else params, lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    history = []
    for step in range(steps):
        set_grads(params, grads, step)
        opt.step()
        sched.step()
        history.append(snapshot(opt, params))
    return history, opt, params
