"""Optimizers whose step is one native pass (``csrc/optim.hip``): :class:`SGD`, :class:`RMSprop`.

Both subclass their ``torch.optim`` namesakes -- ``param_groups``, ``state_dict`` /
``load_state_dict``, ``isinstance`` and the state keys (``momentum_buffer``; ``square_avg``,
``grad_avg``, ``momentum_buffer``, ``step``) are torch's, and a state dict moves between the
two classes in both directions -- and differ in three ways:

* **The learning rate is a tensor.**  ``group['lr']`` is a 0-dim fp32 tensor on the device of
  the group's first parameter, and the kernels read it there.  ``torch.optim.lr_scheduler``
  fills a tensor LR in place, so a schedule changes the rate between the replays of a step
  captured by :class:`~torchgpipe_amd.parallel.graph.StepGraph`.  The other hyperparameters
  are launch constants.
* **One pass.**  fp32, dense GPU parameters (with gradients and state of the same layout)
  are updated by one multi-tensor kernel per group and device: the gradient is read once, the
  parameter and each state tensor are read once and written once.
* **The clip rides along.**  ``step(grad_sumsq=total, max_norm=bound)`` takes the sum of
  squares of all gradients (``ops.gradclip.grad_sumsq``, all-reduced where the model is split
  over ranks) and scales each gradient by ``min(1, max_norm / (sqrt(total) + clip_eps))`` as
  it is loaded.  ``.grad`` is not written: afterwards it still holds the *unclipped*
  gradient.  The result is what ``clip_grad_norm_`` followed by ``step()`` gives, bit for
  bit.  ``PipelineStage.optimizer_step`` / ``GPipe.optimizer_step`` do both halves.

Every other parameter -- CPU, other dtypes, non-dense views, gradients laid out differently
from their parameter -- runs the same formulas as PyTorch operations in the order of torch's
single-tensor loops (the ``_ext`` convention: the CPU path is the oracle of the kernels, and
on fp32 CPU tensors it is bitwise ``torch.optim``'s ``foreach=False``).  A GPU parameter the
kernels take raises when the extension is not built, like every native op.

``maximize``, ``differentiable``, ``capturable`` and ``fused`` are refused.  RMSprop's
``step`` counter (which its update never reads) is advanced on the host when ``step()`` runs
in Python: replays of a captured graph do not advance it.
"""
from typing import Any, Callable, Dict, Iterable, List, Optional, Tuple, Union

import torch
from torch import Tensor

from torchgpipe_amd.ops import _ext
from torchgpipe_amd.ops.gradclip import is_dense

__all__ = ['SGD', 'RMSprop', 'is_native', 'optim_info']

Params = Union[Iterable[Tensor], Iterable[Dict[str, Any]]]


def optim_info() -> List[int]:
    """``[chunk elements, tensors per launch, threads]`` of the step kernels."""
    return list(_ext.require().optim_info())


def is_native(optimizer: object) -> bool:
    """Whether ``optimizer.step`` takes ``grad_sumsq=`` / ``max_norm=`` (the fused clip)."""
    return isinstance(optimizer, _Native)


def _kernel_takes(p: Tensor, others: List[Tensor]) -> bool:
    if not (p.is_cuda and p.dtype == torch.float32 and p.layout == torch.strided and is_dense(p)):
        return False
    return all(t.device == p.device and t.dtype == torch.float32 and t.layout == torch.strided
               and t.shape == p.shape and (t.stride() == p.stride() or t.numel() <= 1)
               for t in others)


class _Clip:
    """The optional fused clip of one ``step`` call: the coefficient per device."""

    def __init__(self, grad_sumsq: Optional[Tensor], max_norm: Optional[float],
                 clip_eps: float) -> None:
        if (grad_sumsq is None) != (max_norm is None):
            raise ValueError('step(): grad_sumsq and max_norm go together')
        self.sumsq = None if grad_sumsq is None else grad_sumsq.detach().reshape(()).double()
        self.max_norm = 0.0 if max_norm is None else float(max_norm)
        self.eps = float(clip_eps)
        self._on: Dict[torch.device, Tensor] = {}

    def on(self, device: torch.device) -> Optional[Tensor]:
        """The sum of squares as a ``[1]`` fp64 tensor on ``device`` (``None``: no clip)."""
        if self.sumsq is None:
            return None
        if device not in self._on:
            self._on[device] = self.sumsq.to(device, non_blocking=True).reshape(1)
        return self._on[device]

    def apply(self, grad: Tensor) -> Tensor:
        """``grad`` clipped, as ``ops.gradclip.scale_grads_`` would leave it, in a new tensor."""
        s = self.on(grad.device)
        if s is None:
            return grad
        coef = torch.clamp(self.max_norm / (s.reshape(()).sqrt() + self.eps), max=1.0)
        return grad.mul(coef)


class _Native:
    """What the native optimizers share: the tensor LR and the routing of ``step``."""

    param_groups: List[Dict[str, Any]]
    state: Dict[Tensor, Dict[str, Any]]

    # -- the tensor learning rate -------------------------------------------------------

    @staticmethod
    def _lr_tensor(group: Dict[str, Any]) -> Tensor:
        params = group['params']
        device = params[0].device if params else torch.device('cpu')
        lr = group['lr']
        if isinstance(lr, Tensor):
            if lr.numel() != 1:
                raise ValueError('Tensor lr must be 1-element')
            return lr.detach().to(device=device, dtype=torch.float32).reshape(()).clone()
        return torch.tensor(float(lr), dtype=torch.float32, device=device)

    def _tensor_lrs(self) -> None:
        for group in self.param_groups:
            lr = group['lr']
            if not (isinstance(lr, Tensor) and lr.dim() == 0 and lr.dtype == torch.float32):
                group['lr'] = self._lr_tensor(group)

    def add_param_group(self, param_group: Dict[str, Any]) -> None:
        super().add_param_group(param_group)  # type: ignore[misc]
        self._tensor_lrs()

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        """As ``torch.optim.Optimizer.load_state_dict``; each group's LR tensor keeps its
        identity (a captured step and a scheduler hold on to it) and takes the loaded value."""
        kept = [group['lr'] for group in self.param_groups]
        super().load_state_dict(state_dict)  # type: ignore[misc]
        for group, lr in zip(self.param_groups, kept):
            if isinstance(lr, Tensor) and group['lr'] is not lr:
                lr.fill_(float(group['lr']))
                group['lr'] = lr
        self._tensor_lrs()

    @staticmethod
    def _refuse(group: Dict[str, Any]) -> None:
        for key in ('maximize', 'differentiable', 'capturable'):
            if group.get(key, False):
                raise ValueError(f'torchgpipe_amd.optim does not support {key}=True '
                                 '(use the torch.optim class)')
        if group.get('fused', None):
            raise ValueError('torchgpipe_amd.optim does not support fused=True: its step is '
                             'the native fused kernel already')

    # -- step ---------------------------------------------------------------------------

    @torch.no_grad()
    def step(self, closure: Optional[Callable[[], Any]] = None, *,  # type: ignore[override]
             grad_sumsq: Optional[Tensor] = None, max_norm: Optional[float] = None,
             clip_eps: float = 1e-6) -> Any:
        """One update.  With ``grad_sumsq`` (the sum of squares of *all* gradients, a 0-dim or
        ``[1]`` tensor on any device) and ``max_norm`` the gradients are clipped to that
        global norm as they are read; ``.grad`` keeps the unclipped values."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = _Clip(grad_sumsq, max_norm, clip_eps)
        for group in self.param_groups:
            self._refuse(group)
            lr = group['lr']
            by_device: Dict[torch.device, List[Tensor]] = {}
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.grad.layout != torch.strided:
                    raise RuntimeError(f'{type(self).__name__} does not support sparse gradients')
                by_device.setdefault(p.device, []).append(p)
            for device, params in by_device.items():
                lr_here = lr if lr.device == device else lr.to(device, non_blocking=True)
                self._step_device(group, params, lr_here, clip)
        return loss

    def _step_device(self, group: Dict[str, Any], params: List[Tensor], lr: Tensor,
                     clip: _Clip) -> None:
        raise NotImplementedError


def _minus_lr_times(param: Tensor, update: Tensor, lr: Tensor) -> None:
    """``param -= lr * update``: torch's ``add_(update, alpha=-lr)`` on the CPU; on a GPU the
    rate stays on the device (no host read, so the call can be captured)."""
    if param.is_cuda:
        param.addcmul_(update, lr.to(param.dtype), value=-1)
    else:
        param.add_(update, alpha=-float(lr))


class SGD(_Native, torch.optim.SGD):
    """``torch.optim.SGD`` on the native one-pass kernel, with a device-resident LR.

    Arguments as ``torch.optim.SGD`` (``foreach`` is accepted and ignored).  See the module
    docstring for ``step(grad_sumsq=, max_norm=)`` and what falls back to PyTorch operations.
    """

    def __init__(self, params: Params, lr: Union[float, Tensor] = 1e-3, momentum: float = 0,
                 dampening: float = 0, weight_decay: float = 0, nesterov: bool = False, *,
                 maximize: bool = False, foreach: Optional[bool] = None,
                 differentiable: bool = False, fused: Optional[bool] = None) -> None:
        self._refuse({'maximize': maximize, 'differentiable': differentiable, 'fused': fused})
        host_lr = float(lr)
        torch.optim.SGD.__init__(self, params, lr=host_lr, momentum=momentum,
                                 dampening=dampening, weight_decay=weight_decay,
                                 nesterov=nesterov, foreach=False)
        self._tensor_lrs()

    def _step_device(self, group: Dict[str, Any], params: List[Tensor], lr: Tensor,
                     clip: _Clip) -> None:
        momentum, dampening = float(group['momentum']), float(group['dampening'])
        wd, nesterov = float(group['weight_decay']), bool(group['nesterov'])
        # [first step, later steps]: parameters, gradients and buffers for the kernel
        native: Tuple[List[List[Tensor]], ...] = ([[], [], []], [[], [], []])
        for p in params:
            g = p.grad
            state = self.state[p]
            buf = state.get('momentum_buffer') if momentum != 0 else None
            if _kernel_takes(p, [g] if buf is None else [g, buf]):
                first = momentum != 0 and buf is None
                if first:
                    buf = state['momentum_buffer'] = torch.empty_like(p)
                lists = native[0 if first else 1]
                lists[0].append(p)
                lists[1].append(g)
                if momentum != 0:
                    lists[2].append(buf)
                continue
            # torch's _single_tensor_sgd
            d = clip.apply(g)
            if wd != 0:
                d = d.add(p, alpha=wd)
            if momentum != 0:
                if buf is None:
                    buf = state['momentum_buffer'] = torch.clone(d).detach()
                else:
                    buf.mul_(momentum).add_(d, alpha=1 - dampening)
                d = d.add(buf, alpha=momentum) if nesterov else buf
            _minus_lr_times(p, d, lr)
        for first, lists in zip((True, False), native):
            if lists[0]:
                _ext.require(lists[0][0]).sgd_step_(
                    lists[0], lists[1], lists[2], lr, momentum, dampening, nesterov, wd, first,
                    clip.on(lr.device), clip.max_norm, clip.eps)


class RMSprop(_Native, torch.optim.RMSprop):
    """``torch.optim.RMSprop`` on the native one-pass kernel, with a device-resident LR.

    Arguments as ``torch.optim.RMSprop`` (``foreach`` is accepted and ignored).  The ``step``
    entry of the state is a host counter that only Python-side steps advance.
    """

    def __init__(self, params: Params, lr: Union[float, Tensor] = 1e-2, alpha: float = 0.99,
                 eps: float = 1e-8, weight_decay: float = 0, momentum: float = 0,
                 centered: bool = False, capturable: bool = False,
                 foreach: Optional[bool] = None, maximize: bool = False,
                 differentiable: bool = False) -> None:
        self._refuse({'maximize': maximize, 'differentiable': differentiable,
                      'capturable': capturable})
        host_lr = float(lr)
        torch.optim.RMSprop.__init__(self, params, lr=host_lr, alpha=alpha, eps=eps,
                                     weight_decay=weight_decay, momentum=momentum,
                                     centered=centered, foreach=False)
        self._tensor_lrs()

    def _state_of(self, p: Tensor, momentum: float, centered: bool) -> Dict[str, Any]:
        state = self.state[p]
        if len(state) == 0:  # torch's RMSprop._init_group
            state['step'] = torch.zeros((), dtype=torch.get_default_dtype())
            state['square_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if momentum > 0:
                state['momentum_buffer'] = torch.zeros_like(
                    p, memory_format=torch.preserve_format)
            if centered:
                state['grad_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    def _step_device(self, group: Dict[str, Any], params: List[Tensor], lr: Tensor,
                     clip: _Clip) -> None:
        alpha, eps = float(group['alpha']), float(group['eps'])
        wd, momentum = float(group['weight_decay']), float(group['momentum'])
        centered = bool(group['centered'])
        native: List[List[Tensor]] = [[], [], [], [], []]
        steps = [self._state_of(p, momentum, centered)['step'] for p in params]
        torch._foreach_add_(steps, 1)  # host counters: one call instead of one per tensor
        for p in params:
            g = p.grad
            state = self.state[p]
            square_avg = state['square_avg']
            grad_avg = state['grad_avg'] if centered else None
            buf = state['momentum_buffer'] if momentum > 0 else None
            tensors = [t for t in (p, g, square_avg, grad_avg, buf) if t is not None]
            if _kernel_takes(p, tensors[1:]):
                for lst, t in zip(native, (p, g, square_avg, grad_avg, buf)):
                    if t is not None:
                        lst.append(t)
                continue
            # torch's _single_tensor_rmsprop
            d = clip.apply(g)
            if wd != 0:
                d = d.add(p, alpha=wd)
            square_avg.mul_(alpha).addcmul_(d, d, value=1 - alpha)
            if grad_avg is not None:
                grad_avg.lerp_(d, 1 - alpha)
                avg = square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_()
            else:
                avg = square_avg.sqrt()
            avg = avg.add_(eps)
            if buf is not None:
                buf.mul_(momentum).addcdiv_(d, avg)
                _minus_lr_times(p, buf, lr)
            elif p.is_cuda:
                p.addcmul_(d.div(avg), lr.to(p.dtype), value=-1)
            else:
                p.addcdiv_(d, avg, value=-float(lr))
        if native[0]:
            _ext.require(native[0][0]).rmsprop_step_(
                native[0], native[1], native[2], native[3], native[4], lr, alpha, eps, wd,
                momentum, centered, clip.on(lr.device), clip.max_norm, clip.eps)
