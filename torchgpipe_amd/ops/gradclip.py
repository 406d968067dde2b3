"""Global-norm gradient clipping on the native multi-tensor kernels (``csrc/gradclip.hip``).

``clip_grad_norm_`` is a drop-in for ``torch.nn.utils.clip_grad_norm_`` over the parameters
of this process.  For the Euclidean norm, fp32 and bf16 gradients on a GPU are read once by
``grad_sumsq`` (squares and sums in fp64, one deterministic result per call) and rewritten
by ``grad_scale_`` only when the norm exceeds the bound: the kernel reads the device-resident
sum itself, so nothing is read on the host and the call can sit inside a captured step.

Everything else -- CPU tensors, fp16 / fp64 gradients, non-dense views, other norm types --
runs the same math in PyTorch operations (the ``_ext`` convention: the CPU path is the
oracle of the kernels).  The pieces are public so that a pipeline stage can sum the squares
over its ranks between the two passes (``PipelineStage.clip_grad_norm_``).
"""
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from torchgpipe_amd.ops import _ext

__all__ = ['is_dense', 'grad_sumsq', 'scale_grads_', 'grad_power_sum', 'norm_of', 'scale_by_norm_',
           'gradients', 'result_dtype', 'check_finite', 'clip_grad_norm_', 'grad_norm',
           'clip_info']

_NATIVE_DTYPES = (torch.float32, torch.bfloat16)


def clip_info() -> List[int]:
    """``[chunk elements (fp32), chunk elements (bf16), tensors per launch, threads]``."""
    return list(_ext.require().grad_clip_info())


def is_dense(t: Tensor) -> bool:
    """Whether the Python layer hands ``t`` to the multi-tensor kernels as one span of storage:
    contiguous, channels_last or channels_last_3d.  Narrower than the ops' own check
    (non-overlapping and dense); other dense permutations take the PyTorch-operation path."""
    if t.is_contiguous():
        return True
    if t.dim() == 4:
        return t.is_contiguous(memory_format=torch.channels_last)
    if t.dim() == 5:
        return t.is_contiguous(memory_format=torch.channels_last_3d)
    return False


def _native(t: Tensor) -> bool:
    return t.is_cuda and t.dtype in _NATIVE_DTYPES and is_dense(t)


def _split(tensors: Sequence[Tensor]) -> Tuple[List[List[Tensor]], List[Tensor]]:
    """``tensors`` as the lists the native ops take (one per dtype) and the rest."""
    native: Dict[torch.dtype, List[Tensor]] = {}
    rest: List[Tensor] = []
    for t in tensors:
        if _native(t):
            native.setdefault(t.dtype, []).append(t)
        else:
            rest.append(t)
    return list(native.values()), rest


def _check_dense_layout(tensors: Sequence[Tensor]) -> None:
    for t in tensors:
        if t.is_sparse or t.layout != torch.strided:
            raise NotImplementedError('gradient clipping does not support sparse gradients')


def _by_device(tensors: Sequence[Tensor]) -> Dict[torch.device, List[Tensor]]:
    groups: Dict[torch.device, List[Tensor]] = {}
    for t in tensors:
        groups.setdefault(t.device, []).append(t)
    return groups


def _device_sumsq(tensors: Sequence[Tensor], device: torch.device) -> Tensor:
    """Sum of squares of ``tensors``, all on ``device``: a 0-dim fp64 tensor there."""
    total: Optional[Tensor] = None
    native, rest = _split(tensors)
    for group in native:
        part = _ext.require(group[0]).grad_sumsq(group).reshape(())
        total = part if total is None else total + part
    for t in rest:
        part = t.double().pow(2).sum()
        total = part if total is None else total + part
    if total is None:
        return torch.zeros((), dtype=torch.float64, device=device)
    return total


def grad_sumsq(tensors: Sequence[Tensor], device: Optional[torch.device] = None) -> Tensor:
    """Sum of squares of every element of ``tensors`` as a 0-dim fp64 tensor.

    The result lives on ``device`` (default: the first tensor's device; the CPU for an empty
    list).  Tensors on other devices are summed there and brought over with non-blocking
    copies; nothing is read on the host.
    """
    _check_dense_layout(tensors)
    if device is None:
        device = tensors[0].device if tensors else torch.device('cpu')
    total: Optional[Tensor] = None
    for dev, group in _by_device(tensors).items():
        part = _device_sumsq(group, dev).to(device, non_blocking=True)
        total = part if total is None else total + part
    if total is None:
        return torch.zeros((), dtype=torch.float64, device=device)
    return total


def scale_grads_(tensors: Sequence[Tensor], sumsq: Tensor, max_norm: float,
                 eps: float = 1e-6) -> None:
    """Multiply ``tensors`` in place by ``min(1, max_norm / (sqrt(sumsq) + eps))``.

    ``sumsq`` is a device-resident fp64 scalar (0-dim or ``[1]``).  The native kernel reads
    it and leaves the gradients untouched when the coefficient is at least 1; a NaN
    coefficient is applied (every element becomes NaN), as in PyTorch.
    """
    _check_dense_layout(tensors)
    sumsq = sumsq.reshape(()).double()
    for dev, group in _by_device(tensors).items():
        s = sumsq.to(dev, non_blocking=True)
        native, rest = _split(group)
        for same in native:
            _ext.require(same[0]).grad_scale_(same, s.reshape(1), float(max_norm), float(eps))
        if rest:
            coef = torch.clamp(max_norm / (s.sqrt() + eps), max=1.0)
            for t in rest:
                t.mul_(coef)


def grad_power_sum(tensors: Sequence[Tensor], norm_type: float = 2.0,
                   device: Optional[torch.device] = None) -> Tensor:
    """What ranks add up (``inf``: take the max of) to form the ``norm_type`` norm.

    The sum of ``|x| ** norm_type`` over all elements (``inf``: the largest ``|x|``) as a
    0-dim fp64 tensor on ``device``; :func:`norm_of` turns the combined value into the norm.
    """
    norm_type = float(norm_type)
    if norm_type == 2.0:
        return grad_sumsq(tensors, device)
    _check_dense_layout(tensors)
    if device is None:
        device = tensors[0].device if tensors else torch.device('cpu')
    total = torch.zeros((), dtype=torch.float64, device=device)
    for t in tensors:
        if t.numel() == 0:
            continue
        norm = torch.linalg.vector_norm(t, norm_type).double().to(device, non_blocking=True)
        total = torch.maximum(total, norm) if math.isinf(norm_type) else \
            total + norm.pow(norm_type)
    return total


def norm_of(power_sum: Tensor, norm_type: float = 2.0) -> Tensor:
    """The norm whose :func:`grad_power_sum` is ``power_sum``."""
    norm_type = float(norm_type)
    if norm_type == 2.0:
        return power_sum.sqrt()
    if math.isinf(norm_type):
        return power_sum
    return power_sum.pow(1.0 / norm_type)


def scale_by_norm_(tensors: Sequence[Tensor], power_sum: Tensor, max_norm: float,
                   norm_type: float = 2.0, eps: float = 1e-6) -> None:
    """Clip ``tensors`` in place given the combined :func:`grad_power_sum`."""
    if float(norm_type) == 2.0:
        scale_grads_(tensors, power_sum, max_norm, eps)
        return
    coef = torch.clamp(max_norm / (norm_of(power_sum, norm_type) + eps), max=1.0)
    for t in tensors:
        t.mul_(coef.to(t.device, non_blocking=True))


def gradients(parameters: Union[Tensor, Iterable[Tensor]]) -> List[Tensor]:
    """The gradients of ``parameters`` that exist (``None`` gradients are skipped)."""
    if isinstance(parameters, Tensor):
        parameters = [parameters]
    return [p.grad for p in parameters if p.grad is not None]


def result_dtype(grads: Sequence[Tensor]) -> torch.dtype:
    """The dtype of the returned norm: fp64 when any gradient is fp64, else fp32."""
    return torch.float64 if any(g.dtype == torch.float64 for g in grads) else torch.float32


def check_finite(norm: Tensor, norm_type: float) -> None:
    """``error_if_nonfinite``: the one host read of the norm."""
    if bool(torch.logical_or(norm.isnan(), norm.isinf())):
        raise RuntimeError(
            f'The total norm of order {norm_type} for gradients from '
            '`parameters` is non-finite, so it cannot be clipped. To disable '
            'this error and scale the gradients by the non-finite norm anyway, '
            'set `error_if_nonfinite=False`')


def grad_norm(parameters: Union[Tensor, Iterable[Tensor]], norm_type: float = 2.0) -> Tensor:
    """The total ``norm_type`` norm of the parameters' gradients; nothing is modified."""
    grads = gradients(parameters)
    if not grads:
        return torch.tensor(0.)
    total = grad_power_sum(grads, norm_type)
    return norm_of(total, norm_type).to(result_dtype(grads))


def clip_grad_norm_(parameters: Union[Tensor, Iterable[Tensor]], max_norm: float,
                    norm_type: float = 2.0, error_if_nonfinite: bool = False) -> Tensor:
    """Clip the global gradient norm of ``parameters`` in place; returns the norm before.

    A drop-in for ``torch.nn.utils.clip_grad_norm_`` over parameters of this process, on any
    mix of devices: per-device sums are combined on the first gradient's device.  Without
    ``error_if_nonfinite`` nothing is read on the host.  The norm comes back as a 0-dim fp32
    tensor (fp64 when any gradient is fp64).

    This clips to the norm of the parameters *given*: for a model split over processes use
    ``PipelineStage.clip_grad_norm_``, which sums over the pipeline's ranks first.
    """
    grads = gradients(parameters)
    max_norm, norm_type = float(max_norm), float(norm_type)
    if not grads:
        return torch.tensor(0.)
    total = grad_power_sum(grads, norm_type)
    norm = norm_of(total, norm_type)
    if error_if_nonfinite:
        check_finite(norm, norm_type)
    scale_by_norm_(grads, total, max_norm, norm_type)
    return norm.to(result_dtype(grads))
