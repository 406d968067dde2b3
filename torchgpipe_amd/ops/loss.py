"""``nn.CrossEntropyLoss`` over logit rows on the native kernels
(``csrc/cross_entropy.hip``), opt-in.

Forward: one read of the fp32 logits ``[R, V]``; a wave per row (a workgroup per row above 4096
columns) streams it with a running ``(max, sum exp)`` pair and writes that pair per row
(``stat[R, 2]``: the maximum and one over the sum, which keep the softmax good to a few ulp
whatever offset the logits share, where a single fp32 log-sum-exp would not) and the row
losses, and one workgroup reduces them for ``mean`` / ``sum``.  The log-softmax is never
written and nothing of size ``[R, V]`` is saved: the backward reads the logits once more, with
``stat``, and writes ``dx``.  Class indices, ``ignore_index``, label smoothing and the three
reductions are served; class weights and probability targets are not.  No atomics (the same
inputs give the same bits) and no host synchronisation: the row count of ``mean`` stays on
the device.

:class:`NativeCrossEntropyLoss` is a drop-in replacement; nothing routes to it by default.
"""
from typing import Any, Tuple

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from torchgpipe_amd.ops import _ext
from torchgpipe_amd.ops.precision import autocast_lowp

__all__ = ['native_cross_entropy', 'NativeCrossEntropyLoss', 'eligible']

_MAX_ROW_BYTES = 0x7ffffff0  # buffer-resource offsets: a row below 2 GiB, the tensor any size
_REDUCTIONS = {'none': 0, 'mean': 1, 'sum': 2}  # ATen's numbering


# -- test / profiling hooks (not public) ------------------------------------------------------

def _limits() -> Tuple[int, int, int]:
    """(the widest row of the wave-per-row instances, the columns one workgroup of the wide
    backward covers on the float4 path, the same on the dword path)."""
    wave_row_max, chunk, dword_chunk = _ext.require()._cross_entropy_limits()
    return int(wave_row_max), int(chunk), int(dword_chunk)


def _force_instance(wide: int = -1, chunk: int = 0) -> None:
    """``0`` runs the wave-per-row instances at any width, ``1`` the workgroup instances,
    ``-1`` restores the host rule; ``chunk`` 4096 or 8192 sets the wide backward's columns per
    workgroup, ``0`` restores the default."""
    _ext.require()._cross_entropy_force_instance(wide, chunk)


def eligible(logits: Tensor, target: Tensor) -> bool:
    """Whether the native kernels take this call: contiguous fp32 logits ``[R, V]`` and
    contiguous int64 class indices ``[R]`` on the same GPU, ``R >= 1``, ``V >= 1`` and a row
    below 2 GiB (the tensor as a whole may be larger)."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
            and logits.is_contiguous()):
        return False
    if not (target.is_cuda and target.device == logits.device and target.dtype == torch.int64
            and target.dim() == 1 and target.is_contiguous()):
        return False
    rows, width = logits.shape
    return rows >= 1 and width >= 1 and target.shape[0] == rows and 4 * width <= _MAX_ROW_BYTES


class _NativeCrossEntropy(torch.autograd.Function):
    """The two native ops under autograd.  Saved: the logits (alive anyway), the targets,
    ``stat[R, 2]`` and the one-element ``inv_count``."""

    @staticmethod
    def forward(ctx: Any, logits: Tensor, target: Tensor,  # type: ignore[override]
                ignore_index: int, label_smoothing: float, reduction: int) -> Tensor:
        loss, stat, inv_count = _ext.require(logits).cross_entropy_forward(
            logits, target, ignore_index, label_smoothing, reduction)
        ctx.save_for_backward(logits, target, stat, inv_count)
        ctx.args = (ignore_index, label_smoothing, reduction)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad: Tensor):  # type: ignore[override]
        logits, target, stat, inv_count = ctx.saved_tensors
        dx = _ext.require(grad).cross_entropy_backward(
            grad.contiguous(), logits, target, stat, inv_count, *ctx.args)
        return dx, None, None, None, None


def native_cross_entropy(logits: Tensor, target: Tensor, ignore_index: int = -100,
                         reduction: str = 'mean', label_smoothing: float = 0.0) -> Tensor:
    """``F.cross_entropy(logits, target, ignore_index=..., reduction=...,
    label_smoothing=...)`` on the native kernels (see :func:`eligible`; anything else raises).
    A target outside ``[0, V)`` that is not ``ignore_index`` gives a NaN loss for its row."""
    if not eligible(logits, target):
        raise ValueError('native_cross_entropy needs contiguous fp32 logits [R, V] and '
                         'contiguous int64 targets [R] on one GPU')
    if reduction not in _REDUCTIONS:
        raise ValueError(f'{reduction!r} is not a valid value for reduction')
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError('native_cross_entropy needs a label_smoothing in [0, 1)')
    return _NativeCrossEntropy.apply(logits, target, ignore_index, label_smoothing,
                                     _REDUCTIONS[reduction])


class NativeCrossEntropyLoss(nn.CrossEntropyLoss):
    """``nn.CrossEntropyLoss`` whose GPU fp32 forward and backward over ``[R, V]`` logits run on
    the native kernels.

    Same constructor.  CPU tensors, other dtypes or layouts, class weights, probability
    targets, inputs that are not ``[R, V]``, a ``label_smoothing`` of 1 and ``torch.autocast``
    to a lower precision run the plain ``nn.CrossEntropyLoss.forward``."""

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        if (self.weight is not None or self.reduction not in _REDUCTIONS
                or not 0.0 <= self.label_smoothing < 1.0 or not input.is_cuda
                or autocast_lowp('cuda') or not eligible(input, target)):
            return nn.CrossEntropyLoss.forward(self, input, target)
        # (a GPU tensor without the built extension raises, as every native op does)
        return _NativeCrossEntropy.apply(input, target, self.ignore_index, self.label_smoothing,
                                         _REDUCTIONS[self.reduction])
