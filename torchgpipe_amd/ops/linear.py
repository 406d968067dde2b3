"""``nn.Linear`` on the native split-bf16 GEMM (``csrc/linear.hip``), opt-in.

The three fp32 matrix products of a Linear layer -- forward, backward-data and the weight
gradient -- as split-bf16 partial products on ``v_mfma_f32_32x32x16_bf16`` with f32
accumulators, the arithmetic of the implicit-GEMM convolutions.  The level of
:func:`~torchgpipe_amd.ops.precision.set_conv_precision` governs them: ``'highest'`` keeps
six partial products (fp32 error bounds), ``'high'`` three, ``'medium'`` ``hi*hi`` alone.

:class:`NativeLinear` is a drop-in ``nn.Linear``; nothing routes to it by default
(``models.vgg.vgg16(native_linear=True)`` builds its classifier from it).  The backward
accumulates the weight and bias gradients straight into ``.grad`` under the
:mod:`~torchgpipe_amd.ops.gradacc` protocol, in the GEMM's epilogue.
"""
from typing import Optional

import torch
from torch import Tensor, nn

from torchgpipe_amd.ops import _ext
from torchgpipe_amd.ops.gradacc import _settle, target
from torchgpipe_amd.ops.precision import autocast_lowp

__all__ = ['native_linear', 'NativeLinear', 'eligible', 'force_plan']

_MAX_BYTES = 0x7ffffff0  # buffer-resource offsets: every operand and result below 2 GiB


def force_plan(tile: int = -1, splits: int = -1) -> None:
    """Test / profiling hook: run every native Linear GEMM on the ``tile`` (64 or 128) with
    ``splits`` reduction splits; ``-1`` restores the host rule."""
    _ext.require().linear_force_plan(tile, splits)


def eligible(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> bool:
    """Whether the native kernels take this call: contiguous fp32 GPU tensors on one device,
    at least one row, and ``x``, ``weight`` and the output each below 2 GiB."""
    tensors = [x, weight] + ([bias] if bias is not None else [])
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               and t.device == x.device for t in tensors):
        return False
    if x.dim() < 1 or weight.dim() != 2 or x.numel() == 0 or weight.numel() == 0:
        return False
    rows = x.numel() // x.shape[-1]
    return 4 * max(x.numel(), weight.numel(), rows * weight.shape[0]) <= _MAX_BYTES


class _NativeLinear(torch.autograd.Function):
    """The four native ops under autograd; gradient accumulation as ``gradacc._Linear``."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor,  # type: ignore[override]
                bias: Optional[Tensor]) -> Tensor:
        ctx.save_for_backward(x, weight)
        ctx.params = (weight, bias)
        return _ext.require(x).linear_forward(x, weight, bias)

    @staticmethod
    def backward(ctx, dy: Tensor):  # type: ignore[override]
        x, weight = ctx.saved_tensors
        wparam, bparam = ctx.params
        ctx.params = (None, None)  # a repeated backward (retain_graph) returns them instead
        need = ctx.needs_input_grad
        ops = _ext.require(dy)
        dy = dy.contiguous()
        dx = ops.linear_backward_data(dy, weight) if need[0] else None
        dw = db = None
        if need[1]:
            fuse, into = target(wparam)
            if fuse and into is not None:
                ops.linear_backward_weight(dy, x, into, True)  # beta = 1 in the epilogue
            else:
                dw = _settle(wparam, ops.linear_backward_weight(dy, x, None, False), fuse, into)
        if need[2]:
            fuse, into = target(bparam)
            if fuse and into is not None:
                ops.linear_bias_grad(dy, into, True)
            else:
                db = _settle(bparam, ops.linear_bias_grad(dy, None, False), fuse, into)
        return dx, dw, db


def native_linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """``F.linear(x, weight, bias)`` on the native kernels (contiguous fp32 GPU tensors, see
    :func:`eligible`; anything else raises)."""
    if not eligible(x, weight, bias):
        raise ValueError('native_linear needs contiguous fp32 GPU tensors below 2 GiB')
    return _NativeLinear.apply(x, weight, bias)


class NativeLinear(nn.Linear):
    """``nn.Linear`` whose GPU fp32 forward and backward run on the native split-bf16 GEMM.

    Same parameters, state-dict keys and constructor.  CPU tensors, other dtypes,
    non-contiguous or oversize operands and ``torch.autocast`` to a lower precision run the
    plain ``nn.Linear.forward``."""

    def forward(self, input: Tensor) -> Tensor:
        if (not input.is_cuda or autocast_lowp('cuda')
                or not eligible(input, self.weight, self.bias)):
            return nn.Linear.forward(self, input)
        # (a GPU tensor without the built extension raises, as every native op does)
        return _NativeLinear.apply(input, self.weight, self.bias)
