"""``nn.LayerNorm`` / ``nn.RMSNorm`` over the last dimension on the native kernels
(``csrc/layernorm.hip``), opt-in.

Forward: a row stays in registers between its one global read and its one global write
(a wave per row up to 1024 columns, a workgroup per row up to 8192); the
statistics are two-pass on the registers.  Backward: one persistent pass over ``dy`` and ``x``
that writes ``dx`` and per-workgroup partials of the affine gradients, and a small fixed-order
reduction that stores them or, under the :mod:`~torchgpipe_amd.ops.gradacc` protocol, adds them
straight into ``.grad``.  No atomics: the same inputs give the same bits.

:class:`NativeLayerNorm` and :class:`NativeRMSNorm` are drop-in replacements; nothing routes
to them by default (``models.transformer_lm(native_norm=True)`` builds its three LayerNorm
sites from the former).
"""
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from torchgpipe_amd.ops import _ext
from torchgpipe_amd.ops.gradacc import _settle, target
from torchgpipe_amd.ops.precision import autocast_lowp

__all__ = ['native_layer_norm', 'native_rms_norm', 'NativeLayerNorm', 'NativeRMSNorm',
           'eligible', 'MAX_WIDTH']

MAX_WIDTH = 8192         # the widest row the kernels hold in registers
_MAX_BYTES = 0x7ffffff0  # buffer-resource offsets: every tensor below 2 GiB

Shape = Union[int, Sequence[int]]


# -- test / profiling hooks (not public) ------------------------------------------------------

def _wave_row_max() -> int:
    """The widest row of the wave-per-row instance; wider rows take a workgroup each."""
    return int(_ext.require()._layernorm_limits(1)[0])


def _backward_sweep_rows(width: int) -> int:
    """Rows that one sweep of the persistent backward grid covers at this row width."""
    return int(_ext.require()._layernorm_limits(width)[1])


def _force_instance(wide: int = -1) -> None:
    """``0`` runs the wave-per-row instance wherever it has the registers (rows up to 2048),
    ``1`` the workgroup-per-row instance everywhere; ``-1`` restores the host rule."""
    _ext.require()._layernorm_force_instance(wide)


def _last_dim_only(normalized_shape: Shape) -> Optional[int]:
    if isinstance(normalized_shape, int):
        return normalized_shape
    shape = tuple(normalized_shape)
    return int(shape[0]) if len(shape) == 1 else None


def eligible(x: Tensor, normalized_shape: Shape, weight: Optional[Tensor] = None,
             bias: Optional[Tensor] = None) -> bool:
    """Whether the native kernels take this call: fp32 GPU tensors on one device, a contiguous
    ``x`` of at least one row, normalisation over the last dimension only, rows of at most
    :data:`MAX_WIDTH` elements, and every tensor below 2 GiB."""
    width = _last_dim_only(normalized_shape)
    if width is None or x.dim() < 1 or x.shape[-1] != width or not 1 <= width <= MAX_WIDTH:
        return False
    tensors = [x] + [t for t in (weight, bias) if t is not None]
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               and t.device == x.device for t in tensors):
        return False
    if any(t.shape != (width,) for t in tensors[1:]):
        return False
    return x.numel() > 0 and 4 * x.numel() <= _MAX_BYTES


class _NativeNorm(torch.autograd.Function):
    """The two native ops under autograd; gradient accumulation as ``_NativeLinear``."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Optional[Tensor],  # type: ignore[override]
                bias: Optional[Tensor], eps: float, rms: bool) -> Tensor:
        y, mean, rstd = _ext.require(x).layernorm_forward(x, weight, bias, eps, rms)
        ctx.save_for_backward(x, mean, rstd, weight)
        ctx.params = (weight, bias)
        ctx.rms = rms
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):  # type: ignore[override]
        x, mean, rstd, weight = ctx.saved_tensors
        wparam, bparam = ctx.params
        ctx.params = (None, None)  # a repeated backward (retain_graph) returns them instead
        need = ctx.needs_input_grad
        need_w = weight is not None and need[1]
        need_b = need[2]  # (a bias only comes with a weight, and never with rms)
        fuse_w, into_w = target(wparam) if need_w else (False, None)
        fuse_b, into_b = target(bparam) if need_b else (False, None)
        # a given `into` is added to by the reduction kernel; the others come back fresh
        dx, dw, db = _ext.require(dy).layernorm_backward(
            dy.contiguous(), x, mean, rstd, weight, into_w, into_b, True, need[0], ctx.rms,
            need_w, need_b)
        dw = None if into_w is not None else _settle(wparam, dw, fuse_w, None)
        db = None if into_b is not None else _settle(bparam, db, fuse_b, None)
        return dx, dw, db, None, None


def _check(x: Tensor, normalized_shape: Shape, weight: Optional[Tensor],
           bias: Optional[Tensor], name: str) -> None:
    if not eligible(x, normalized_shape, weight, bias):
        raise ValueError(f'{name} needs fp32 GPU tensors on one device, a contiguous x and '
                         f'normalisation over a last dimension of at most {MAX_WIDTH}')


def native_layer_norm(x: Tensor, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                      eps: float = 1e-5) -> Tensor:
    """``F.layer_norm(x, x.shape[-1:], weight, bias, eps)`` on the native kernels (see
    :func:`eligible`; anything else raises, as does a bias without a weight)."""
    _check(x, x.shape[-1:], weight, bias, 'native_layer_norm')
    if weight is None and bias is not None:
        raise ValueError('native_layer_norm takes a bias only together with a weight')
    return _NativeNorm.apply(x, weight, bias, eps, False)


def native_rms_norm(x: Tensor, weight: Optional[Tensor] = None,
                    eps: Optional[float] = None) -> Tensor:
    """``F.rms_norm(x, x.shape[-1:], weight, eps)`` on the native kernels (see
    :func:`eligible`; anything else raises)."""
    _check(x, x.shape[-1:], weight, None, 'native_rms_norm')
    return _NativeNorm.apply(x, weight, None, _rms_eps(eps), True)


def _rms_eps(eps: Optional[float]) -> float:
    return torch.finfo(torch.float32).eps if eps is None else eps


def _native(x: Tensor, normalized_shape: Tuple[int, ...], weight: Optional[Tensor],
            bias: Optional[Tensor]) -> bool:
    return (x.is_cuda and not autocast_lowp('cuda')
            and eligible(x, normalized_shape, weight, bias))


class NativeLayerNorm(nn.LayerNorm):
    """``nn.LayerNorm`` whose GPU fp32 forward and backward run on the native kernels.

    Same parameters, state-dict keys and constructor.  CPU tensors, other dtypes, a
    multi-dimensional ``normalized_shape``, rows wider than :data:`MAX_WIDTH`, non-contiguous
    or oversize inputs and ``torch.autocast`` to a lower precision run the plain
    ``nn.LayerNorm.forward``."""

    def forward(self, input: Tensor) -> Tensor:
        if not _native(input, self.normalized_shape, self.weight, self.bias):
            return nn.LayerNorm.forward(self, input)
        # (a GPU tensor without the built extension raises, as every native op does)
        return _NativeNorm.apply(input, self.weight, self.bias, self.eps, False)


class NativeRMSNorm(nn.RMSNorm):
    """``nn.RMSNorm`` on the native kernels; falls back as :class:`NativeLayerNorm` does."""

    def forward(self, x: Tensor) -> Tensor:
        if not _native(x, self.normalized_shape, self.weight, None):
            return nn.RMSNorm.forward(self, x)
        return _NativeNorm.apply(x, self.weight, None, _rms_eps(self.eps), True)
