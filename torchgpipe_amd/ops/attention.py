"""Fused fp32 scaled-dot-product attention for head dims 64 and 128 (``csrc/attention.hip``,
``csrc/attention128.hip``), opt-in.

``softmax(scale * q k^T [+ causal mask]) v`` without the ``T x T`` score matrix in memory,
forward and backward, as split-bf16 partial products on ``v_mfma_f32_32x32x16_bf16`` with
f32 accumulators -- the arithmetic of the native convolutions and of
:class:`~torchgpipe_amd.ops.linear.NativeLinear`.  The level of
:func:`~torchgpipe_amd.ops.precision.set_conv_precision` governs every GEMM of both passes
(``'highest'`` six partial products, ``'high'`` three, ``'medium'`` ``hi*hi``); the softmax
itself is fp32.  The backward recomputes the scores from the saved ``logsumexp`` and uses no
atomics: two calls with the same inputs give the same bits.

:class:`NativeSelfAttention` is a self-attention layer on these kernels (one fused qkv
projection whose output the kernels read in place, attention, output projection);
``models.transformer.transformer_lm`` is built from it.
"""
import math
from typing import Optional

import torch
from torch import Tensor, nn
import torch.nn.functional as F

from torchgpipe_amd.ops import _ext
from torchgpipe_amd.ops.linear import NativeLinear
from torchgpipe_amd.ops.precision import autocast_lowp

__all__ = ['native_attention', 'NativeSelfAttention', 'eligible', 'HEAD_DIM', 'HEAD_DIMS']

HEAD_DIM = 64          # the first head dim the kernels had; kept for its importers
HEAD_DIMS = (64, 128)  # every head dim with kernels
_MAX_BYTES = 0x7ffffff0  # buffer-resource offsets: every view spans less than 2 GiB


def _readable(t: Tensor) -> bool:
    """The kernels' stride rules for one ``[B, H, T, D]`` view."""
    strides = [0 if n == 1 else s for n, s in zip(t.shape[:3], t.stride()[:3])]
    span = sum((n - 1) * s for n, s in zip(t.shape[:3], strides)) + t.shape[3]
    return (t.stride(3) == 1 and all(s % 4 == 0 for s in strides)
            and t.data_ptr() % 16 == 0 and 4 * span <= _MAX_BYTES)


def eligible(q: Tensor, k: Tensor, v: Tensor) -> bool:
    """Whether the native kernels take this call: fp32 GPU tensors on one device of one shape
    ``[B, H, T, D]`` with ``D`` in :data:`HEAD_DIMS` and ``T >= 1``, last stride 1, the other
    strides multiples of 4 elements, 16-byte aligned, each view spanning less than 2 GiB."""
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == q.device
               and t.shape == q.shape for t in (q, k, v)):
        return False
    if q.dim() != 4 or q.shape[3] not in HEAD_DIMS or q.numel() == 0:
        return False
    return all(_readable(t) for t in (q, k, v))


class _NativeAttention(torch.autograd.Function):

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor,  # type: ignore[override]
                causal: bool, scale: float) -> Tensor:
        o, lse = _ext.require(q).attention_forward(q, k, v, causal, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale = causal, scale
        return o

    @staticmethod
    def backward(ctx, do: Tensor):  # type: ignore[override]
        q, k, v, o, lse = ctx.saved_tensors
        if not _readable(do):
            do = do.contiguous()
        dq, dk, dv = _ext.require(do).attention_backward(do, q, k, v, o, lse, ctx.causal,
                                                         ctx.scale)
        return dq, dk, dv, None, None


def native_attention(q: Tensor, k: Tensor, v: Tensor, causal: bool = False,
                     scale: Optional[float] = None) -> Tensor:
    """``F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale)`` on the native
    kernels (see :func:`eligible`; anything else raises).  ``scale`` defaults to
    ``1 / sqrt(D)``.  The result is ``[B, T, H, D]`` memory viewed as ``[B, H, T, D]``, and so
    are the gradients."""
    if not eligible(q, k, v):
        raise ValueError('native_attention needs fp32 GPU tensors [B, H, T, 64 or 128] of one '
                         'shape with last stride 1 and 16-byte aligned rows')
    scale = 1.0 / math.sqrt(q.shape[3]) if scale is None else float(scale)
    return _NativeAttention.apply(q, k, v, bool(causal), scale)


class NativeSelfAttention(nn.Module):
    """Multi-head self-attention over ``x [B, T, embed_dim]``: one fused projection ``qkv``,
    attention per head, the output projection ``proj``.

    With head dim 64 or 128 a GPU fp32 call runs the native kernels: they read q, k, v as slices
    of the ``[B, T, 3, H, D]`` projection output and write ``[B, T, H, D]``, which ``proj``
    reads as it is -- no transpose copies.  CPU tensors, ``torch.autocast`` to a lower
    precision, other head dims and ineligible strides run
    ``F.scaled_dot_product_attention`` on the same parameters.  ``native_linear`` builds the
    two projections from :class:`~torchgpipe_amd.ops.linear.NativeLinear`."""

    def __init__(self, embed_dim: int, num_heads: int, causal: bool = False, bias: bool = True,
                 native_linear: bool = False) -> None:
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError('embed_dim must be a multiple of num_heads')
        self.embed_dim, self.num_heads, self.causal = embed_dim, num_heads, causal
        linear = NativeLinear if native_linear else nn.Linear
        self.qkv = linear(embed_dim, 3 * embed_dim, bias=bias)
        self.proj = linear(embed_dim, embed_dim, bias=bias)

    def forward(self, x: Tensor) -> Tensor:
        b, t, _ = x.shape
        qkv = self.qkv(x).view(b, t, 3, self.num_heads, self.embed_dim // self.num_heads)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        if x.is_cuda and not autocast_lowp('cuda') and eligible(q, k, v):
            # (a GPU tensor without the built extension raises, as every native op does)
            o = native_attention(q, k, v, self.causal)
        else:
            o = F.scaled_dot_product_attention(q, k, v, is_causal=self.causal)
        return self.proj(o.transpose(1, 2).reshape(b, t, self.embed_dim))
