"""A decoder-only Transformer language model as a flat ``nn.Sequential`` for ``GPipe``.

Pre-LayerNorm blocks of causal self-attention
(:class:`~torchgpipe_amd.ops.attention.NativeSelfAttention`: the fused fp32 attention kernels
when the head dim is 64 or 128) and a GELU MLP.  Every layer maps one tensor to one tensor, so
any ``balance`` over the ``2 * layers + 2`` children is a valid partition.
"""
from torch import Tensor, nn
import torch

from torchgpipe_amd.ops.attention import NativeSelfAttention
from torchgpipe_amd.ops.layernorm import NativeLayerNorm
from torchgpipe_amd.ops.linear import NativeLinear

__all__ = ['transformer_lm']


class Embedding(nn.Module):
    """Token plus learned position embedding: ``tokens [B, T]`` (int64) -> ``[B, T, d_model]``."""

    def __init__(self, vocab: int, d_model: int, seq_len: int) -> None:
        super().__init__()
        self.token = nn.Embedding(vocab, d_model)
        self.position = nn.Embedding(seq_len, d_model)

    def forward(self, tokens: Tensor) -> Tensor:
        positions = torch.arange(tokens.shape[1], device=tokens.device)
        return self.token(tokens) + self.position(positions)


class AttentionBlock(nn.Module):
    """``x + attention(norm(x))``, causal."""

    def __init__(self, d_model: int, heads: int, native_linear: bool,
                 native_norm: bool = False) -> None:
        super().__init__()
        self.norm = (NativeLayerNorm if native_norm else nn.LayerNorm)(d_model)
        self.attn = NativeSelfAttention(d_model, heads, causal=True,
                                        native_linear=native_linear)

    def forward(self, x: Tensor) -> Tensor:
        return x + self.attn(self.norm(x))


class MLPBlock(nn.Module):
    """``x + fc2(gelu(fc1(norm(x))))`` with a hidden width of ``4 * d_model``."""

    def __init__(self, d_model: int, native_linear: bool, native_norm: bool = False) -> None:
        super().__init__()
        linear = NativeLinear if native_linear else nn.Linear
        self.norm = (NativeLayerNorm if native_norm else nn.LayerNorm)(d_model)
        self.fc1 = linear(d_model, 4 * d_model)
        self.act = nn.GELU()
        self.fc2 = linear(4 * d_model, d_model)

    def forward(self, x: Tensor) -> Tensor:
        return x + self.fc2(self.act(self.fc1(self.norm(x))))


class Head(nn.Module):
    """Final LayerNorm and the vocabulary projection: ``[B, T, d_model]`` -> ``[B, T, vocab]``."""

    def __init__(self, d_model: int, vocab: int, native_linear: bool,
                 native_norm: bool = False) -> None:
        super().__init__()
        self.norm = (NativeLayerNorm if native_norm else nn.LayerNorm)(d_model)
        self.out = (NativeLinear if native_linear else nn.Linear)(d_model, vocab, bias=False)

    def forward(self, x: Tensor) -> Tensor:
        return self.out(self.norm(x))


def transformer_lm(vocab: int = 32000, d_model: int = 768, heads: int = 12, layers: int = 12,
                   seq_len: int = 1024, native_linear: bool = False,
                   native_norm: bool = False) -> nn.Sequential:
    """Embedding, ``layers`` x (attention block, MLP block), head: ``2 * layers + 2`` children
    mapping int64 ``tokens [B, T <= seq_len]`` to logits ``[B, T, vocab]``.

    ``d_model == 64 * heads`` or ``128 * heads`` puts the attention on the native kernels;
    ``native_linear`` builds every projection from ``ops.linear.NativeLinear``, ``native_norm``
    every LayerNorm from ``ops.layernorm.NativeLayerNorm``."""
    blocks = [Embedding(vocab, d_model, seq_len)]
    for _ in range(layers):
        blocks.append(AttentionBlock(d_model, heads, native_linear, native_norm))
        blocks.append(MLPBlock(d_model, native_linear, native_norm))
    blocks.append(Head(d_model, vocab, native_linear, native_norm))
    return nn.Sequential(*blocks)
