"""Opt-in reduced fp32 precision of the split-bf16 convolution kernels.

The implicit-GEMM tile configurations 7-11 (``csrc/conv_gemm.hip``) and the batched-GEMM
Winograd kernel (``bg_gemm_emu_kernel``, ``csrc/winograd_f4.hip``) emulate an fp32 product
on the bf16 matrix pipes: each operand is split exactly into three bf16 parts
``hi + mid + lo`` and a product is six partial products.  At the reduced levels the fused
F(4x4) Winograd forward / backward-data of the 64-256-channel 3x3 layers runs on them too
(``f4_conv_emu_kernel``, the three ``'high'`` products; ``ops.conv.f4_variant`` routes).
The levels are those of :func:`torch.set_float32_matmul_precision`:

``'highest'`` (default)
    all six partial products: fp32 error bounds.
``'high'``
    ``hi*hi + hi*mid + mid*hi`` ("bf16x3"): at worst ``3 * 2**-18`` relative per product,
    half the MFMA work, two thirds of the LDS fragment traffic.
``'medium'``
    ``hi*hi``: bf16 operands, fp32 accumulation; ``2**-8`` per product, one sixth of the
    MFMA work.  The Winograd kernels run ``'high'`` at this level (plain bf16 operands
    lose too much in the transform domain).

The level is process-wide and read when a kernel is launched: a captured graph keeps the
level it was captured at.  Set it before building ``GPipe`` / ``PipelineStage`` and do not
change it inside a step (checkpoint recomputation must see the forward's level).  The f32
MFMA configurations 0-6, the fused Winograd weight gradient of the 64/128-channel layers,
the fused forward / backward-data kernels outside the routed shape classes
(``ops.conv.f4_emu_faster``) and every library (MIOpen) path compute as before at every
level; so do CPU tensors.  The level does
not follow :func:`torch.get_float32_matmul_precision`.

``split_bf16`` and the ``reference_*`` functions are the fp64 oracle of these semantics.
"""
import contextlib
from typing import Iterator, Sequence, Tuple, Union

import torch
from torch import Tensor
import torch.nn.functional as F

__all__ = ['LEVELS', 'set_conv_precision', 'get_conv_precision', 'conv_precision',
           'autocast_lowp', 'split_bf16', 'reference_conv2d', 'reference_conv2d_backward']

LEVELS = ('highest', 'high', 'medium')

_level = 0

_Pair = Union[int, Sequence[int]]


def _index(level: str) -> int:
    if not isinstance(level, str) or level not in LEVELS:
        raise ValueError(f'conv precision must be one of {LEVELS}, got {level!r}')
    return LEVELS.index(level)


def _push() -> None:
    """Hand the level to the native extension (called when it loads and on every set)."""
    from torchgpipe_amd.ops import _ext
    if _ext.loaded():
        torch.ops.tgpipe.conv_precision(_level)


def set_conv_precision(level: str) -> None:
    """Set the process-wide level: ``'highest'``, ``'high'`` or ``'medium'``."""
    global _level
    _level = _index(level)
    _push()


def get_conv_precision() -> str:
    return LEVELS[_level]


@contextlib.contextmanager
def conv_precision(level: str) -> Iterator[None]:
    """Run the body at ``level`` and restore the level in force before."""
    before = get_conv_precision()
    set_conv_precision(level)
    try:
        yield
    finally:
        set_conv_precision(before)


def autocast_lowp(device_type: str) -> bool:
    """Whether ``torch.autocast`` is enabled on this thread for ``device_type`` with a dtype
    other than fp32.  The native fp32 ops that replace an ATen op on autocast's
    lower-precision list (convolutions, linear) step aside when it is: their modules run
    the plain ``nn`` forward, which ATen casts.  ``set_conv_precision`` has no say there."""
    return torch.is_autocast_enabled(device_type) and \
        torch.get_autocast_dtype(device_type) != torch.float32


def split_bf16(t: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """``t == hi + mid + lo`` exactly, each part a bf16 value held in fp32 (round to nearest,
    as the kernels split)."""
    t = t.float()
    hi = t.bfloat16().float()
    r = t - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi, mid, lo


def _conv(x: Tensor, w: Tensor, stride: _Pair, padding: _Pair) -> Tensor:
    return F.conv2d(x.double(), w.double(), stride=stride, padding=padding)


def reference_conv2d(x: Tensor, w: Tensor, stride: _Pair = 1, padding: _Pair = 0,
                     level: str = 'highest', relu: bool = False) -> Tensor:
    """fp64 ``conv2d(relu?(x), w)`` with the partial products of ``level``."""
    lv = _index(level)
    x = x.detach()
    w = w.detach()
    if relu:
        x = F.relu(x)
    if lv == 0:
        return _conv(x, w, stride, padding)
    xh, xm, _ = split_bf16(x)
    wh, wm, _ = split_bf16(w)
    if lv == 2:
        return _conv(xh, wh, stride, padding)
    return _conv(xh, wh.double() + wm.double(), stride, padding) + _conv(xm, wh, stride, padding)


def reference_conv2d_backward(dz: Tensor, x: Tensor, w: Tensor, stride: _Pair = 1,
                              padding: _Pair = 0, level: str = 'highest',
                              relu: bool = False) -> Tuple[Tensor, Tensor]:
    """fp64 ``(dx, dw)`` of ``conv2d(relu?(x), w)`` for the output gradient ``dz``: dX from
    the parts of dZ and W, dW from the parts of dZ and relu?(X)."""
    lv = _index(level)
    dz, x, w = dz.detach(), x.detach(), w.detach()
    xr = F.relu(x) if relu else x

    def dgrad(g: Tensor, wt: Tensor) -> Tensor:
        return torch.nn.grad.conv2d_input(x.shape, wt.double(), g.double(), stride=stride,
                                          padding=padding)

    def wgrad(g: Tensor, inp: Tensor) -> Tensor:
        return torch.nn.grad.conv2d_weight(inp.double(), w.shape, g.double(), stride=stride,
                                           padding=padding)

    if lv == 0:
        dx, dw = dgrad(dz, w), wgrad(dz, xr)
    else:
        gh, gm, _ = split_bf16(dz)
        wh, wm, _ = split_bf16(w)
        xh, xm, _ = split_bf16(xr)
        if lv == 2:
            dx, dw = dgrad(gh, wh), wgrad(gh, xh)
        else:
            dx = dgrad(gh, wh.double() + wm.double()) + dgrad(gm, wh)
            dw = wgrad(gh, xh.double() + xm.double()) + wgrad(gm, xh)
    if relu:
        dx = dx * (x > 0).double()
    return dx, dw
