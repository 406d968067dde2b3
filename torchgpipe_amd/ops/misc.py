"""Small device utilities: spin kernel (K5), multi-tensor pack/unpack (K6) and the same
with a reduced-precision wire format (``pack_wire`` / ``unpack_wire``, csrc/wire.hip)."""
from typing import Any, List, Optional, Sequence

import torch
from torch import Tensor

from torchgpipe_amd.ops import _ext

__all__ = ['spin', 'pack', 'unpack', 'philox_uniform', 'pack_wire', 'unpack_wire',
           'wire_nbytes']


def spin(seconds: float, device: torch.device) -> None:
    """Enqueue a kernel that busy-waits ``seconds`` of wall time on ``device``'s stream.

    The HIP counterpart of ``torch.cuda._sleep`` used by race-provoking tests
    (reference ``tests/conftest.py:10-26``); it is calibrated in nanoseconds
    (``s_memrealtime`` runs at a constant 100 MHz), so no cycles-per-ms probe
    is needed.
    """
    _ext.require().spin(int(seconds * 1e9), device)


def philox_uniform(n: int, seed: int, offset: int, device: torch.device) -> Tensor:
    return _ext.require().philox_uniform(n, seed, offset, device)


def pack(tensors: Sequence[Tensor], out: Tensor) -> Tensor:
    """Copy ``tensors`` back to back into the flat byte buffer ``out`` (one launch)."""
    views: List[Tensor] = []
    pos = 0
    for t in tensors:
        nbytes = t.numel() * t.element_size()
        views.append(out[pos:pos + nbytes])
        pos = (pos + nbytes + 15) // 16 * 16  # keep every segment 16-byte aligned
    srcs = [t.contiguous().view(-1).view(torch.uint8) for t in tensors]
    if out.is_cuda:
        _ext.require(out).copy_segments(srcs, views)
    else:
        for s, v in zip(srcs, views):
            v.copy_(s)
    return out


def packed_nbytes(tensors: Sequence[Tensor]) -> int:
    pos = 0
    for t in tensors:
        pos = (pos + t.numel() * t.element_size() + 15) // 16 * 16
    return pos


def unpack(buf: Tensor, outs: Sequence[Tensor]) -> None:
    """Inverse of :func:`pack`: scatter the flat buffer into the (contiguous) ``outs``."""
    srcs: List[Tensor] = []
    dsts: List[Tensor] = []
    pos = 0
    for t in outs:
        nbytes = t.numel() * t.element_size()
        srcs.append(buf[pos:pos + nbytes])
        dsts.append(t.view(-1).view(torch.uint8))
        pos = (pos + nbytes + 15) // 16 * 16
    if buf.is_cuda:
        _ext.require(buf).copy_segments(srcs, dsts)
    else:
        for s, d in zip(srcs, dsts):
            d.copy_(s)


# -- wire format ------------------------------------------------------------------------------
# The layout of ``pack`` (segments back to back, each starting on a 16-byte boundary) with
# every float32 tensor stored in ``wire_dtype`` (bfloat16: 2 bytes per element, rounded to
# nearest even); tensors of any other dtype are stored verbatim.  ``wire_dtype=None`` is
# ``pack`` / ``unpack`` / ``packed_nbytes`` themselves.

_COPY, _ENCODE, _DECODE = 0, 1, 2  # csrc/kernels.h WireMode


def _check_wire_dtype(wire_dtype: Optional[torch.dtype]) -> None:
    if wire_dtype is not None and wire_dtype != torch.bfloat16:
        raise ValueError(f'wire_dtype must be None or torch.bfloat16, not {wire_dtype!r}')


def _wire_size(numel: int, dtype: torch.dtype, wire_dtype: Optional[torch.dtype]) -> int:
    if wire_dtype is not None and dtype == torch.float32:
        return numel * wire_dtype.itemsize
    return numel * dtype.itemsize


def wire_nbytes(metas_or_tensors: Sequence[Any], wire_dtype: Optional[torch.dtype]) -> int:
    """Bytes :func:`pack_wire` writes for tensors (or anything with ``shape`` and ``dtype``,
    e.g. ``TensorMeta``) of these shapes and dtypes."""
    _check_wire_dtype(wire_dtype)
    pos = 0
    for m in metas_or_tensors:
        numel = 1
        for d in m.shape:
            numel *= d
        pos = (pos + _wire_size(numel, m.dtype, wire_dtype) + 15) // 16 * 16
    return pos


def pack_wire(tensors: Sequence[Tensor], out: Tensor,
              wire_dtype: Optional[torch.dtype]) -> Tensor:
    """:func:`pack` with every float32 tensor rounded to ``wire_dtype`` on the way (one
    launch per 16 tensors on the GPU; ``Tensor.copy_`` on the CPU, the same bytes)."""
    _check_wire_dtype(wire_dtype)
    if wire_dtype is None:
        return pack(tensors, out)
    srcs: List[Tensor] = []
    views: List[Tensor] = []
    modes: List[int] = []
    pos = 0
    for t in tensors:
        encode = t.dtype == torch.float32
        nbytes = _wire_size(t.numel(), t.dtype, wire_dtype)
        flat = t.contiguous().view(-1)
        srcs.append(flat if encode else flat.view(torch.uint8))
        views.append(out[pos:pos + nbytes])
        modes.append(_ENCODE if encode else _COPY)
        pos = (pos + nbytes + 15) // 16 * 16
    if out.is_cuda:
        if srcs:
            _ext.require(out).wire_segments(srcs, views, modes)
    else:
        for s, v, mode in zip(srcs, views, modes):
            (v.view(wire_dtype) if mode == _ENCODE else v).copy_(s)
    return out


def unpack_wire(buf: Tensor, outs: Sequence[Tensor],
                wire_dtype: Optional[torch.dtype]) -> None:
    """Inverse of :func:`pack_wire`: scatter the wire buffer into the (contiguous) ``outs``,
    widening what was rounded back to float32 (exact)."""
    _check_wire_dtype(wire_dtype)
    if wire_dtype is None:
        unpack(buf, outs)
        return
    srcs: List[Tensor] = []
    dsts: List[Tensor] = []
    modes: List[int] = []
    pos = 0
    for t in outs:
        decode = t.dtype == torch.float32
        nbytes = _wire_size(t.numel(), t.dtype, wire_dtype)
        flat = t.view(-1)
        srcs.append(buf[pos:pos + nbytes])
        dsts.append(flat if decode else flat.view(torch.uint8))
        modes.append(_DECODE if decode else _COPY)
        pos = (pos + nbytes + 15) // 16 * 16
    if buf.is_cuda:
        if srcs:
            _ext.require(buf).wire_segments(srcs, dsts, modes)
    else:
        for s, d, mode in zip(srcs, dsts, modes):
            d.copy_(s.view(wire_dtype) if mode == _DECODE else s)
