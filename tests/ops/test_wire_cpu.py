"""The wire format of inter-stage messages on the CPU (``ops.misc.pack_wire`` /
``unpack_wire`` / ``wire_nbytes``): the branch gloo CPU ranks run, and the oracle of the
HIP kernel's bytes (``test_wire_gpu.py``)."""
import pytest
import torch

from tests.ops import wire_cases
from torchgpipe_amd.ops import misc

BF16 = torch.bfloat16


def roundtrip(tensors, wire_dtype=BF16):
    n = misc.wire_nbytes(tensors, wire_dtype)
    buf = torch.full((n,), 0xAB, dtype=torch.uint8)
    misc.pack_wire(tensors, buf, wire_dtype)
    outs = [torch.empty_like(t) for t in tensors]
    misc.unpack_wire(buf, outs, wire_dtype)
    return buf, outs


@pytest.mark.parametrize('n', [0, 1, 7, 8, 9, 2049])
def test_roundtrip_is_bf16_rounding(n):
    x = wire_cases.spread(n, seed=n)
    _, (y,) = roundtrip([x])
    want = x.to(BF16).to(torch.float32)
    assert y.dtype == torch.float32 and y.shape == x.shape
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))


def test_special_values():
    x = wire_cases.special_values()
    buf, (y,) = roundtrip([x])
    want = x.to(BF16)
    assert torch.equal(buf[:2 * x.numel()].view(torch.int16), want.view(torch.int16))
    assert torch.equal(y.view(torch.int32), want.to(torch.float32).view(torch.int32))
    # what the format promises, stated without torch's cast
    by_bits = dict(zip(wire_cases.SPECIAL_BITS, y.view(torch.int32).tolist()))
    assert by_bits[0x3f808000] == 0x3f800000  # 1 + 2^-8: tie, down to even
    assert by_bits[0x3f818000] == 0x3f820000  # 1 + 3 * 2^-8: tie, up to even
    assert by_bits[0x7f7fffff] == 0x7f800000  # past the largest bf16: inf
    assert by_bits[0x00000001] == 0 and by_bits[0x00000000] == 0
    assert by_bits[0x80000000] == -2 ** 31  # -0 keeps its sign
    _, (n,) = roundtrip([wire_cases.nan_values()])
    assert torch.isnan(n).all()


def test_mixed_message_leaves_other_dtypes_alone():
    tensors = wire_cases.mixed()
    buf, outs = roundtrip(tensors)
    for t, o in zip(tensors, outs):
        assert o.dtype == t.dtype and o.shape == t.shape
        if t.dtype == torch.float32:
            assert torch.equal(o, t.to(BF16).to(torch.float32))
        else:
            assert torch.equal(o.view(torch.uint8), t.view(torch.uint8))
    # the layout: 16-byte aligned segments, 2 bytes per fp32 element
    sizes = [2 * 15, 8 * 7, 2 * 9, 11, 2 * 8]
    pos = 0
    for t, size in zip(tensors, sizes):
        seg = buf[pos:pos + size]
        want = t.to(BF16) if t.dtype == torch.float32 else t
        assert torch.equal(seg, want.contiguous().view(-1).view(torch.uint8))
        pos = (pos + size + 15) // 16 * 16
    assert pos == buf.numel() == misc.wire_nbytes(tensors, BF16)


def test_wire_nbytes_matches_the_buffer_written():
    tensors = wire_cases.mixed(1)
    n = misc.wire_nbytes(tensors, BF16)
    buf = torch.zeros(n + 64, dtype=torch.uint8)
    buf[n:] = 0xCD
    misc.pack_wire(tensors, buf, BF16)
    assert (buf[n:] == 0xCD).all()
    end = buf[:n].nonzero().max().item()
    assert n - 16 <= end < n  # the last segment ends in the buffer's last 16 bytes
    # shapes and dtypes alone decide it
    from torchgpipe_amd.parallel.p2p import TensorMeta
    assert misc.wire_nbytes([TensorMeta.of(t) for t in tensors], BF16) == n
    assert misc.wire_nbytes([], BF16) == 0


def test_none_is_pack_byte_for_byte():
    tensors = wire_cases.mixed(2)
    n = misc.packed_nbytes(tensors)
    assert misc.wire_nbytes(tensors, None) == n
    a = torch.full((n,), 0x11, dtype=torch.uint8)
    b = torch.full((n,), 0x11, dtype=torch.uint8)
    misc.pack(tensors, a)
    misc.pack_wire(tensors, b, None)
    assert torch.equal(a, b)
    outs_a = [torch.empty_like(t) for t in tensors]
    outs_b = [torch.empty_like(t) for t in tensors]
    misc.unpack(a, outs_a)
    misc.unpack_wire(b, outs_b, None)
    for t, x, y in zip(tensors, outs_a, outs_b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        assert torch.equal(x.view(torch.uint8), t.view(torch.uint8))


def test_only_bfloat16_is_a_wire_dtype():
    x = torch.zeros(4)
    for bad in (torch.float16, torch.float32, torch.int8):
        with pytest.raises(ValueError):
            misc.wire_nbytes([x], bad)
        with pytest.raises(ValueError):
            misc.pack_wire([x], torch.empty(16, dtype=torch.uint8), bad)
        with pytest.raises(ValueError):
            misc.unpack_wire(torch.empty(16, dtype=torch.uint8), [x], bad)
