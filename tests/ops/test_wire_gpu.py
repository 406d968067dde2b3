"""The HIP wire-format kernel (csrc/wire.hip) against the CPU branch of
``ops.misc.pack_wire`` / ``unpack_wire``, byte for byte: segment sizes around the 8-element
vector step and past one grid sweep, misaligned sources and destinations (the scalar path),
16 and 17 segments (one and two launches), mixed dtypes, and the special values."""
import pytest
import torch

from tests.ops import wire_cases
from torchgpipe_amd.ops import misc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = torch.device('cuda', 0)
FILL = 0x5A
BIG = (1 << 20) + 3  # many blocks and a tail; several grid sweeps as one of 16 segments


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


def _to_dev(t):
    """``t`` (contiguous) on the device at the same offset into its storage as on the host."""
    off = t.storage_offset()
    store = torch.empty(off + t.numel(), dtype=t.dtype, device=DEV)
    view = store[off:].view(t.shape)
    view.copy_(t)
    return view


def _pack_both(tensors, pad=0):
    """The wire buffer of ``tensors`` from the CPU branch and from the kernel (the device
    buffer starting ``pad`` bytes into its storage)."""
    n = misc.wire_nbytes(tensors, BF16)
    want = torch.full((n,), FILL, dtype=torch.uint8)
    misc.pack_wire(tensors, want, BF16)
    store = torch.full((n + pad + 64,), FILL, dtype=torch.uint8, device=DEV)
    got = store[pad:pad + n]
    misc.pack_wire([_to_dev(t) for t in tensors], got, BF16)
    torch.cuda.synchronize()
    # nothing outside the buffer was touched
    assert (store[:pad] == FILL).all() and (store[pad + n:] == FILL).all()
    return want, got.cpu()


def _unpack_both(buf, like, pad=0):
    want = [torch.full_like(t, 3) for t in like]
    misc.unpack_wire(buf, want, BF16)
    store = torch.full((buf.numel() + pad,), FILL, dtype=torch.uint8, device=DEV)
    store[pad:].copy_(buf)
    got = [torch.full_like(t, 3, device=DEV) for t in like]
    misc.unpack_wire(store[pad:], got, BF16)
    torch.cuda.synchronize()
    return want, [t.cpu() for t in got]


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(-1).view(torch.uint8),
                       b.contiguous().view(-1).view(torch.uint8))


@pytest.mark.parametrize('n', [0, 1, 7, 8, 9, 2049, BIG])
def test_segment_sizes(n):
    _gpu()
    x = wire_cases.spread(n, seed=n)
    want, got = _pack_both([x])
    assert torch.equal(got, want)
    want_out, got_out = _unpack_both(want, [x])
    assert _same_bytes(got_out[0], want_out[0])
    assert _same_bytes(got_out[0], x.to(BF16).to(torch.float32))


@pytest.mark.parametrize('n', [1, 9, 2049])
def test_source_four_byte_aligned_only(n):
    """A source view that starts one element into its storage: the scalar path."""
    _gpu()
    base = wire_cases.spread(n + 1, seed=100 + n)
    x = base[1:]
    n_bytes = misc.wire_nbytes([x], BF16)
    want = torch.full((n_bytes,), FILL, dtype=torch.uint8)
    misc.pack_wire([x], want, BF16)
    view = base.to(DEV)[1:]
    assert view.data_ptr() % 16 == 4
    got = torch.full((n_bytes,), FILL, dtype=torch.uint8, device=DEV)
    misc.pack_wire([view], got, BF16)
    assert torch.equal(got.cpu(), want)
    # decode into a destination that is 4-byte aligned only
    out = torch.full((n + 1,), 3.0, device=DEV)
    misc.unpack_wire(got, [out[1:]], BF16)
    assert out[0].item() == 3.0
    assert _same_bytes(out[1:].cpu(), x.to(BF16).to(torch.float32))


@pytest.mark.parametrize('sizes', [(7, 2049), (1, 9, 8), (3, 0, 5)])
def test_segment_after_an_odd_sized_predecessor(sizes):
    """Later segments start on the 16-byte boundary after an odd-sized one; with the wire
    buffer itself 2 bytes into its storage every bf16 side is 2-byte aligned only."""
    _gpu()
    tensors = [wire_cases.spread(n, seed=200 + n) for n in sizes]
    for pad in (0, 2):
        want, got = _pack_both(tensors, pad=pad)
        assert torch.equal(got, want)
        want_out, got_out = _unpack_both(want, tensors, pad=pad)
        for a, b in zip(got_out, want_out):
            assert _same_bytes(a, b)


@pytest.mark.parametrize('count,big', [(16, 0), (17, 0), (16, BIG)])
def test_segment_counts(count, big):
    """16 segments: one launch; 17: two.  With a large segment among 16 the launch's blocks
    are shared out, so that segment takes several sweeps of the grid-stride loop."""
    _gpu()
    tensors = [wire_cases.spread(5 + 3 * k, seed=300 + k) for k in range(count)]
    if big:
        tensors[5] = wire_cases.spread(big, seed=399)
    want, got = _pack_both(tensors)
    assert torch.equal(got, want)
    want_out, got_out = _unpack_both(want, tensors)
    for a, b in zip(got_out, want_out):
        assert _same_bytes(a, b)


def test_mixed_dtypes():
    _gpu()
    tensors = wire_cases.mixed()
    want, got = _pack_both(tensors)
    assert torch.equal(got, want)
    want_out, got_out = _unpack_both(want, tensors)
    for t, a, b in zip(tensors, got_out, want_out):
        assert a.dtype == t.dtype and _same_bytes(a, b)
        if t.dtype != torch.float32:
            assert _same_bytes(a, t)


def test_special_values():
    _gpu()
    x = wire_cases.special_values()
    for tensors in ([x], [x[1:]], [x[:3], x]):  # vector path, scalar path, tail
        want, got = _pack_both(tensors)
        assert torch.equal(got, want)
        _, got_out = _unpack_both(want, tensors)
        for t, a in zip(tensors, got_out):
            assert _same_bytes(a, t.to(BF16).to(torch.float32))
    _, got = _pack_both([x])
    by_bits = dict(zip(wire_cases.SPECIAL_BITS,
                       (got[:2 * x.numel()].view(torch.int16).to(torch.int32) & 0xffff).tolist()))
    assert by_bits[0x00000000] == 0x0000 and by_bits[0x80000000] == 0x8000
    assert by_bits[0x00000001] == 0x0000          # the smallest subnormal
    assert by_bits[0x3f808000] == 0x3f80          # 1 + 2^-8: tie, down to even
    assert by_bits[0x3f818000] == 0x3f82          # 1 + 3 * 2^-8: tie, up to even
    assert by_bits[0x7f7fffff] == 0x7f80          # the largest fp32 becomes inf
    assert by_bits[0x7f800000] == 0x7f80 and by_bits[0xff800000] == 0xff80


def test_nan_stays_nan():
    _gpu()
    x = wire_cases.nan_values()
    for src in (x, torch.cat([x, x])[1:]):  # the tail alone; a vector step and a tail
        n = misc.wire_nbytes([src], BF16)
        buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
        misc.pack_wire([src.to(DEV)], buf, BF16)
        out = torch.zeros(src.numel(), device=DEV)
        misc.unpack_wire(buf, [out], BF16)
        assert torch.isnan(out).all()
        assert torch.isnan(buf[:2 * src.numel()].view(BF16)).all()


def test_empty_lists_and_bad_segments():
    _gpu()
    buf = torch.full((32,), FILL, dtype=torch.uint8, device=DEV)
    misc.pack_wire([], buf, BF16)
    misc.unpack_wire(buf, [], BF16)
    misc.pack_wire([torch.empty(0, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV)],
                   buf, BF16)
    assert (buf == FILL).all()
    from torchgpipe_amd.ops import _ext
    ops = _ext.require(buf)
    x = torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError):  # an encode's destination holds 2 bytes per element
        ops.wire_segments([x], [buf[:32]], [1])
    with pytest.raises(RuntimeError):  # a decode's source too
        ops.wire_segments([buf[:32]], [x], [2])
    with pytest.raises(RuntimeError):  # bf16 side on an odd address
        ops.wire_segments([x], [torch.empty(33, dtype=torch.uint8, device=DEV)[1:17]], [1])
    with pytest.raises(RuntimeError):  # one device
        ops.wire_segments([x], [torch.empty(16, dtype=torch.uint8)], [1])
    with pytest.raises(RuntimeError):
        ops.wire_segments([x], [buf[:16]], [7])
