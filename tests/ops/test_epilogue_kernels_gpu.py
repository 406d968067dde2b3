"""Edges of the kernels around the matrix-core ones (GPU only): DropNormAct, elementwise
dropout and the Philox draws, pack / unpack (``csrc/kernels.hip``), and ``up2x_cat``,
``MaxPool2x2`` and ``add_relu`` (``csrc/unet_ops.hip``).

DropNormAct is held to fp64 by a bound that moves with the inputs: the kernel's largest
error may be 8x that of the project's own fp32 composite (``fused._composite`` on the CPU,
with autograd) on the same tensors, plus 1e-7.  Two correct fp32 implementations that sum
in different orders stay inside the factor 8; an unbiased variance, a one-pass variance or
a plane leaking into its neighbour's reduction do not.  The inputs and the case tables come
from ``epilogue_cases.py``; run with ``-s`` to see each case's kernel error, composite
error and their ratio.

The factor 8 was fixed before the kernels were first measured against it.  Largest kernel /
composite ratios then measured on an MI355X, per tile (float4 and scalar instances, training
and eval together):

    tile        y      dx     mean   rstd
    (16,1)      2.03   2.35   1.34   1.29
    (64,1)      2.43   1.70   2.57   2.14
    (64,3)      2.02   1.87   0.81   2.61
    (64,9)      1.91   1.73   1.55   1.49
    (256,9)     1.75   1.38   1.17   6.42   (rstd: 1.3e-8 against 2.0e-9, under the 1e-7 floor)
    (1024,9)    2.97   1.25   5.12   1.37   (mean: 1.28e-5 against 2.49e-6 at mean = 100 sigma)
    streaming   1.26   1.00   4.92   1.32   (mean: 1.98e-7 against 4.03e-8)

The two large ``mean`` ratios are the sums' order: the kernel adds 36 values per lane in a
row before its tree, ATen's CPU sum is pairwise throughout.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.ops import epilogue_cases as ec
from torchgpipe_amd.ops import _ext, fused, fusion, misc, philox
from torchgpipe_amd.ops import dropout as dropout_ops
from torchgpipe_amd.ops.fused import _signed64
from torchgpipe_amd.ops.unet_ops import MaxPool2x2, up2x_cat

pytestmark = pytest.mark.gpu

cuda = torch.device('cuda', 0)
FACTOR = 8.0
FLOOR = 1e-7


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


def ops():
    return torch.ops.tgpipe


def misaligned(t):
    """A contiguous GPU copy of ``t`` that starts one element past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=cuda)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous()
    assert t.numel() == 0 or view.data_ptr() % 16 == t.element_size() % 16
    return view


# ---------------------------------------------------------------------------------------------
# DropNormAct
# ---------------------------------------------------------------------------------------------
class Errors:
    """Collects ``kernel error <= 8 * composite error + 1e-7`` checks, prints every figure,
    then asserts them together (so a failing case still shows all of its numbers)."""

    def __init__(self, label):
        self.label = label
        self.rows = []

    def add(self, name, got, want64, plain32):
        kernel = (got.detach().double().cpu().reshape(want64.shape) - want64).abs().max().item()
        plain = (plain32.detach().double().reshape(want64.shape) - want64).abs().max().item()
        ratio = kernel / plain if plain > 0 else (0.0 if kernel == 0 else float('inf'))
        print(f'DNA {self.label} {name}: kernel={kernel:.3e} composite={plain:.3e} '
              f'ratio={ratio:.2f}')
        self.rows.append((name, kernel, plain))

    def check(self):
        for name, kernel, plain in self.rows:
            assert kernel <= FACTOR * plain + FLOOR, \
                f'{self.label} {name}: kernel error {kernel:.3e} > 8 * {plain:.3e} + 1e-7'


def reference_margin(y64, scale):
    """Smallest ``|z|`` of the fp64 reference itself (``y64`` with the LeakyReLU undone) on
    the planes ``scale`` keeps."""
    z = torch.where(y64 > 0, y64, y64 / ec.SLOPE).abs().reshape(scale.numel(), -1)
    kept = scale > 0
    return z[kept].min().item() if kept.any() else float('inf')


def dna(case, training, x, dy):
    """Forward and backward straight on the ops: ``(y, dx, mean, rstd, scale)``."""
    y, mean, rstd, scale = ops().dna_forward(x, ec.P, ec.EPS, ec.SLOPE, _signed64(case.seed),
                                             _signed64(case.offset), training, None)
    dx = ops().dna_backward(dy, x, mean, rstd, scale, ec.SLOPE)
    return y, dx, mean, rstd, scale


def check_against_fp64(case, training, label, y, dx, mean, rstd, scale, x, dy):
    """Everything the fp64 reference says about one run on the CPU inputs ``(x, dy)``."""
    want_scale = ec.plane_scale(case, training)
    y64, dx64, y32, dx32 = ec.reference(case, x, dy, training)
    assert reference_margin(y64, want_scale) >= ec.MARGIN
    mean64, rstd64, mean32, rstd32 = ec.reference_stats(case, x, training)
    errors = Errors(f'{case.name} {"train" if training else "eval"} {label}')
    errors.add('y', y, y64, y32)
    errors.add('dx', dx, dx64, dx32)
    errors.add('mean', mean, mean64, mean32)
    # (a dropped plane's rstd is eps^-1/2 = 316, a kept one's about 1 / std: each kind is
    # held to the composite's error on its own kind, the small ones not to the large ones')
    dropped = want_scale == 0
    for name, chosen in (('rstd-kept', ~dropped), ('rstd-dropped', dropped)):
        if chosen.any():
            errors.add(name, rstd.cpu()[chosen], rstd64[chosen], rstd32[chosen])
    # the Dropout2d draw is exact, and a dropped plane is exactly zero
    assert torch.equal(scale.cpu(), want_scale)
    planes = case.num_planes
    assert (y.detach().cpu().view(planes, -1)[dropped] == 0).all()
    assert (dx.detach().cpu().view(planes, -1)[dropped] == 0).all()
    assert (y64.view(planes, -1)[dropped] == 0).all()
    assert (dx64.view(planes, -1)[dropped] == 0).all()
    errors.check()


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('case', ec.TABLE, ids=[c.name for c in ec.TABLE])
def test_drop_norm_act_matches_fp64(case, training):
    x, dy = ec.make_input(case)
    seed, offset = _signed64(case.seed), _signed64(case.offset)
    xg = x.to(cuda).requires_grad_(True)
    y = fused._DropNormAct.apply(xg, ec.P, ec.EPS, ec.SLOPE, seed, offset, training)
    y.backward(dy.to(cuda))
    _, mean, rstd, scale = ops().dna_forward(xg.detach(), ec.P, ec.EPS, ec.SLOPE, seed, offset,
                                             training, None)
    check_against_fp64(case, training, ec.instance(case.s), y, xg.grad, mean, rstd, scale, x, dy)


@pytest.mark.parametrize('which', ['x', 'dy'])
@pytest.mark.parametrize('case', ec.ALIGNMENT, ids=[c.name for c in ec.ALIGNMENT])
def test_drop_norm_act_misaligned_pointer(case, which):
    """``x`` off a 16-byte boundary: the scalar instance forward and backward on a plane
    size that otherwise takes float4.  Only ``dy`` off it: float4 forward, scalar backward."""
    x, dy = ec.make_input(case)
    xa, dya = x.to(cuda), dy.to(cuda)
    assert xa.data_ptr() % 16 == 0 and dya.data_ptr() % 16 == 0
    xk = misaligned(xa) if which == 'x' else xa
    dyk = misaligned(dya) if which == 'dy' else dya
    y, dx, mean, rstd, scale = dna(case, True, xk, dyk)
    aligned = dna(case, True, xa, dya)
    assert torch.equal(scale, aligned[4])
    label = f'{which}-misaligned {ec.instance(case.s, aligned=False)}'
    check_against_fp64(case, True, label, y, dx, mean, rstd, scale, x, dy)


@pytest.mark.parametrize('poison', ['finite', 'nan'])
@pytest.mark.parametrize('victim', ['kept', 'dropped'])
@pytest.mark.parametrize('case', ec.ISOLATION, ids=[c.name for c in ec.ISOLATION])
def test_drop_norm_act_planes_are_isolated(case, victim, poison):
    """The 16 (S = 36) or 4 (S = 576) planes of a workgroup share nothing: rewriting one
    leaves every other plane's results bit for bit.  A NaN makes its own plane NaN, a
    dropped one too (the reference's ``x * 0``)."""
    x, dy = ec.make_input(case)
    planes, s = case.num_planes, case.s
    scale = ec.plane_scale(case, True)
    index = int(torch.nonzero(scale > 0 if victim == 'kept' else scale == 0)[0])
    assert index < planes - 1, 'the victim shares its workgroup with later planes'
    gen = torch.Generator().manual_seed(7)
    x2, dy2 = x.clone(), dy.clone()
    x2.view(planes, s)[index] = torch.randn(s, generator=gen) * 50 - 20
    dy2.view(planes, s)[index] = torch.randn(s, generator=gen) * 7
    if poison == 'nan':
        x2.view(planes, s)[index, s // 2] = float('nan')
        dy2.view(planes, s)[index, 1] = float('nan')

    before = dna(case, True, x.to(cuda), dy.to(cuda))
    after = dna(case, True, x2.to(cuda), dy2.to(cuda))
    others = torch.arange(planes) != index
    for name, a, b in zip(('y', 'dx', 'mean', 'rstd', 'scale'), before, after):
        a, b = a.cpu().view(planes, -1), b.cpu().view(planes, -1)
        assert torch.equal(a[others], b[others]), f'{name} of another plane changed'
        assert torch.isfinite(a).all()

    y64, dx64, _, _ = ec.reference(case, x2, dy2, True)
    y, dx, mean, rstd, _ = (t.cpu() for t in after)
    if poison == 'nan':
        assert torch.isnan(y64.view(planes, s)[index]).all()
        assert torch.isnan(dx64.view(planes, s)[index]).all()
        assert torch.isnan(mean[index]) and torch.isnan(rstd[index])
    else:
        assert torch.isfinite(y64).all() and torch.isfinite(dx64).all()
    assert torch.equal(torch.isnan(y), torch.isnan(y64))
    assert torch.equal(torch.isnan(dx), torch.isnan(dx64))


@pytest.mark.parametrize('spatial', [(8, 8), (16, 16)], ids=['S64', 'S256'])
def test_drop_norm_act_constant_plane(spatial):
    """A plane of 1.5 has an exact mean (S is a power of two), so z is exactly 0: y is 0 and
    dx = rstd * slope * (dy - mean(dy)), finite.  (Eval mode: 1.5 / 0.7 is no fp32 number,
    and past it even the fp64 reference's z is rounding noise of either sign.)  Bound on dx:
    that product is a chain of seven fp32 roundings (slope, eps, rsqrt, dy * slope, the mean,
    the difference, the final product) of at most one ulp each, so 8 ulp of the largest
    |dx|."""
    case = ec.Case('constant', (1, 3), spatial, *ec.PHILOX_PAIRS[0])
    x = torch.full(case.shape, 1.5)
    dy = torch.randn(case.shape, generator=torch.Generator().manual_seed(3))
    y, dx, mean, rstd, scale = (t.cpu() for t in dna(case, False, x.to(cuda), dy.to(cuda)))
    assert (scale == 1).all()
    assert (y == 0).all()
    assert (mean == 1.5).all()
    y64, dx64, _, _ = ec.reference(case, x, dy, False)
    assert (y64 == 0).all() and torch.isfinite(dx64).all()
    assert (dx64.view(3, -1).abs().amax(1) > 0.1).all(), 'the expected dx is not trivial'
    assert torch.isfinite(dx).all()
    bound = 8 * torch.finfo(torch.float32).eps * dx64.abs().max().item()
    error = (dx.double() - dx64).abs().max().item()
    print(f'DNA constant S={case.s}: dx error {error:.3e} bound {bound:.3e}')
    assert error <= bound


def test_drop_norm_act_p_zero_keeps_every_plane():
    x = torch.randn(3, 7, 5, 5, device=cuda)
    for seed, offset in ec.PHILOX_PAIRS:
        scale = ops().dna_forward(x, 0.0, ec.EPS, ec.SLOPE, _signed64(seed), _signed64(offset),
                                  True, None)[3]
        assert torch.equal(scale, torch.ones(21, device=cuda))


@pytest.mark.parametrize('shape', [(0, 3, 4, 4), (2, 0, 4, 4)])
def test_drop_norm_act_without_planes(shape):
    x = torch.empty(shape, device=cuda, requires_grad=True)
    y = fused._DropNormAct.apply(x, ec.P, ec.EPS, ec.SLOPE, 1, 2, True)
    assert y.shape == x.shape
    y.backward(torch.empty_like(y))
    assert x.grad.shape == x.shape
    outs = ops().dna_forward(x.detach(), ec.P, ec.EPS, ec.SLOPE, 1, 2, True, None)
    assert [tuple(t.shape) for t in outs] == [shape, (0,), (0,), (0,)]


# ---------------------------------------------------------------------------------------------
# The device-resident Philox slot: rng = [seed, base] and the call's offset = delta must
# draw what (seed, base + delta) draws.
# ---------------------------------------------------------------------------------------------
JUNK_SEED = 0x5EEDBAD
SLOTS = [
    pytest.param(12345, 7, 5, id='small'),
    pytest.param(2 ** 40 + 3, 2 ** 32 - 3, 8, id='offset-carries-past-2^32'),
    pytest.param(2 ** 63 + 11, 2 ** 33, 1, id='seed-above-2^63'),
]


def slot(seed, base):
    return torch.tensor([_signed64(seed), _signed64(base)], dtype=torch.int64, device=cuda)


@pytest.mark.parametrize('seed,base,delta', SLOTS)
def test_philox_slot_dna_forward(seed, base, delta):
    x = torch.randn(2, 9, 6, 6, device=cuda)
    got = ops().dna_forward(x, ec.P, ec.EPS, ec.SLOPE, JUNK_SEED, delta, True, slot(seed, base))
    want = ops().dna_forward(x, ec.P, ec.EPS, ec.SLOPE, _signed64(seed), _signed64(base + delta),
                             True, None)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    scale = fused.plane_scale_reference(18, ec.P, seed, base + delta, torch.device('cpu'))
    assert torch.equal(got[3].cpu(), scale)
    assert (scale == 0).any() and (scale > 0).any()


@pytest.mark.parametrize('seed,base,delta', SLOTS)
def test_philox_slot_dropout(seed, base, delta):
    x = torch.randn(1027, device=cuda)
    got = ops().dropout(x, 0.5, JUNK_SEED, delta, slot(seed, base))
    want = ops().dropout(x, 0.5, _signed64(seed), _signed64(base + delta), None)
    assert torch.equal(got, want)
    assert torch.equal(got.cpu(), dropout_ops._reference(x.cpu(), 0.5, seed, base + delta))


@pytest.mark.parametrize('seed,base,delta', SLOTS)
def test_philox_slot_uniform(seed, base, delta):
    got = ops().philox_uniform(1027, JUNK_SEED, delta, cuda, slot(seed, base))
    want = ops().philox_uniform(1027, _signed64(seed), _signed64(base + delta), cuda, None)
    assert torch.equal(got, want)
    assert torch.equal(got.cpu(), philox.uniform(1027, seed, base + delta))


# ---------------------------------------------------------------------------------------------
# Elementwise dropout and philox_uniform: the grid is capped at 2048 x 256 quads.
# ---------------------------------------------------------------------------------------------
STREAM_SIZES = [3, 4, 5, 2097152 + 1027]      # the last: a second grid-stride trip and a tail
STREAM_SEED, STREAM_OFFSET = 2 ** 40 + 3, 2 ** 33


@functools.lru_cache(maxsize=None)
def stream_uniforms(n):
    return philox.uniform(n, STREAM_SEED, STREAM_OFFSET)


@pytest.mark.parametrize('n', STREAM_SIZES)
def test_philox_uniform_sizes(n):
    got = misc.philox_uniform(n, STREAM_SEED, STREAM_OFFSET, cuda)
    assert torch.equal(got.cpu(), stream_uniforms(n))


@pytest.mark.parametrize('p', [0.5, 0.3])
@pytest.mark.parametrize('n', STREAM_SIZES)
def test_dropout_sizes(n, p):
    """Against ``dropout_ops._reference``, forward and backward.  The kernel multiplies by
    1 / (1 - p) where the reference divides by 1 - p: the same bits at p = 0.5 (a power of
    two); at p = 0.3 the same mask, and values 3 * 2^-24 apart at most: the kernel's two
    roundings (the reciprocal, the product) against the reference's one (the quotient)."""
    gen = torch.Generator().manual_seed(n)
    # (no zeros among the inputs: a zero of the output is then a dropped element)
    x = torch.randn(n, generator=gen)
    dy = torch.randn(n, generator=gen)
    x[x == 0] = 1.0
    dy[dy == 0] = 1.0
    xg = x.to(cuda).requires_grad_(True)
    y = dropout_ops._Dropout.apply(xg, p, STREAM_SEED, STREAM_OFFSET)
    (dx,) = torch.autograd.grad(y, xg, dy.to(cuda))
    keep = stream_uniforms(n) >= p
    for got, source in ((y.detach().cpu(), x), (dx.cpu(), dy)):
        want = dropout_ops._reference(source, p, STREAM_SEED, STREAM_OFFSET)
        assert torch.equal(got != 0, keep)
        if p == 0.5:
            assert torch.equal(got, want)
        else:
            torch.testing.assert_close(got, want, rtol=3.01 * 2.0 ** -24, atol=0)


@pytest.mark.parametrize('n', [5, 4101, 2097152 + 1027])
def test_dropout_misaligned_pointer(n):
    x = torch.randn(n, device=cuda)
    dy = torch.randn(n, device=cuda)

    def run(x, dy):
        x = x.requires_grad_(True)
        y = dropout_ops._Dropout.apply(x, 0.3, STREAM_SEED, STREAM_OFFSET)
        (dx,) = torch.autograd.grad(y, x, dy)
        return y.detach(), dx

    y, dx = run(x.clone(), dy)
    y_mis, _ = run(misaligned(x), dy)
    _, dx_mis = run(x.clone(), misaligned(dy))
    assert torch.equal(y_mis, y)
    assert torch.equal(dx_mis, dx)


@pytest.mark.parametrize('n', [5, 4101])
def test_dropout_p_zero_is_identity(n):
    x = torch.randn(n, device=cuda)
    assert torch.equal(dropout_ops._Dropout.apply(x, 0.0, STREAM_SEED, STREAM_OFFSET), x)


# ---------------------------------------------------------------------------------------------
# Pack / unpack against misc.pack's own CPU branch, byte for byte, in a buffer pre-filled
# with 0xA5 and 64 bytes longer than the message.
# ---------------------------------------------------------------------------------------------
FILL = 0xA5
BIG = 4 * 1024 * 1024 + 4805          # > 1024 x 256 x 16 bytes: grid-stride, and a 5-byte tail
DTYPES = [torch.uint8, torch.float16, torch.float32, torch.int64]


def random_bytes(nbytes, gen):
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=gen)


def mixed_tensors(count, gen):
    """``count`` small tensors cycling through the dtypes, with sizes of 1 to 13 elements."""
    out = []
    for i in range(count):
        dtype = DTYPES[i % len(DTYPES)]
        numel = 1 + (i * 7) % 13
        out.append(random_bytes(numel * torch.empty((), dtype=dtype).element_size(), gen)
                   .view(dtype))
    return out


def byte_tensors(sizes, gen):
    return [random_bytes(n, gen) for n in sizes]


def at_byte_one(t, fill=None):
    """``t`` (uint8, CPU) on its device of choice as a contiguous view at byte offset 1 of
    a longer buffer: ``(view, buffer)``."""
    buf = torch.empty(t.numel() + 33, dtype=torch.uint8, device=t.device)
    if fill is not None:
        buf.fill_(fill)
    view = buf[1:1 + t.numel()]
    view.copy_(t)
    return view, buf


PACK_CASES = {
    'seventeen': lambda gen: mixed_tensors(17, gen),
    'thirty-three': lambda gen: mixed_tensors(33, gen),
    'sizes': lambda gen: byte_tensors([0, 1, 15, 16, 17, BIG], gen),
    'zero-between': lambda gen: byte_tensors([1, 15, 0, 16, 0, 17, BIG, 0, 3], gen),
}


# (a typed tensor cannot start at byte offset 1: the offset views are the uint8 cases)
PACK_RUNS = [(name, False) for name in PACK_CASES] + [('sizes', True), ('zero-between', True)]
PACK_IDS = [f'{name}-{"byte-offset-1" if offset else "aligned"}' for name, offset in PACK_RUNS]


@pytest.mark.parametrize('name,offset_sources', PACK_RUNS, ids=PACK_IDS)
def test_pack_matches_cpu_branch(name, offset_sources):
    gen = torch.Generator().manual_seed(11)
    tensors = PACK_CASES[name](gen)
    if offset_sources:
        sources = [at_byte_one(t.to(cuda))[0] for t in tensors]
        assert all(s.data_ptr() % 16 == 1 for s in sources if s.numel())
    else:
        sources = [t.to(cuda) for t in tensors]
    nbytes = misc.packed_nbytes(tensors)
    want = torch.full((nbytes + 64,), FILL, dtype=torch.uint8)
    misc.pack(tensors, want)
    got = torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device=cuda)
    assert got.data_ptr() % 16 == 0
    misc.pack(sources, got)
    got = got.cpu()
    assert torch.equal(got, want)
    # said once more, of the bytes that belong to nobody
    assert (got[nbytes:] == FILL).all()
    pos = 0
    for t in tensors:
        end = pos + t.numel() * t.element_size()
        pos = (end + 15) // 16 * 16
        assert (got[end:pos] == FILL).all()
    assert pos == nbytes


@pytest.mark.parametrize('name,offset_dests', PACK_RUNS, ids=PACK_IDS)
def test_unpack_matches_cpu_branch(name, offset_dests):
    gen = torch.Generator().manual_seed(12)
    shapes = PACK_CASES[name](gen)
    message = random_bytes(misc.packed_nbytes(shapes) + 64, gen)

    def destinations(device):
        # (views, the buffers around them): every byte of a buffer is compared afterwards
        if offset_dests:
            pairs = [at_byte_one(torch.empty_like(t, device=device), FILL) for t in shapes]
            for view, _ in pairs:
                view.fill_(FILL)
            return [p[0] for p in pairs], [p[1] for p in pairs]
        outs = [torch.full_like(t.view(torch.uint8), FILL, device=device).view(t.dtype)
                for t in shapes]
        return outs, outs

    want_outs, want_bufs = destinations(torch.device('cpu'))
    misc.unpack(message, want_outs)
    got_outs, got_bufs = destinations(cuda)
    if offset_dests:
        assert all(o.data_ptr() % 16 == 1 for o in got_outs if o.numel())
    misc.unpack(message.to(cuda), got_outs)
    for got, want in zip(got_bufs, want_bufs):
        assert torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8))
    # and the CPU branch did deliver the message (the oracle is not vacuous)
    pos = 0
    for out in want_outs:
        n = out.numel() * out.element_size()
        assert torch.equal(out.view(-1).view(torch.uint8), message[pos:pos + n])
        pos = (pos + n + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------
# unet_ops: grids are capped at 16384 blocks of 256
# ---------------------------------------------------------------------------------------------
CAP = 16384 * 256


def up2x_reference(x, skip):
    x64 = x.detach().double().requires_grad_()
    s64 = skip.detach().double().requires_grad_()
    return x64, s64, torch.cat((F.interpolate(x64, scale_factor=2, mode='nearest'), s64), 1)


@pytest.mark.parametrize('shape', [
    pytest.param((2, 24, 128, 250, 9), id='forward-loops'),
    pytest.param((2, 66, 128, 250, 1), id='backward-loops-too'),
])
def test_up2x_cat_past_the_grid_cap(shape):
    n, c1, h, w, c2 = shape
    assert n * (c1 + c2) * 2 * h * w > CAP              # output pairs
    if c1 == 66:
        assert n * c1 * h * w > CAP                     # dx elements
    x = torch.randn(n, c1, h, w, device=cuda, requires_grad=True)
    skip = torch.randn(n, c2, 2 * h, 2 * w, device=cuda, requires_grad=True)
    out = up2x_cat(x, skip)
    assert out.grad_fn.__class__.__name__.startswith('_Up2xCat')
    x64, s64, ref = up2x_reference(x, skip)
    torch.testing.assert_close(out.double(), ref, rtol=0, atol=0)
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g.double())
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(skip.grad.double(), s64.grad, rtol=0, atol=0)


def test_up2x_cat_channels_last_gradient():
    """A channels_last gradient is no channel slice: the backward copies it first."""
    x = torch.randn(2, 3, 5, 7, device=cuda, requires_grad=True)
    skip = torch.randn(2, 4, 10, 14, device=cuda, requires_grad=True)
    out = up2x_cat(x, skip)
    assert out.grad_fn.__class__.__name__.startswith('_Up2xCat')
    x64, s64, ref = up2x_reference(x, skip)
    g = torch.randn_like(out).contiguous(memory_format=torch.channels_last)
    assert not g.is_contiguous()
    out.backward(g)
    ref.backward(g.double())
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(skip.grad.double(), s64.grad, rtol=0, atol=0)


def test_maxpool2x2_past_the_grid_cap():
    x = torch.randn(2, 8, 1025, 1027, device=cuda)
    assert 16 * 512 * 513 > CAP
    x[0, 0, 0, :2] = 1.5   # ties: the first maximum wins
    x[0, 0, 1, :2] = 1.5
    x[1, 7, 1023, 1025] = float('nan')
    x.requires_grad_(True)
    y = MaxPool2x2()(x)
    assert y.grad_fn.__class__.__name__.startswith('_MaxPool2x2')
    xr = x.detach().clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    torch.testing.assert_close(y, yr, rtol=0, atol=0, equal_nan=True)
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    torch.testing.assert_close(x.grad, xr.grad, rtol=0, atol=0, equal_nan=True)


def test_maxpool2x2_window_of_minus_infinity():
    x = torch.randn(1, 2, 4, 6, device=cuda)
    x[0, 1, 2:4, 4:6] = float('-inf')
    x.requires_grad_(True)
    y = MaxPool2x2()(x)
    xr = x.detach().clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    assert y[0, 1, 1, 2].item() == float('-inf')
    torch.testing.assert_close(y, yr, rtol=0, atol=0)
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    torch.testing.assert_close(x.grad, xr.grad, rtol=0, atol=0)
    window = x.grad[0, 1, 2:4, 4:6].flatten().tolist()
    assert window == [g[0, 1, 1, 2].item(), 0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------
# add_relu: capped at 8192 blocks of 256 quads; total % 4 goes to a tail, total < 4 has no
# quad at all.  8 388 608 + 3 fills the capped grid exactly once; + 7 adds the quad that
# sends one thread round the loop again.
# ---------------------------------------------------------------------------------------------
JOIN_TOTALS = [1, 3, 4, 5, 1027, 8388608 + 3, 8388608 + 7]
SPECIALS = {
    'finite': (0.5, 0.25),
    'nan-in-a': (float('nan'), 1.0),
    'nan-in-b': (1.0, float('nan')),
    'inf-minus-inf': (float('inf'), float('-inf')),
}


@pytest.mark.parametrize('special', list(SPECIALS))
@pytest.mark.parametrize('total', JOIN_TOTALS)
def test_add_relu_matches_aten(total, special):
    a = torch.randn(total, device=cuda)
    b = torch.randn(total, device=cuda)
    spots = sorted({0, total // 2, total - 1})      # the vector loop and the tail
    va, vb = SPECIALS[special]
    a[spots], b[spots] = va, vb
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = torch.relu(ar + br)
    if special != 'finite':
        assert torch.isnan(want[spots]).all()

    direct = ops().add_relu_forward(a, b)
    torch.testing.assert_close(direct, want.detach(), rtol=0, atol=0, equal_nan=True)

    ag, bg = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = fusion.add_relu(ag, bg)
    assert y.grad_fn.__class__.__name__.startswith('_AddReLU')
    torch.testing.assert_close(y.detach(), want.detach(), rtol=0, atol=0, equal_nan=True)
    g = torch.randn(total, device=cuda)
    got = torch.autograd.grad(y, (ag, bg), g)
    ref = torch.autograd.grad(want, (ar, br), g)
    for one, other in zip(got, ref):
        torch.testing.assert_close(one, other, rtol=0, atol=0, equal_nan=True)
    if special != 'finite':
        # ATen lets the gradient through where the sum is NaN: so does the join
        assert torch.equal(ref[0][spots], g[spots])


# ---------------------------------------------------------------------------------------------
# Pointers off a 16-byte boundary: the bindings copy such an input before the kernels'
# 8- and 16-byte accesses see it.
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['a', 'b', 'both'])
def test_add_relu_misaligned_pointer(which):
    a = torch.randn(1027, device=cuda)
    b = torch.randn(1027, device=cuda)
    am = misaligned(a) if which in ('a', 'both') else a
    bm = misaligned(b) if which in ('b', 'both') else b
    torch.testing.assert_close(ops().add_relu_forward(am, bm), torch.relu(a + b), rtol=0, atol=0)


@pytest.mark.parametrize('which', ['x', 'skip'])
def test_up2x_cat_misaligned_pointer(which):
    x = torch.randn(2, 3, 5, 7, device=cuda)
    skip = torch.randn(2, 4, 10, 14, device=cuda)
    xm = misaligned(x) if which == 'x' else x
    sm = misaligned(skip) if which == 'skip' else skip
    want = torch.cat((F.interpolate(x, scale_factor=2, mode='nearest'), skip), 1)
    torch.testing.assert_close(ops().up2x_cat_forward(xm, sm), want, rtol=0, atol=0)
    torch.testing.assert_close(up2x_cat(xm, sm), want, rtol=0, atol=0)


@pytest.mark.parametrize('c', [7, 3], ids=['every-channel', 'channel-slice'])
def test_up2x_backward_misaligned_pointer(c):
    dy = torch.randn(2, 7, 10, 14, device=cuda)
    want = F.avg_pool2d(dy[:, :c].double(), 2) * 4
    got = ops().up2x_backward(misaligned(dy), c)
    torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(ops().up2x_backward(dy, c), got, rtol=0, atol=0)
