"""The fused F(4x4) Winograd kernel on the bf16 matrix pipes (csrc/winograd_f4.hip
f4_conv_emu_kernel, variant 24, with the wino4_weight_emu image): its Winograd-domain
products are the three `high` partial products of split-bf16 U and V.

The oracle and the exact-transform input grids are those of tests/ops/test_precision_gpu.py
(wino_conv_emulated, _dyadic), copied so that this file stands alone.  Every geometry is the
smallest that reaches one way to go wrong (GEOS)."""
import pytest
import torch
import torch.nn.functional as F

from torchgpipe_amd.ops import _ext, precision
from torchgpipe_amd.ops.precision import split_bf16

pytestmark = pytest.mark.gpu

EMU = 24    # the split-bf16 fused kernel
EXACT = 6   # the f32 fused kernel of the same workgroup shape


@pytest.fixture(autouse=True)
def need_gpu_and_restore():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()
    assert precision.get_conv_precision() == 'highest'
    try:
        yield
    finally:
        precision.set_conv_precision('highest')


def ops():
    return torch.ops.tgpipe


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# (n, R, H, W, O)
GEOS = {
    'one-workgroup': (2, 64, 12, 12, 64),   # 18 of 32 tiles live
    'ragged': (3, 24, 10, 14, 48),          # R % 16, O % 16, H % 4, W % 4 != 0; 36 tiles: a tile
                                            # block spans two images, the second is mostly empty
    'two-channel-blocks': (1, 40, 9, 11, 80),
    'eight-chunks': (2, 128, 8, 8, 64),     # split-K: 3 does not divide 8 chunks
    'wide-rows': (1, 16, 8, 24, 32),        # W % 4 == 0 and W >= 24 (16-byte patch-row loads)
}
# (geometry, forced splits (0: the plan's), bias, backward-data)
CASES = [
    ('one-workgroup', 0, False, False),
    ('ragged', 0, False, False),
    ('two-channel-blocks', 0, False, False),
    ('eight-chunks', 1, False, False),
    ('eight-chunks', 2, False, False),
    ('eight-chunks', 3, False, False),
    ('wide-rows', 0, False, False),
    ('ragged', 1, True, False),
    ('ragged', 2, True, False),
    ('ragged', 0, False, True),
    ('eight-chunks', 3, False, True),
]
CASE_IDS = [f'{g}-s{s}{"-bias" if b else ""}{"-dgrad" if f else ""}' for g, s, b, f in CASES]

_MATS = ([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
          [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
         [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
          [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
         [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]])


def _three_products(eq, a, b, level):
    """einsum over the fp32 operands a, b: exact, or the three `high` products."""
    if level == 'highest':
        return torch.einsum(eq, a.double(), b.double())
    ah, am, _ = split_bf16(a)
    bh, bm, _ = split_bf16(b)
    return (torch.einsum(eq, ah.double() + am.double(), bh.double())
            + torch.einsum(eq, ah.double(), bm.double()))


def wino_conv_emulated(x, w, level):
    """F(4x4) with the kernel's roundings: transforms in fp64, U and V rounded to fp32,
    split, the products of the level, output transform (w = [O][R][3][3])."""
    bt, g, at = [torch.tensor(m, dtype=torch.float64, device=x.device) for m in _MATS]
    n, _, h, wd = x.shape
    th, tw = -(-h // 4), -(-wd // 4)
    xp = F.pad(x.double(), (1, 4 * tw + 1 - wd, 1, 4 * th + 1 - h))
    d = xp.unfold(2, 6, 4).unfold(3, 6, 4)                            # n c th tw 6 6
    v = torch.einsum('ia,nctwab,jb->nctwij', bt, d, bt).float()
    u = torch.einsum('ia,kcab,jb->kcij', g, w.double(), g).float()
    m = _three_products('kcij,nctwij->nktwij', u, v, level)
    y = torch.einsum('pi,nktwij,qj->nktwpq', at, m, at)
    y = y.permute(0, 1, 2, 4, 3, 5).reshape(n, w.shape[0], 4 * th, 4 * tw)
    return y[:, :, :h, :wd]


def _dyadic(shape, step, bound, gen):
    """Multiples of `step` up to `bound` steps: few significant bits, so that the Winograd
    transforms of these tensors are exact in fp32 and the kernel's V is the oracle's."""
    return torch.randint(-bound, bound + 1, shape, device='cuda', generator=gen).float() * step


_DATA = {}   # (geometry, flip) -> (x, kernel weight, conv weight [O][R][3][3], bias)
_EMUS = {}   # (geometry, flip, level) -> the oracle's result, computed once


@pytest.fixture(scope='module', autouse=True)
def release_shared_tensors():
    yield
    _DATA.clear()
    _EMUS.clear()


def _data(geo, flip):
    if (geo, flip) not in _DATA:
        n, r, h, w, o = GEOS[geo]
        gen = torch.Generator(device='cuda').manual_seed(11 + len(_DATA))
        x = _dyadic((n, r, h, w), 1 / 128, 512, gen)
        conv_w = _dyadic((o, r, 3, 3), 24 / 65536, 63, gen)
        # backward-data takes the forward layer's [R][O][3][3] weights and rotates them
        wt = conv_w.flip(2, 3).transpose(0, 1).contiguous() if flip else conv_w
        bias = _dyadic((o,), 1 / 128, 64, gen)
        _DATA[(geo, flip)] = (x, wt, conv_w, bias)
    return _DATA[(geo, flip)]


def _emulated(geo, flip, level):
    if (geo, flip, level) not in _EMUS:
        x, _, conv_w, _ = _data(geo, flip)
        _EMUS[(geo, flip, level)] = wino_conv_emulated(x, conv_w, level)
    return _EMUS[(geo, flip, level)]


def _run(geo, splits, bias, flip, variant=EMU):
    x, wt, _, b = _data(geo, flip)
    o = GEOS[geo][4]
    u = ops().wino4_weight_emu(wt, flip) if variant == EMU else ops().wino4_weight(wt, flip)
    return ops().wino4_conv(x, u, b if bias else None, o, variant, splits)


def _close(got, want):
    torch.testing.assert_close(got.double(), want, rtol=1e-4,
                               atol=2e-5 * (want.abs().max().item() + 1))


@pytest.mark.parametrize('geo,splits,bias,flip', CASES, ids=CASE_IDS)
def test_kernel_runs_the_high_products(geo, splits, bias, flip):
    """Within the tolerance of tests/ops/test_precision_gpu.py of the `high` oracle, ten
    times closer to it than the levels are apart (a dropped or doubled product is as far
    off as the levels; the accumulation order is 5e-8 .. 1.2e-6), the same bits at `high`
    and `medium`, and not the exact kernel's result."""
    add = _data(geo, flip)[3].double()[None, :, None, None] if bias else 0
    high = _emulated(geo, flip, 'high') + add
    highest = _emulated(geo, flip, 'highest') + add
    got = {}
    for level in ('high', 'medium'):
        with precision.conv_precision(level):
            got[level] = _run(geo, splits, bias, flip)
    exact = _run(geo, splits, bias, flip, EXACT)
    err, apart = rel_err(got['high'], high), rel_err(high, highest)
    print(f'{geo} splits={splits} bias={bias} flip={flip}: vs high {err:.2e}, '
          f'high vs highest {apart:.2e}, vs exact kernel {rel_err(got["high"], exact):.2e}')
    assert got['high'].shape == high.shape
    _close(got['high'], high)
    assert err <= 0.1 * apart
    assert torch.equal(got['high'], got['medium'])
    assert not torch.equal(got['high'], exact)
    _close(exact, highest)  # (the comparison kernel is the exact one)


@pytest.mark.parametrize('splits', [1, 3])
def test_two_runs_are_bit_identical(splits):
    """Checkpoint recomputation relies on it."""
    with precision.conv_precision('high'):
        a = _run('eight-chunks', splits, False, False)
        b = _run('eight-chunks', splits, False, False)
    assert torch.equal(a, b)


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('geo', ['one-workgroup', 'ragged', 'two-channel-blocks'])
def test_error_on_normal_inputs_is_that_of_the_high_level(geo, seed):
    """x standard normal, w scaled by (9R)^-1/2: the relative Frobenius error against fp64
    conv2d lies in [2e-5, 1e-4].  The oracle itself gives 4.1e-5 .. 5.3e-5 on these shapes
    and seeds (`highest`: 3.3e-7 .. 4.1e-7), so the band is a factor of two either side:
    below it the reduced products did not run, above it something else was lost."""
    n, r, h, w, o = GEOS[geo]
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(n, r, h, w, device='cuda', generator=gen)
    wt = torch.randn(o, r, 3, 3, device='cuda', generator=gen) / (9 * r) ** 0.5
    with precision.conv_precision('high'):
        got = ops().wino4_conv(x, ops().wino4_weight_emu(wt, False), None, o, EMU, 0)
    err = rel_err(got, F.conv2d(x.double(), wt.double(), padding=1))
    print(f'{geo} seed {seed}: {err:.2e}')
    assert 2e-5 <= err <= 1e-4


def test_wrong_weight_image_raises():
    x, wt, _, _ = _data('one-workgroup', False)
    with pytest.raises(RuntimeError, match='wino4_weight_emu'):
        ops().wino4_conv(x, ops().wino4_weight(wt, False), None, 64, EMU, 0)
    with pytest.raises(RuntimeError, match='does not match'):
        ops().wino4_conv(x, ops().wino4_weight_emu(wt, False), None, 64, EXACT, 0)
    # an image of other channel counts
    with pytest.raises(RuntimeError, match='wino4_weight_emu'):
        ops().wino4_conv(x, ops().wino4_weight_emu(wt[:, :32].contiguous(), False), None, 64,
                         EMU, 0)
    torch.cuda.synchronize()


def test_weight_image_refreshes_in_place():
    """wino4_weight_emu(out=) overwrites an existing image (the per-step cache refresh)."""
    _, wt, _, _ = _data('ragged', False)
    u = ops().wino4_weight_emu(wt, False)
    v = ops().wino4_weight_emu(2 * wt, False)
    assert not torch.equal(u.view(torch.int32), v.view(torch.int32))
    back = ops().wino4_weight_emu(2 * wt, False, u)
    assert back.data_ptr() == u.data_ptr()
    assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    with pytest.raises(RuntimeError, match='shape'):
        ops().wino4_weight_emu(wt, False, torch.empty(3, device='cuda'))
