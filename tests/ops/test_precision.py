"""The conv precision levels (ops/precision.py) on the CPU: the exact three-way bf16 split,
the level API, and the fp64 oracle of the levels' semantics that the GPU tests compare the
kernels with."""
import pytest
import torch
import torch.nn.functional as F

from torchgpipe_amd.ops import precision

# the geometries of tests/ops/test_precision_gpu.py: (n, ci, h, w, co, kh, kw, stride, pad)
SHAPES = [
    (4, 32, 28, 28, 48, 1, 1, 1, 0),
    (5, 24, 7, 7, 40, 1, 1, 1, 0),
    (3, 16, 14, 14, 20, 1, 7, 1, 3),
    (2, 24, 15, 15, 16, 1, 1, 2, 0),
    (4, 1024, 7, 7, 256, 1, 1, 1, 0),
    (2, 3, 32, 32, 16, 3, 3, 1, 1),
    (3, 16, 15, 15, 24, 3, 3, 2, 1),
]


@pytest.fixture(autouse=True)
def restore_level():
    before = precision.get_conv_precision()
    yield
    precision.set_conv_precision(before)


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _case(shape):
    n, ci, h, w, co, kh, kw, stride, pad = shape
    torch.manual_seed(0)
    x = torch.randn(n, ci, h, w)
    wt = torch.randn(co, ci, kh, kw) / (ci * kh * kw) ** 0.5
    padding = (pad if kh > 1 else 0, pad if kw > 1 else 0)
    return x, wt, stride, padding


def test_split_is_exact_and_every_part_is_a_bf16():
    torch.manual_seed(0)
    x = torch.cat([torch.randn(1 << 16), torch.randn(1 << 12) * 1e-20,
                   torch.randn(1 << 12) * 1e20, torch.zeros(4)])
    hi, mid, lo = precision.split_bf16(x)
    # bit for bit: the sum of the parts, smallest first, is x itself
    assert torch.equal((lo + mid) + hi, x)
    assert torch.equal((lo.double() + mid.double() + hi.double()).float(), x)
    assert torch.equal(lo.double() + mid.double() + hi.double(), x.double())
    for part in (hi, mid, lo):
        assert part.dtype == torch.float32
        assert torch.equal(part.bfloat16().float(), part)
    # round to nearest: hi is the bf16 nearest to x, mid the one nearest to the rest
    assert torch.equal(hi, x.bfloat16().float())
    assert torch.equal(mid, (x - hi).bfloat16().float())


def test_level_api_round_trip():
    assert precision.get_conv_precision() == 'highest'
    for level in ('high', 'medium', 'highest'):
        precision.set_conv_precision(level)
        assert precision.get_conv_precision() == level


def test_context_manager_restores_the_level_on_exception():
    precision.set_conv_precision('high')
    with pytest.raises(RuntimeError, match='boom'):
        with precision.conv_precision('medium'):
            assert precision.get_conv_precision() == 'medium'
            raise RuntimeError('boom')
    assert precision.get_conv_precision() == 'high'
    with precision.conv_precision('highest'):
        assert precision.get_conv_precision() == 'highest'
    assert precision.get_conv_precision() == 'high'


@pytest.mark.parametrize('bad', ['tf32', 'HIGH', '', None, 1])
def test_bad_level_names_raise_value_error(bad):
    with pytest.raises(ValueError):
        precision.set_conv_precision(bad)
    with pytest.raises(ValueError):
        with precision.conv_precision(bad):
            pass
    with pytest.raises(ValueError):
        precision.reference_conv2d(torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 1, 1), level=bad)
    assert precision.get_conv_precision() == 'highest'


def test_level_does_not_follow_torch_matmul_precision():
    before = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision('medium')
        assert precision.get_conv_precision() == 'highest'
        precision.set_conv_precision('high')
        assert torch.get_float32_matmul_precision() == 'medium'
    finally:
        torch.set_float32_matmul_precision(before)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape', SHAPES[:4] + SHAPES[5:], ids=str)
def test_reference_at_highest_is_the_fp64_convolution(shape, relu):
    x, wt, stride, padding = _case(shape)
    x64 = x.double().requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    want = F.conv2d(F.relu(x64) if relu else x64, w64, stride=stride, padding=padding)
    got = precision.reference_conv2d(x, wt, stride, padding, 'highest', relu)
    assert got.dtype == torch.float64
    assert torch.equal(got, want.detach())
    dz = torch.randn(want.shape)
    want.backward(dz.double())
    dx, dw = precision.reference_conv2d_backward(dz, x, wt, stride, padding, 'highest', relu)
    torch.testing.assert_close(dx, x64.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dw, w64.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_reference_levels_keep_their_distance_from_exact(shape, relu):
    """The GPU tests tell the levels apart by their distance from the exact result: `high`
    must lie beyond 3e-6 and `medium` beyond 1e-3 (relative Frobenius), both far inside what
    their error model allows (3 * 2^-18 and 2^-8 per product)."""
    x, wt, stride, padding = _case(shape)
    exact = precision.reference_conv2d(x, wt, stride, padding, 'highest', relu)
    high = rel_err(precision.reference_conv2d(x, wt, stride, padding, 'high', relu), exact)
    medium = rel_err(precision.reference_conv2d(x, wt, stride, padding, 'medium', relu), exact)
    print(f'{shape} relu={relu}: high {high:.3e} medium {medium:.3e}')
    assert 3.5e-6 < high < 3 * 2.0 ** -18
    assert 1.5e-3 < medium < 2.0 ** -8
    # backward-data and weight gradient: the same bands
    dz = torch.randn(exact.shape)
    dx0, dw0 = precision.reference_conv2d_backward(dz, x, wt, stride, padding, 'highest', relu)
    dx1, dw1 = precision.reference_conv2d_backward(dz, x, wt, stride, padding, 'high', relu)
    dx2, dw2 = precision.reference_conv2d_backward(dz, x, wt, stride, padding, 'medium', relu)
    print(f'  dx high {rel_err(dx1, dx0):.3e} medium {rel_err(dx2, dx0):.3e}; '
          f'dw high {rel_err(dw1, dw0):.3e} medium {rel_err(dw2, dw0):.3e}')
    assert 3.5e-6 < rel_err(dx1, dx0) < 3 * 2.0 ** -18
    assert 1.5e-3 < rel_err(dx2, dx0) < 2.0 ** -8
    assert rel_err(dw1, dw0) < 3 * 2.0 ** -18
    assert 1.5e-3 < rel_err(dw2, dw0) < 2.0 ** -8


def test_medium_reference_is_the_convolution_of_the_hi_parts():
    x, wt, stride, padding = _case(SHAPES[2])
    xh = precision.split_bf16(F.relu(x))[0]
    wh = precision.split_bf16(wt)[0]
    want = F.conv2d(xh.double(), wh.double(), stride=stride, padding=padding)
    assert torch.equal(precision.reference_conv2d(x, wt, stride, padding, 'medium', True), want)
    # and the hi parts are fixed points of the split: `highest` on them is `medium` on x
    assert torch.equal(precision.reference_conv2d(xh, wh, stride, padding, 'highest'), want)
