"""Row-staged fused Winograd F(4x4,3x3) kernels (variants 16 / 17) vs an fp64 convolution
and vs the per-tap variants 6 / 7, whose arithmetic they share (GPU only)."""
import pytest
import torch
import torch.nn.functional as F

from torchgpipe_amd.ops import _ext

pytestmark = pytest.mark.gpu
cuda = torch.device('cuda', 0)

# (raw input rows through LDS, the per-tap kernel it derives from and falls back to):
# 64-channel workgroups, and the 32-channel arm.  The latter has the 7-segment instance
# only: below W = 24 (and where W % 4 != 0) the planner runs it as variant 7, so of the
# shapes below only the 24-, 36- and 192-wide ones reach f4_conv_rows_kernel<46, 9, 2>; on
# the others that arm compares variant 7 with itself.
ARMS = [(16, 6), (17, 7)]
ROWS, TAPS = ARMS[0]


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


SHAPES = [  # (N, C, K, H, W)
    (2, 64, 64, 24, 24),     # 6 tiles per row: a workgroup spans several tile rows, both images
    (1, 64, 192, 20, 36),    # 9 tiles per row; the last workgroup is partly past the last tile
    (3, 16, 96, 9, 12),      # H not a multiple of 4: bottom rows are zero
    (1, 3, 64, 16, 16),      # channels padded to the 4-channel step read zeros
    (2, 40, 64, 8, 8),       # 2 tiles per row: 16 row segments per workgroup
    (2, 256, 128, 12, 12),
    (1, 4, 64, 12, 192),     # 48 tiles per row: one workgroup inside a row, the next straddles
    (1, 24, 130, 14, 10),    # W % 4 != 0: runs as variant 6
]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('splits', [0, 1, 3])
@pytest.mark.parametrize('ROWS,TAPS', ARMS)
def test_rows_forward_and_flip(shape, splits, ROWS, TAPS):
    # The row-staged kernel feeds the same patches to the same transform and MFMA order as
    # the per-tap kernel of its workgroup shape (16 / 6: 64 channels, 17 / 7: 32), so on
    # top of the fp64 bound of test_f4_forward_and_flip its output equals the per-tap
    # kernel's bit for bit (on W % 4 != 0 it is that kernel).
    n, c, k, h, w = shape
    torch.manual_seed(3)
    x = torch.randn(n, c, h, w, device=cuda)
    wt = torch.randn(k, c, 3, 3, device=cuda) / (3 * c ** 0.5)
    b = torch.randn(k, device=cuda)
    ops = _ext.require(x)
    u = ops.wino4_weight(wt, False)
    y = ops.wino4_conv(x, u, b, k, ROWS, splits)
    want = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    torch.testing.assert_close(y.double(), want, rtol=1e-4,
                               atol=5e-5 * (want.abs().max().item() + 1))
    assert torch.equal(y, ops.wino4_conv(x, u, b, k, TAPS, splits))

    dy = torch.randn(n, k, h, w, device=cuda)
    uf = ops.wino4_weight(wt, True)
    dx = ops.wino4_conv(dy, uf, None, c, ROWS, splits)
    want_dx = torch.ops.aten.convolution_backward(
        dy.double(), x.double(), wt.double(), None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
        [True, False, False])[0]
    torch.testing.assert_close(dx.double(), want_dx, rtol=1e-4,
                               atol=5e-5 * (want_dx.abs().max().item() + 1))
    assert torch.equal(dx, ops.wino4_conv(dy, uf, None, c, TAPS, splits))


def test_rows_does_not_read_a_neighbouring_plane_for_padding():
    # The chunk left of column 0 is the previous row's tail and the chunk right of column
    # W - 1 the next row's head: in-bounds memory that must still read as zero.  Huge values
    # in every other plane and row would show in the borders.
    n, c, k, h, w = 2, 8, 64, 12, 16
    torch.manual_seed(4)
    x = torch.randn(n, c, h, w, device=cuda)
    x[:, :, :, 0] = 1e4
    x[:, :, :, -1] = -1e4
    wt = torch.randn(k, c, 3, 3, device=cuda) / (3 * c ** 0.5)
    ops = _ext.require(x)
    u = ops.wino4_weight(wt, False)
    y = ops.wino4_conv(x, u, None, k, ROWS, 1)
    want = F.conv2d(x.double(), wt.double(), padding=1)
    torch.testing.assert_close(y.double(), want, rtol=1e-4,
                               atol=5e-5 * (want.abs().max().item() + 1))
    assert torch.equal(y, ops.wino4_conv(x, u, None, k, TAPS, 1))


# -- weight gradient with the x operand's rows through LDS (wino4_wgrad variant 3) ----------
# The shapes and tolerance of test_f4_wgrad.  Variant 3 needs W % 4 == 0 and W >= 16 and
# runs as variant 0 elsewhere: the 24-, 36- and 40-wide shapes reach f4_wgrad_rows_kernel
# (36 and 40 wide: 9 / 10 tiles per row, so steps of 4 tiles straddle row and image ends).
WGRAD_SHAPES = [(2, 64, 64, 24, 24), (1, 24, 130, 14, 10), (3, 16, 96, 9, 12), (2, 40, 64, 8, 8),
                (1, 3, 64, 16, 16), (2, 5, 70, 7, 9), (1, 16, 8, 1, 1), (4, 32, 32, 33, 2),
                (2, 256, 128, 12, 12), (5, 64, 33, 20, 36), (2, 70, 40, 9, 40)]


def _wgrad_ref(x, dy, k, c):
    return torch.ops.aten.convolution_backward(
        dy.double(), x.double(), torch.zeros(k, c, 3, 3, device=cuda, dtype=torch.double), None,
        [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]


@pytest.mark.parametrize('shape', WGRAD_SHAPES)
@pytest.mark.parametrize('splits', [0, 1, 3, 1000])
def test_rows_wgrad(shape, splits):
    # the same patches into the same transform and MFMA order as variant 0: equal bit for bit
    n, c, k, h, w = shape
    torch.manual_seed(5)
    x = torch.randn(n, c, h, w, device=cuda)
    dy = torch.randn(n, k, h, w, device=cuda)
    ops = _ext.require(x)
    got = ops.wino4_wgrad(x, dy, splits, 3)
    want = _wgrad_ref(x, dy, k, c)
    torch.testing.assert_close(got.double(), want, rtol=1e-4,
                               atol=5e-5 * (want.abs().max().item() + 1))
    assert torch.equal(got, ops.wino4_wgrad(x, dy, splits, 0))


@pytest.mark.parametrize('shape', [(3, 70, 130, 13, 13), (3, 70, 130, 12, 20)])
@pytest.mark.parametrize('splits', [1, 2])
def test_rows_wgrad_accumulates_into_existing_gradient(shape, splits):
    # 13 x 13 is test_f4_wgrad_accumulates_into_existing_gradient's shape (runs as variant
    # 0); 12 x 20 reaches f4_wgrad_rows_kernel, with and without split partials
    n, c, k, h, w = shape
    torch.manual_seed(6)
    x = torch.randn(n, c, h, w, device=cuda)
    dy = torch.randn(n, k, h, w, device=cuda)
    base = torch.randn(k, c, 3, 3, device=cuda)
    into = base.clone()
    got = _ext.require(x).wino4_wgrad(x, dy, splits, 3, into)
    assert got.data_ptr() == into.data_ptr()
    want = base.double() + _wgrad_ref(x, dy, k, c)
    torch.testing.assert_close(got.double(), want, rtol=1e-4,
                               atol=5e-5 * (want.abs().max().item() + 1))
