"""The step of the row-staged fused F(4x4) kernels against the serial step kept under a
second id (GPU only).  Weight gradient: id 3 issues the transforms and ring reads between
the MFMAs of a step (f4_pipe_step), id 4 is the serial kernel -- the same arithmetic in the
same order, so equal bit for bit, and bit-stable from run to run.  Forward / backward-data:
id 25 names the kernels of id 16 (the pipelined step measured slower there and id 16 kept
the serial one, profiles/KERNELS.md "Round 19"); the cases stay as the check of whatever
body id 16 takes next."""
import pytest
import torch

from torchgpipe_amd.ops import _ext

pytestmark = pytest.mark.gpu
cuda = torch.device('cuda', 0)

NEW, SERIAL = 16, 25
WG_NEW, WG_SERIAL = 3, 4


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


CONV_CASES = [  # ((N, C, K, H, W), splits)
    ((1, 4, 64, 24, 24), 0),      # one step: the prologue alone, clamped look-ahead
    ((2, 8, 64, 24, 24), 0),      # two steps; 72 tiles: a workgroup spans the image boundary,
                                  # the last one is part-filled
    ((1, 12, 40, 24, 28), 0),     # odd step count (tail step); part channel block; row break
                                  # inside a workgroup
    ((2, 20, 64, 10, 24), 3),     # H % 4 != 0 (clipped stores); uneven split ranges
    ((1, 36, 128, 24, 24), 0),
    ((1, 36, 128, 24, 24), 1000),
    ((2, 8, 64, 8, 8), 0),        # the <66, 5> instance (below 6 tiles per row)
    ((1, 12, 64, 12, 16), 0),
]


@pytest.mark.parametrize('shape,splits', CONV_CASES)
@pytest.mark.parametrize('flip', [False, True])
def test_step_forward_and_flip(shape, splits, flip):
    n, c, k, h, w = shape
    torch.manual_seed(19)
    wt = torch.randn(k, c, 3, 3, device=cuda) / (3 * c ** 0.5)
    ops = _ext.require(wt)
    if flip:   # backward-data: dy [N][K] -> dx [N][C], no bias
        x = torch.randn(n, k, h, w, device=cuda)
        u, b, out = ops.wino4_weight(wt, True), None, c
    else:
        x = torch.randn(n, c, h, w, device=cuda)
        u, b, out = ops.wino4_weight(wt, False), torch.randn(k, device=cuda), k
    want = ops.wino4_conv(x, u, b, out, SERIAL, splits)
    got = ops.wino4_conv(x, u, b, out, NEW, splits)
    again = ops.wino4_conv(x, u, b, out, NEW, splits)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert torch.equal(again, got)
    assert torch.equal(ops.wino4_conv(x, u, b, out, SERIAL, splits), want)


WGRAD_CASES = [  # ((N, C, K, H, W), splits)
    ((1, 32, 16, 16, 16), 0),
    ((2, 32, 64, 24, 24), 0),
    ((3, 64, 40, 12, 28), 0),
    ((3, 64, 40, 12, 28), 1),
    ((3, 64, 40, 12, 28), 3),
    ((3, 64, 40, 12, 28), 1000),
]


@pytest.mark.parametrize('shape,splits', WGRAD_CASES)
def test_step_wgrad(shape, splits):
    n, c, k, h, w = shape
    torch.manual_seed(20)
    x = torch.randn(n, c, h, w, device=cuda)
    dy = torch.randn(n, k, h, w, device=cuda)
    ops = _ext.require(x)
    want = ops.wino4_wgrad(x, dy, splits, WG_SERIAL)
    got = ops.wino4_wgrad(x, dy, splits, WG_NEW)
    again = ops.wino4_wgrad(x, dy, splits, WG_NEW)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    assert torch.equal(again, got)
    assert torch.equal(ops.wino4_wgrad(x, dy, splits, WG_SERIAL), want)


def test_step_wgrad_accumulates_into_existing_gradient():
    n, c, k, h, w = 2, 32, 32, 24, 24
    torch.manual_seed(21)
    x = torch.randn(n, c, h, w, device=cuda)
    dy = torch.randn(n, k, h, w, device=cuda)
    base = torch.randn(k, c, 3, 3, device=cuda)
    ops = _ext.require(x)
    want = ops.wino4_wgrad(x, dy, 0, WG_SERIAL, base.clone())
    for _ in range(2):
        into = base.clone()
        got = ops.wino4_wgrad(x, dy, 0, WG_NEW, into)
        assert got.data_ptr() == into.data_ptr()
        assert torch.equal(got, want)
    assert not torch.equal(want, base)
