"""WinogradConv2d on the fused split-bf16 F(4x4) kernel (variant 24): at the conv precision
levels 'high' / 'medium' the routing of ops/conv.py sends the 64-channel 24^2 layer below
-- the smallest shape of the measured classes -- to it in both directions; at 'highest'
nothing changes."""
import pytest
import torch

from tests.ops.test_f4_emu_gpu import _close, _dyadic, rel_err, wino_conv_emulated
from torchgpipe_amd.ops import _ext, conv, precision
from torchgpipe_amd.ops.conv import WinogradConv2d

pytestmark = pytest.mark.gpu

N, C, H, W, K = 1, 64, 24, 24, 64
F32_IMAGE_BYTES = 64 * 64 * 36 * 4   # U4 of 64 x 64 channels; the bf16 image is as large


@pytest.fixture(autouse=True)
def need_gpu_and_restore(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()
    assert precision.get_conv_precision() == 'highest'
    # a cache budget of this test's own, whatever earlier pipelines sized the device's to
    monkeypatch.delenv('TGPIPE_WINOGRAD_CACHE_MB', raising=False)
    monkeypatch.setitem(conv._DEVICE_BUDGET, torch.device('cuda', 0), 1 << 30)
    try:
        yield
    finally:
        precision.set_conv_precision('highest')


def ops():
    return torch.ops.tgpipe


def _layer(seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    layer = WinogradConv2d(C, K, 3, padding=1, bias=False).to('cuda:0')
    with torch.no_grad():
        layer.weight.copy_(_dyadic((K, C, 3, 3), 24 / 65536, 63, gen))
    x = _dyadic((N, C, H, W), 1 / 128, 512, gen).requires_grad_(True)
    dy = _dyadic((N, K, H, W), 1 / 128, 512, gen)
    return layer, x, dy


def test_routing_of_this_layer():
    for level in ('high', 'medium'):
        assert conv.f4_variant((N, C, H, W), K, level) == conv.F4_EMU_VARIANT    # forward
        assert conv.f4_variant((N, K, H, W), C, level) == conv.F4_EMU_VARIANT    # backward-data
    assert conv.f4_variant((N, C, H, W), K, 'highest') == 7
    assert conv.f4_variant((N, C, H - 1, W), K, 'high') == 7                     # no smaller plane


def test_high_runs_the_split_bf16_kernel_and_keeps_the_weight_gradient_exact():
    layer, x, dy = _layer(3)
    w = layer.weight.detach()
    with precision.conv_precision('high'):
        y = layer(x)
        y.backward(dy)
    dx, dw = x.grad, layer.weight.grad
    exact = ops().wino4_conv(x.detach(), ops().wino4_weight(w, False), None, K, 7, 0)
    want = wino_conv_emulated(x.detach(), w, 'high')
    apart = rel_err(want, wino_conv_emulated(x.detach(), w, 'highest'))
    _close(y, want)
    assert rel_err(y, want) <= 0.1 * apart
    assert not torch.equal(y, exact)
    w_t = w.flip(2, 3).transpose(0, 1).contiguous()   # backward-data as a convolution of dy
    want_dx = wino_conv_emulated(dy, w_t, 'high')
    _close(dx, want_dx)
    apart = rel_err(want_dx, wino_conv_emulated(dy, w_t, 'highest'))
    assert rel_err(dx, want_dx) <= 0.1 * apart
    # the fused weight gradient is exact at every level: the fp64 bound of
    # tests/ops/test_winograd_gpu.py
    want_dw = torch.nn.grad.conv2d_weight(x.detach().double(), w.shape, dy.double(), padding=1)
    torch.testing.assert_close(dw.double(), want_dw, rtol=1e-4,
                               atol=2e-5 * (want_dw.abs().max().item() + 1))


def test_highest_is_bit_identical_to_the_exact_variant_and_derives_no_new_image():
    layer, x, dy = _layer(4)
    w = layer.weight.detach()
    before = conv.cache_bytes()
    y = layer(x)
    y.backward(dy)
    # the two f32 images (forward and backward-data) and nothing else
    assert conv.cache_bytes() - before == 2 * F32_IMAGE_BYTES
    u, u_flip = ops().wino4_weight(w, False), ops().wino4_weight(w, True)
    assert torch.equal(y, ops().wino4_conv(x.detach(), u, None, K, 7, 0))
    assert torch.equal(x.grad, ops().wino4_conv(dy, u_flip, None, C, 7, 0))
    dw_highest = layer.weight.grad.clone()
    # ... and the weight gradient at 'high' is the same kernel on the same data
    layer.weight.grad = None
    x.grad = None
    with precision.conv_precision('high'):
        layer(x).backward(dy)
    assert torch.equal(layer.weight.grad, dw_highest)
    assert conv.cache_bytes() - before == 4 * F32_IMAGE_BYTES  # + the two bf16 images


def test_per_step_refresh_rewrites_the_image_in_place():
    layer, x, _ = _layer(5)
    with precision.conv_precision('high'), torch.no_grad():
        y1 = layer(x)
        held = [u.data_ptr() for u in layer._wino.derived()]
        assert len(held) == 1
        layer.weight.data.mul_(2)            # an optimizer-style update: no version bump
        conv.new_step()
        conv.refresh_step_caches(layer)
        assert [u.data_ptr() for u in layer._wino.derived()] == held
        before = conv.cache_bytes()
        y2 = layer(x)
        assert conv.cache_bytes() == before  # a hit on the refreshed image
    assert torch.equal(y2, 2 * y1)           # (scaling by two is exact through the split)
    _close(y2, wino_conv_emulated(x.detach(), layer.weight.detach(), 'high'))
