"""NativeLinear off the GPU, the Linear oracles of ops/precision.py, and vgg16's switch."""
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd.models.vgg import vgg16
from torchgpipe_amd.ops.linear import NativeLinear
from torchgpipe_amd.ops.precision import reference_linear, split_bf16


def _operands():
    torch.manual_seed(0)
    return torch.randn(5, 37), torch.randn(10, 37) / 37 ** 0.5, torch.randn(10)


def test_cpu_forward_is_nn_linear():
    x, w, b = _operands()
    native, plain = NativeLinear(37, 10), nn.Linear(37, 10)
    plain.load_state_dict(native.state_dict())
    assert torch.equal(native(x), plain(x))


def test_reference_highest_is_fp64_linear():
    x, w, b = _operands()
    assert torch.equal(reference_linear(x, w, b, 'highest'),
                       F.linear(x.double(), w.double(), b.double()))


def test_reference_medium_is_hi_times_hi():
    x, w, b = _operands()
    expect = F.linear(split_bf16(x)[0].double(), split_bf16(w)[0].double()) + b.double()
    assert torch.equal(reference_linear(x, w, b, 'medium'), expect)


def test_vgg16_native_linear_switch():
    def count(model):
        return sum(isinstance(m, NativeLinear) for m in model.modules())
    with torch.device('meta'):  # (the structure only: no 120 M parameters to initialise)
        default, native = vgg16(num_classes=10), vgg16(num_classes=10, native_linear=True)
    assert count(default) == 0 and count(native) == 3
    assert list(default.state_dict()) == list(native.state_dict())
