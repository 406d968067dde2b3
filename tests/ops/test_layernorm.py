"""ops/layernorm.py without a GPU: the modules step aside for CPU tensors, keep their parents'
state-dict keys, `eligible` refuses what the kernels do not take, and
transformer_lm(native_norm=True) is the default model on the CPU."""
import pytest
import torch
from torch import nn

from torchgpipe_amd.models.transformer import transformer_lm
from torchgpipe_amd.ops.layernorm import NativeLayerNorm, NativeRMSNorm, eligible


@pytest.mark.parametrize('native, parent', [(NativeLayerNorm, nn.LayerNorm),
                                            (NativeRMSNorm, nn.RMSNorm)])
def test_cpu_tensors_take_the_parent(native, parent):
    torch.manual_seed(0)
    layer, ref = native(24), parent(24)
    with torch.no_grad():
        layer.weight.add_(torch.randn(24))
    assert list(layer.state_dict()) == list(ref.state_dict())
    ref.load_state_dict(layer.state_dict())
    x = torch.randn(5, 24) + 3
    assert torch.equal(layer(x), ref(x))


class _Stub:
    """Only what `eligible` asks of a tensor: it never touches the data, and a CPU-only machine
    has no GPU tensor to show it."""
    is_cuda = True
    device = 'cuda:0'

    def __init__(self, shape, dtype=torch.float32, contiguous=True):
        self.shape, self.dtype, self._contiguous = torch.Size(shape), dtype, contiguous

    def dim(self):
        return len(self.shape)

    def numel(self):
        return self.shape.numel()

    def is_contiguous(self):
        return self._contiguous


def test_eligible():
    w = _Stub((64,))
    assert eligible(_Stub((4, 64)), (64,), w, w)
    assert eligible(_Stub((4, 8192)), 8192)
    assert not eligible(_Stub((4, 64), dtype=torch.float64), (64,))
    assert not eligible(_Stub((4, 64), contiguous=False), (64,))
    assert not eligible(_Stub((4, 8196)), (8196,))
    assert not eligible(_Stub((3, 4, 64)), (4, 64))
    assert not eligible(torch.randn(4, 64), (64,))  # a CPU tensor


def test_transformer_lm_native_norm_on_cpu():
    torch.manual_seed(1)
    model = transformer_lm(vocab=50, d_model=64, heads=1, layers=1, seq_len=12,
                           native_norm=True)
    plain = transformer_lm(vocab=50, d_model=64, heads=1, layers=1, seq_len=12)
    assert len(model) == len(plain) == 4 and isinstance(model[1].norm, NativeLayerNorm)
    plain.load_state_dict(model.state_dict())
    tokens = torch.randint(50, (2, 12))
    assert torch.equal(model(tokens), plain(tokens))
