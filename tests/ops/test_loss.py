"""ops/loss.py without a GPU: the module steps aside for CPU tensors, and `eligible` refuses
what the kernels do not take (and `native_cross_entropy` raises on it)."""
import pytest
import torch
from torch import nn

from torchgpipe_amd.ops.loss import NativeCrossEntropyLoss, eligible, native_cross_entropy


@pytest.mark.parametrize('kwargs', [{}, {'ignore_index': 1, 'label_smoothing': 0.1},
                                    {'reduction': 'none', 'weight': torch.rand(9)}])
def test_cpu_tensors_take_the_parent(kwargs):
    torch.manual_seed(0)
    x, t = torch.randn(6, 9), torch.randint(9, (6,))
    assert torch.equal(NativeCrossEntropyLoss(**kwargs)(x, t), nn.CrossEntropyLoss(**kwargs)(x, t))


class _Stub:
    """Only what `eligible` asks of a tensor: it never touches the data, and a CPU-only machine
    has no GPU tensor to show it."""
    is_cuda = True
    device = 'cuda:0'

    def __init__(self, shape, dtype=torch.float32, contiguous=True):
        self.shape, self.dtype, self._contiguous = torch.Size(shape), dtype, contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous


@pytest.mark.parametrize('logits, target', [
    (torch.randn(4, 9), torch.randint(9, (4,))),                     # CPU tensors
    (_Stub((4, 9), torch.float64), _Stub((4,), torch.int64)),
    (_Stub((4, 9), contiguous=False), _Stub((4,), torch.int64)),
    (_Stub((4, 9)), _Stub((4,), torch.int64, contiguous=False)),
    (_Stub((2, 9, 5)), _Stub((2, 5), torch.int64)),                  # [B, V, T]
    (_Stub((4, 9)), _Stub((4,), torch.int32)),
    (_Stub((4, 9)), _Stub((4, 9))),                                  # probability targets
], ids=['cpu', 'fp64', 'strided', 'strided target', 'B V T', 'int32', 'probabilities'])
def test_not_eligible(logits, target):
    assert eligible(_Stub((4, 9)), _Stub((4,), torch.int64))
    assert not eligible(logits, target)
    with pytest.raises(ValueError):
        native_cross_entropy(logits, target)
