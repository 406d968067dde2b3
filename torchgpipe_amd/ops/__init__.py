"""Hand-written HIP/CDNA4 kernels of the framework and their PyTorch bindings.

* :mod:`.dbn` — DeferredBatchNorm statistics (K1 track, K2 commit)
* :mod:`.fused` — fused Dropout2d → InstanceNorm2d → LeakyReLU (U-Net cell)
* :mod:`.dropout` — Philox dropout with explicit (seed, offset)
* :mod:`.philox` — bit-exact CPU reference of the Philox stream
* :mod:`.misc` — spin kernel (race tests), multi-tensor pack/unpack
* :mod:`.gradclip` — global-norm gradient clipping (fp64 sum of squares, in-place scale)
* :mod:`.linear` — ``nn.Linear`` on the split-bf16 dense GEMM (``NativeLinear``, opt-in)
* :mod:`.attention` — fused fp32 attention, head dims 64 / 128, split-bf16
  (``NativeSelfAttention``)
* :mod:`.layernorm` — ``nn.LayerNorm`` / ``nn.RMSNorm`` over the last dimension, rows in
  registers, fixed-order affine gradients (``NativeLayerNorm``, ``NativeRMSNorm``, opt-in)
* :mod:`.loss` — softmax cross-entropy over streamed logit rows: one read forward, one read
  and one write backward, no saved log-softmax (``NativeCrossEntropyLoss``, opt-in)
"""
from torchgpipe_amd.ops import _ext, gradclip, layernorm, linear, loss
from torchgpipe_amd.ops.layernorm import (NativeLayerNorm, NativeRMSNorm, native_layer_norm,
                                          native_rms_norm)
from torchgpipe_amd.ops.loss import NativeCrossEntropyLoss, native_cross_entropy

available = _ext.available

__all__ = ['available', 'gradclip', 'layernorm', 'linear', 'loss', 'NativeLayerNorm',
           'NativeRMSNorm', 'native_layer_norm', 'native_rms_norm', 'NativeCrossEntropyLoss',
           'native_cross_entropy']
