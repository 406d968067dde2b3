"""The attention oracles of ops/precision.py, NativeSelfAttention off the GPU, and
transformer_lm through GPipe on CPU devices."""
import copy

import pytest
import torch

from torchgpipe_amd import GPipe
from torchgpipe_amd.models import transformer_lm
from torchgpipe_amd.ops.attention import NativeSelfAttention
from torchgpipe_amd.ops.precision import reference_attention, reference_attention_backward


def plain(q, k, v, causal):
    """softmax(q k^T / 8) v in fp64, written out."""
    s = q.double() @ k.double().transpose(-1, -2) / 8
    if causal:
        t = s.shape[-1]
        s = s.masked_fill(torch.ones(t, t, dtype=torch.bool).triu(1), float('-inf'))
    return s.softmax(-1) @ v.double()


@pytest.mark.parametrize('causal', [False, True])
def test_reference_highest_is_plain_fp64(causal):
    torch.manual_seed(0)
    q, k, v, do = (torch.randn(2, 3, 33, 64) for _ in range(4))
    leaves = [t.double().requires_grad_() for t in (q, k, v)]
    out = plain(*leaves, causal)
    grads = torch.autograd.grad(out, leaves, do.double())
    torch.testing.assert_close(reference_attention(q, k, v, causal), out.detach(),
                               rtol=1e-13, atol=1e-13)
    for got, want in zip(reference_attention_backward(do, q, k, v, causal), grads):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_cpu_module_is_the_plain_computation():
    torch.manual_seed(1)
    layer = NativeSelfAttention(128, 2, causal=True).double()
    assert list(layer.state_dict()) == ['qkv.weight', 'qkv.bias', 'proj.weight', 'proj.bias']
    x = torch.randn(2, 9, 128, dtype=torch.float64)
    q, k, v = (x @ w.t() + b for w, b in zip(layer.qkv.weight.chunk(3), layer.qkv.bias.chunk(3)))
    heads = [plain(*(t[..., 64 * h:64 * h + 64] for t in (q, k, v)), True) for h in range(2)]
    want = torch.cat(heads, -1) @ layer.proj.weight.t() + layer.proj.bias
    torch.testing.assert_close(layer(x), want, rtol=1e-12, atol=1e-12)


def test_transformer_lm_through_gpipe_on_cpu():
    torch.manual_seed(2)
    model = transformer_lm(vocab=50, d_model=64, heads=1, layers=1, seq_len=12)
    assert len(model) == 4
    tokens, target = torch.randint(50, (4, 12)), torch.randint(50, (4 * 12,))
    single = copy.deepcopy(model)
    want = torch.nn.functional.cross_entropy(single(tokens).flatten(0, 1), target)
    want.backward()
    pipe = GPipe(model, balance=[2, 2], devices=['cpu', 'cpu'], chunks=2, checkpoint='always')
    loss = torch.nn.functional.cross_entropy(pipe(tokens).flatten(0, 1), target)
    loss.backward()
    torch.testing.assert_close(loss, want, rtol=1e-5, atol=1e-6)
    for (name, p), r in zip(model.named_parameters(), single.parameters()):
        torch.testing.assert_close(p.grad, r.grad, rtol=1e-4, atol=1e-6, msg=name)
