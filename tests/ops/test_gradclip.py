"""``ops.gradclip`` on the CPU (the PyTorch path, the oracle of the kernels) against
``torch.nn.utils.clip_grad_norm_``."""
import math

import pytest
import torch
from torch import nn

from torchgpipe_amd.ops import gradclip

SIZES = (1, 3, 257, 65537)
SCALES = (1.0, 10.0, 0.1, 1.0)


def _params(dtype=torch.float64, seed=0):
    gen = torch.Generator().manual_seed(seed)
    params = []
    for n, s in zip(SIZES, SCALES):
        p = nn.Parameter(torch.zeros(n, dtype=dtype))
        p.grad = (torch.randn(n, generator=gen, dtype=torch.float64) * s).to(dtype)
        params.append(p)
    return params


def _clone(params):
    out = []
    for p in params:
        q = nn.Parameter(p.detach().clone())
        q.grad = None if p.grad is None else p.grad.clone()
        out.append(q)
    return out


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_matches_torch_fp64():
    ours, ref = _params(), _params()
    want = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    got = gradclip.clip_grad_norm_(ours, 1.0)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(float(got) - float(want)) <= 1e-12 * float(want)
    assert float(want) > 1.0  # the clip is active
    for p, q in zip(ours, ref):
        assert _rel(p.grad, q.grad) <= 1e-12


def test_grad_norm_leaves_gradients():
    ours = _params()
    before = [p.grad.clone() for p in ours]
    want = torch.nn.utils.clip_grad_norm_(_params(), 1.0)
    got = gradclip.grad_norm(ours)
    assert abs(float(got) - float(want)) <= 1e-12 * float(want)
    assert all(torch.equal(p.grad, b) for p, b in zip(ours, before))


def test_inactive_clip_is_bit_identical():
    ours = _params()
    before = [p.grad.clone() for p in ours]
    norm = gradclip.clip_grad_norm_(ours, 1e6)
    assert float(norm) < 1e6
    assert all(torch.equal(p.grad, b) for p, b in zip(ours, before))


def test_fp32_returns_fp32_norm():
    ours = _params(torch.float32)
    got = gradclip.clip_grad_norm_(ours, 1.0)
    assert got.dtype == torch.float32
    want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in
                         (p.grad for p in _params(torch.float32))))
    assert abs(float(got) - want) <= 1e-6 * want


def test_none_gradients_and_empty_list():
    ours = _params()
    ours[1].grad = None
    ref = _clone(ours)
    want = torch.nn.utils.clip_grad_norm_(ref, 0.5)
    got = gradclip.clip_grad_norm_(ours, 0.5)
    assert abs(float(got) - float(want)) <= 1e-12 * float(want)
    assert ours[1].grad is None
    assert float(gradclip.clip_grad_norm_([], 1.0)) == 0.0
    assert float(gradclip.clip_grad_norm_([nn.Parameter(torch.zeros(3))], 1.0)) == 0.0
    assert float(gradclip.grad_sumsq([])) == 0.0
    assert gradclip.grad_sumsq([]).dtype == torch.float64


def test_single_tensor_argument():
    p = _params()[2]
    want = torch.nn.utils.clip_grad_norm_(_clone([p]), 1.0)
    got = gradclip.clip_grad_norm_(p, 1.0)
    assert abs(float(got) - float(want)) <= 1e-12 * float(want)


def test_nan_poisons_every_gradient():
    ours = _params()
    ours[2].grad[100] = float('nan')
    norm = gradclip.clip_grad_norm_(ours, 1.0)
    assert math.isnan(float(norm))
    assert all(bool(p.grad.isnan().all()) for p in ours)


def test_inf_matches_torch():
    ours = _params()
    ours[2].grad[100] = float('inf')
    ref = _clone(ours)
    want = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    got = gradclip.clip_grad_norm_(ours, 1.0)
    assert math.isinf(float(got)) and math.isinf(float(want))
    for p, q in zip(ours, ref):
        assert torch.equal(p.grad.isnan(), q.grad.isnan())
        assert torch.allclose(p.grad, q.grad, rtol=0, atol=0, equal_nan=True)
    assert bool(ours[2].grad[100].isnan()) and float(ours[2].grad[99]) == 0.0


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_error_if_nonfinite(bad):
    ours = _params()
    ours[3].grad[5] = bad
    before = [p.grad.clone() for p in ours]
    with pytest.raises(RuntimeError, match='non-finite'):
        gradclip.clip_grad_norm_(ours, 1.0, error_if_nonfinite=True)
    for p, b in zip(ours, before):
        assert torch.allclose(p.grad, b, rtol=0, atol=0, equal_nan=True)
    gradclip.clip_grad_norm_(_params(), 1.0, error_if_nonfinite=True)  # finite: no error


@pytest.mark.parametrize('norm_type', [float('inf'), 1.0, 3.0])
def test_other_norm_types_match_torch(norm_type):
    ours, ref = _params(), _params()
    want = torch.nn.utils.clip_grad_norm_(ref, 0.5, norm_type=norm_type)
    got = gradclip.clip_grad_norm_(ours, 0.5, norm_type=norm_type)
    assert abs(float(got) - float(want)) <= 1e-12 * float(want)
    for p, q in zip(ours, ref):
        assert _rel(p.grad, q.grad) <= 1e-12


def test_sparse_gradients_are_refused():
    p = nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.sparse_coo_tensor([[0], [1]], [1.0], (4, 3))
    with pytest.raises(NotImplementedError):
        gradclip.clip_grad_norm_([p], 1.0)


def test_scale_grads_uses_the_given_sum():
    # the sum may have been combined with other ranks' since: 4x the local sum halves more
    g = [torch.full((5,), 3.0, dtype=torch.float64)]
    local = gradclip.grad_sumsq(g)
    assert float(local) == 45.0
    gradclip.scale_grads_(g, local * 4, max_norm=1.0)
    want = 3.0 / (2 * math.sqrt(45.0) + 1e-6)
    assert torch.allclose(g[0], torch.full((5,), want, dtype=torch.float64), rtol=1e-14, atol=0)


def test_non_contiguous_and_half_tensors():
    base = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    view = base.t()  # not dense-contiguous
    half = torch.ones(7, dtype=torch.float16) * 2
    want = float(base.double().pow(2).sum()) + 28.0
    assert float(gradclip.grad_sumsq([view, half])) == want
