"""The gradient-clipping kernels (``csrc/gradclip.hip``) against the fp64 formula on CPU
copies (GPU only).  Shapes come from the build (``grad_clip_info``)."""
import math

import pytest
import torch
from torch import nn

from torchgpipe_amd.ops import _ext, gradclip

pytestmark = pytest.mark.gpu

cuda = torch.device('cuda', 0)
EPS = 1e-6
# relative error of one scaled element against g64 * coef64: the coefficient's rounding to
# f32, the product's rounding and the reference's own (fp32); one rounding to 8 bits (bf16)
TOL = {torch.float32: 2.0 ** -22, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


def _chunk(dtype):
    info = gradclip.clip_info()
    return info[0] if dtype == torch.float32 else info[1]


def _make(numels, dtype, seed=0):
    """Gradients of ``numels`` elements, per-tensor scales from 1e-3 to 1e3, on the GPU."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(numels):
        scale = 10.0 ** (-3 + 6 * (i % 7) / 6)
        out.append((torch.randn(n, generator=gen, dtype=torch.float64) * scale).to(dtype)
                   .to(cuda))
    return out


def _sumsq64(tensors):
    return sum(float(t.cpu().double().pow(2).sum()) for t in tensors)


def _assert_scaled(after, before, coef, tol):
    want = before.cpu().double() * coef
    err = (after.cpu().double() - want).abs()
    assert bool((err <= tol * want.abs()).all()), float((err / want.abs().clamp_min(1e-300)).max())


def _boundary_numels(dtype):
    c = _chunk(dtype)
    return [1, 3, 63, 64, 65, 255, 256, 257, c - 1, c, c + 1, 2 * c + 5]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_sumsq_and_active_clip_at_boundary_sizes(dtype):
    grads = _make(_boundary_numels(dtype), dtype)
    assert sum(g.numel() for g in grads) < 2 ** 20
    before = [g.clone() for g in grads]
    want = _sumsq64(grads)
    sumsq = torch.ops.tgpipe.grad_sumsq(grads)
    assert sumsq.dtype == torch.float64 and sumsq.shape == (1,) and sumsq.device == cuda
    assert abs(float(sumsq) - want) <= 2e-10 * want
    assert all(torch.equal(g, b) for g, b in zip(grads, before))  # read-only
    max_norm = math.sqrt(want) / 3
    torch.ops.tgpipe.grad_scale_(grads, sumsq, max_norm, EPS)
    coef = max_norm / (math.sqrt(want) + EPS)
    for g, b in zip(grads, before):
        _assert_scaled(g, b, coef, TOL[dtype])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('big_first', [True, False])
def test_more_tensors_than_one_launch(dtype, big_first):
    per_launch = gradclip.clip_info()[2]
    big = [2 * _chunk(dtype) + 5]
    ones = [1] * (per_launch + 1)
    grads = _make(big + ones if big_first else ones + big, dtype, seed=1)
    before = [g.clone() for g in grads]
    want = _sumsq64(grads)
    sumsq = torch.ops.tgpipe.grad_sumsq(grads)
    assert abs(float(sumsq) - want) <= 2e-10 * want
    max_norm = math.sqrt(want) / 2
    torch.ops.tgpipe.grad_scale_(grads, sumsq, max_norm, EPS)
    coef = max_norm / (math.sqrt(want) + EPS)
    for g, b in zip(grads, before):
        _assert_scaled(g, b, coef, TOL[dtype])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_offset_views_are_bitwise_alike_and_stay_in_bounds(dtype):
    n = _chunk(dtype) + 37  # a full chunk and a ragged one
    values = _make([n], dtype, seed=2)[0]
    pad = 16
    sums, scaled = [], []
    for offset in range(16 // values.element_size()):
        buf = torch.full((n + 2 * pad,), 7.0, dtype=dtype, device=cuda)
        view = buf[pad + offset:pad + offset + n]
        view.copy_(values)
        assert view.data_ptr() % 16 == (offset * values.element_size()) % 16
        sumsq = torch.ops.tgpipe.grad_sumsq([view])
        sums.append(sumsq.cpu())
        torch.ops.tgpipe.grad_scale_([view], sumsq, 0.25 * math.sqrt(float(sumsq)), EPS)
        scaled.append(view.cpu().clone())
        # the sentinels ahead of and behind the view are as they were
        assert bool((buf[:pad + offset] == 7.0).all())
        assert bool((buf[pad + offset + n:] == 7.0).all())
    assert all(torch.equal(s, sums[0]) for s in sums), [float(s) for s in sums]
    assert all(torch.equal(s, scaled[0]) for s in scaled)
    want = _sumsq64([values])
    assert abs(float(sums[0]) - want) <= 2e-10 * want
    _assert_scaled(scaled[0], values, 0.25 * math.sqrt(want) / (math.sqrt(want) + EPS),
                   TOL[dtype])


def test_repeated_calls_are_bitwise_equal():
    grads = _make(_boundary_numels(torch.float32), torch.float32, seed=3)
    a = torch.ops.tgpipe.grad_sumsq(grads).cpu()
    b = torch.ops.tgpipe.grad_sumsq(grads).cpu()
    assert torch.equal(a, b)


def _as_params(grads):
    params = []
    for g in grads:
        p = nn.Parameter(torch.zeros_like(g))
        p.grad = g
        params.append(p)
    return params


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_inactive_clip_touches_nothing(dtype):
    grads = _make(_boundary_numels(dtype), dtype, seed=4)
    before = [g.clone() for g in grads]
    want = math.sqrt(_sumsq64(grads))
    norm = gradclip.clip_grad_norm_(_as_params(grads), 1.5 * want)
    assert norm.dtype == torch.float32 and norm.dim() == 0 and norm.device == cuda
    assert abs(float(norm) - want) <= 1e-6 * want
    assert all(torch.equal(g, b) for g, b in zip(grads, before))


def test_huge_and_tiny_values_neither_overflow_nor_vanish():
    # fp32 accumulation gives inf for the first list and 0 for the second
    grads = [torch.full((1,), 1e25, device=cuda) for _ in range(4)]
    want = _sumsq64(grads)
    sumsq = torch.ops.tgpipe.grad_sumsq(grads)
    assert math.isfinite(float(sumsq)) and abs(float(sumsq) - want) <= 2e-10 * want
    before = [g.clone() for g in grads]
    norm = gradclip.clip_grad_norm_(_as_params(grads), 1e25)
    assert abs(float(norm) - math.sqrt(want)) <= 1e-6 * math.sqrt(want)
    for g, b in zip(grads, before):
        _assert_scaled(g, b, 1e25 / (math.sqrt(want) + EPS), TOL[torch.float32])

    grads = [torch.full((1,), 1e-25, device=cuda) for _ in range(4)]
    before = [g.clone() for g in grads]
    want = _sumsq64(grads)
    sumsq = torch.ops.tgpipe.grad_sumsq(grads)
    assert float(sumsq) > 0 and abs(float(sumsq) - want) <= 2e-10 * want
    # with eps = 0 the coefficient is 1e-26 / 2e-25 = 0.05
    gradclip.scale_grads_(grads, sumsq.reshape(()), 1e-26, eps=0.0)
    for g, b in zip(grads, before):
        _assert_scaled(g, b, 1e-26 / math.sqrt(want), TOL[torch.float32])
    # with torch's eps the coefficient is ~1e-20 and the product the smallest subnormal:
    # right to one unit of it
    grads = [b.clone() for b in before]
    norm = gradclip.clip_grad_norm_(_as_params(grads), 1e-26)
    assert abs(float(norm) - math.sqrt(want)) <= 1e-6 * math.sqrt(want)
    coef = 1e-26 / (math.sqrt(want) + EPS)
    for g, b in zip(grads, before):
        assert abs(float(g.double()) - float(b.double()) * coef) <= 2.0 ** -149


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_nonfinite_element_follows_torch(bad):
    c = _chunk(torch.float32)
    grads = _make([5, 2 * c + 5, 300], torch.float32, seed=5)
    grads[1][c + 11] = bad
    ref = _as_params([g.clone() for g in grads])
    want = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    got = gradclip.clip_grad_norm_(_as_params(grads), 1.0)
    assert (math.isnan(float(got)) and math.isnan(float(want))) or float(got) == float(want)
    for g, r in zip(grads, ref):
        assert torch.allclose(g, r.grad, rtol=0, atol=0, equal_nan=True)
    assert bool(grads[1][c + 11].isnan())


def test_mixed_list_is_scaled_by_one_coefficient():
    c = _chunk(torch.float32)
    gen = torch.Generator().manual_seed(6)
    base = torch.randn(40, 30, generator=gen).to(cuda)
    grads = [_make([c + 9], torch.float32, seed=7)[0],
             _make([777], torch.bfloat16, seed=8)[0],
             torch.randn(513, generator=gen).to(torch.float16).to(cuda),
             base.t()]  # not contiguous
    assert not grads[3].is_contiguous()
    before = [g.clone() for g in grads]
    want = math.sqrt(_sumsq64(grads))
    norm = gradclip.clip_grad_norm_(_as_params(grads), want / 4)
    assert abs(float(norm) - want) <= 1e-6 * want
    coef = (want / 4) / (want + EPS)
    for g, b in zip(grads, before):
        _assert_scaled(g, b, coef, TOL[g.dtype])


def test_empty_lists_and_empty_tensors():
    out = torch.ops.tgpipe.grad_sumsq([])
    assert out.dtype == torch.float64 and float(out) == 0.0
    empty = torch.zeros(0, device=cuda)
    assert float(torch.ops.tgpipe.grad_sumsq([empty])) == 0.0
    g = torch.full((3,), 2.0, device=cuda)
    sumsq = torch.ops.tgpipe.grad_sumsq([empty, g, empty.reshape(0, 4)])
    assert float(sumsq) == 12.0
    torch.ops.tgpipe.grad_scale_([], sumsq, 1.0, EPS)
    torch.ops.tgpipe.grad_scale_([empty], sumsq, 1.0, EPS)
    torch.ops.tgpipe.grad_scale_([empty, g], sumsq, 1.0, EPS)
    _assert_scaled(g, torch.full((3,), 2.0), 1.0 / (math.sqrt(12.0) + EPS), TOL[torch.float32])
    assert float(gradclip.grad_sumsq([empty])) == 0.0


def test_native_op_refuses_what_the_python_layer_routes_away():
    half = torch.ones(4, dtype=torch.float16, device=cuda)
    with pytest.raises(RuntimeError, match='float32 or bfloat16'):
        torch.ops.tgpipe.grad_sumsq([half])
    with pytest.raises(RuntimeError, match='one dtype'):
        torch.ops.tgpipe.grad_sumsq([torch.ones(4, device=cuda),
                                     torch.ones(4, device=cuda, dtype=torch.bfloat16)])
    with pytest.raises(RuntimeError, match='dense'):
        torch.ops.tgpipe.grad_sumsq([torch.ones(4, 6, device=cuda)[:, :3]])
    with pytest.raises(RuntimeError, match='GPU'):
        torch.ops.tgpipe.grad_sumsq([torch.ones(4)])
