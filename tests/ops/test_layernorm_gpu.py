"""The native LayerNorm / RMSNorm kernels (csrc/layernorm.hip, ops/layernorm.py) on the GPU:
every path against fp64 with the library's own fp32 error as the yardstick, bitwise
reproducibility, accumulation into .grad, and transformer_lm(native_norm=True) in a pipeline."""
import copy

import pytest
import torch
import torch.nn.functional as F

from torchgpipe_amd import GPipe
from torchgpipe_amd.models.transformer import transformer_lm
from torchgpipe_amd.ops import _ext, layernorm
from torchgpipe_amd.ops.layernorm import (NativeLayerNorm, _backward_sweep_rows, _wave_row_max,
                                          native_layer_norm, native_rms_norm)

pytestmark = pytest.mark.gpu

EPS = 1e-5
FLOOR = 5e-7  # native error <= max(3 x the library's fp32 error, FLOOR)
KINDS = ['affine', 'plain', 'nobias', 'rms']
# (R, N, offset); 'W' = the wave-per-row instance's widest row, 'Rg' = one more than twice
# the rows the persistent backward grid covers in one sweep
CASES = [
    (3, 5, 0),           # dword path, fewer rows than waves in a workgroup
    (7, 768, 100),       # the model's width, a large row mean
    (4, 'W', 0),         # both sides of the switch-over
    (4, 'W+4', 0),
    (5, 8192, 100),      # the widest row
    (3, 8190, 0),        # wide and unaligned
    ('Rg', 8, 100),      # the row walk and the partial reduction
]
_DATA = {}


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _norm(kind, x, w, b, native):
    """y of the kind's normalisation: native kernels, or F.* in the dtype of x."""
    w = None if kind == 'plain' else w
    b = b if kind == 'affine' else None
    if kind == 'rms':
        return (native_rms_norm(x, w, EPS) if native
                else F.rms_norm(x, x.shape[-1:], w, EPS))
    return (native_layer_norm(x, w, b, EPS) if native
            else F.layer_norm(x, x.shape[-1:], w, b, EPS))


def _run(kind, x, w, b, dy, native=False, dtype=torch.float32):
    """(y, dx, dweight, dbias) with None where the kind has no such parameter."""
    x, w, b = (t.detach().to(dtype).requires_grad_() for t in (x, w, b))
    y = _norm(kind, x, w, b, native)
    wanted = [x] + ([w] if kind != 'plain' else []) + ([b] if kind == 'affine' else [])
    grads = list(torch.autograd.grad(y, wanted, dy.to(dtype))) + [None, None]
    return [y.detach()] + grads[:3]


def _case(k):
    """The case's inputs and, per kind, its fp64 reference and the library's fp32 result."""
    if k not in _DATA:
        sizes = {'W': _wave_row_max(), 'W+4': _wave_row_max() + 4,
                 'Rg': 2 * _backward_sweep_rows(8) + 1}
        r, n, offset = (sizes.get(v, v) for v in CASES[k])
        torch.manual_seed(k)
        x = torch.randn(r, n, device='cuda') + offset
        w = 1 + 0.1 * torch.randn(n, device='cuda')
        b = 0.1 * torch.randn(n, device='cuda')
        dy = torch.randn(r, n, device='cuda')
        refs = {kind: (_run(kind, x, w, b, dy, dtype=torch.float64), _run(kind, x, w, b, dy))
                for kind in KINDS}
        _DATA[k] = ((x, w, b, dy), refs)
    return _DATA[k]


def _check(got, ref, lib, what):
    for name, g, r, li in zip(('y', 'dx', 'dweight', 'dbias'), got, ref, lib):
        assert (g is None) == (r is None), name
        if g is None:
            continue
        err, lib_err = rel_err(g, r), rel_err(li, r)
        print(what, name, f'native {err:.3e} library {lib_err:.3e}')
        assert g.shape == r.shape
        assert err <= max(3 * lib_err, FLOOR), (what, name, err, lib_err)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('k', range(len(CASES)), ids=[str(c) for c in CASES])
def test_against_fp64(k, kind):
    inputs, refs = _case(k)
    ref, lib = refs[kind]
    _check(_run(kind, *inputs, native=True), ref, lib, (CASES[k], kind))


@pytest.mark.parametrize('k', [6, 4], ids=['Rg x 8', '5 x 8192'])
def test_backward_is_reproducible(k):
    (x, w, _, dy), _ = _case(k)
    ops = torch.ops.tgpipe
    _, mean, rstd = ops.layernorm_forward(x, w, None, EPS, False)
    first, second = (ops.layernorm_backward(dy, x, mean, rstd, w, None, None, False, True,
                                            False) for _ in range(2))
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_accumulates_into_grad():
    torch.manual_seed(7)
    layer = NativeLayerNorm(768).cuda()
    with torch.no_grad():
        layer.weight.add_(0.1 * torch.randn(768, device='cuda'))
        layer.bias.add_(0.1 * torch.randn(768, device='cuda'))
    plain = torch.nn.LayerNorm(768).cuda()  # the library, accumulating through autograd
    plain.load_state_dict(layer.state_dict())
    exact = copy.deepcopy(plain).double()
    xs = [torch.randn(70, 768, device='cuda') + 100 for _ in range(3)]
    dys = [torch.randn(70, 768, device='cuda') for _ in range(3)]
    for x, dy in zip(xs[:2], dys[:2]):  # no zero_grad: the reduction kernel adds into .grad
        layer(x).backward(dy)
        plain(x).backward(dy)
        exact(x.double()).backward(dy.double())
    for name in ('weight', 'bias'):
        got, lib, ref = (getattr(m, name).grad for m in (layer, plain, exact))
        err, lib_err = rel_err(got, ref), rel_err(lib, ref)
        print(name, f'native {err:.3e} library {lib_err:.3e}')
        assert err <= max(3 * lib_err, FLOOR), (name, err, lib_err)
    before = (layer.weight.grad.clone(), layer.bias.grad.clone())
    got, lib, ref = (torch.autograd.grad(m(x), [m.weight, m.bias], dy) for m, x, dy in
                     ((layer, xs[2], dys[2]), (plain, xs[2], dys[2]),
                      (exact, xs[2].double(), dys[2].double())))
    for g, li, r in zip(got, lib, ref):  # autograd.grad: returned, .grad untouched
        assert rel_err(g, r) <= max(3 * rel_err(li, r), FLOOR)
    assert torch.equal(layer.weight.grad, before[0]) and torch.equal(layer.bias.grad, before[1])


def test_repeated_backward_over_a_retained_graph():
    (x, w, b, dy), refs = _case(1)
    ref, lib = refs['affine']  # (y, dx, dweight, dbias): fp64, and the library in fp32
    bounds = [max(3 * rel_err(li, r), FLOOR) for li, r in zip(lib[2:], ref[2:])]
    layer = NativeLayerNorm(x.shape[-1], eps=EPS).cuda()
    with torch.no_grad():
        layer.weight.copy_(w)
        layer.bias.copy_(b)
    y = layer(x)
    y.backward(dy, retain_graph=True)
    y.backward(dy, retain_graph=True)  # the second pass adds both gradients as well
    assert rel_err(layer.weight.grad, 2 * ref[2]) <= bounds[0]
    assert rel_err(layer.bias.grad, 2 * ref[3]) <= bounds[1]
    dw, db = torch.autograd.grad(y, [layer.weight, layer.bias], dy)  # a third pass, returned
    assert rel_err(dw, ref[2]) <= bounds[0] and rel_err(db, ref[3]) <= bounds[1]


def test_transformer_lm_on_the_native_norm(monkeypatch):
    calls = []
    apply = layernorm._NativeNorm.apply
    monkeypatch.setattr(layernorm._NativeNorm, 'apply',
                        lambda *args: calls.append(1) or apply(*args))
    torch.manual_seed(2)
    model = transformer_lm(vocab=50, d_model=64, heads=1, layers=1, seq_len=12,
                           native_norm=True).cuda()
    single = transformer_lm(vocab=50, d_model=64, heads=1, layers=1, seq_len=12).cuda()
    single.load_state_dict(model.state_dict())
    tokens = torch.randint(50, (4, 12), device='cuda')
    target = torch.randint(50, (4 * 12,), device='cuda')
    want = F.cross_entropy(single(tokens).flatten(0, 1), target)
    want.backward()
    assert not calls
    pipe = GPipe(model, balance=[2, 2], devices=[0, 0], chunks=2, checkpoint='always')
    loss = F.cross_entropy(pipe(tokens).flatten(0, 1), target)
    loss.backward()
    assert len(calls) >= 3 * 2  # three norms, two micro-batches (and their recomputation)
    torch.testing.assert_close(loss, want, rtol=1e-5, atol=1e-6)
    for (name, p), r in zip(model.named_parameters(), single.parameters()):
        torch.testing.assert_close(p.grad, r.grad, rtol=1e-4, atol=1e-6, msg=name)
