"""The native cross-entropy kernels (csrc/cross_entropy.hip, ops/loss.py) on the GPU: every path
against F.cross_entropy in fp64 with the library's own fp32 error as the yardstick, bitwise
reproducibility, what the forward keeps alive, logits beyond 2 GiB, and a transformer_lm
pipeline under NativeCrossEntropyLoss.

Label smoothing over a logit of -inf makes the loss +inf in the library too, and both give such
a column the gradient -s eps / V: there the loss has to be the same +inf, and the exact zero
at -inf columns is asked of the kinds without smoothing."""
import copy

import pytest
import torch
import torch.nn.functional as F

from torchgpipe_amd import GPipe
from torchgpipe_amd.models.transformer import transformer_lm
from torchgpipe_amd.ops import _ext, loss as loss_ops
from torchgpipe_amd.ops.loss import (NativeCrossEntropyLoss, _force_instance, _limits,
                                     native_cross_entropy)

pytestmark = pytest.mark.gpu

FLOOR = 5e-7  # native error <= max(3 x the library's fp32 error, FLOOR)
IGNORE = -100
# kind: (reduction, every third row ignored, label smoothing)
KINDS = {'mean': ('mean', False, 0.0), 'sum': ('sum', False, 0.0), 'none': ('none', False, 0.0),
         'mean+ignore': ('mean', True, 0.0), 'mean+smooth': ('mean', False, 0.1),
         'none+ignore+smooth': ('none', True, 0.1)}
# (R, V); 'W' = the wave-per-row instances' widest row, 'C' / 'C4' = a backward chunk's columns
# on the dword / float4 path
CASES = [
    (3, 5),          # dword path, fewer rows than waves in a workgroup
    (7, 1000),       # a classifier's width; -inf columns and one dominant logit
    (5, 'W'),        # both sides of the switch-over
    (5, 'W+4'),
    (3, 32000),      # wide float4 path
    (4, 50257),      # wide dword path; row bases at all four alignments
    (2, 128256),     # many iterations per lane
    (3, 'C+1'),      # one column more than a backward chunk
    (3, 'C4+4'),     # the same with float4 accesses
]
MASKED = slice(100, 200)  # the -inf columns of case 1
_DATA = {}


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _run(kind, x, t, g, native=False, dtype=torch.float32):
    """(loss, dx) of the kind, upstream gradient 0.37 (or g per row): the native kernels, or
    F.cross_entropy in `dtype`."""
    reduction, ignore, eps = KINDS[kind]
    x = x.detach().to(dtype).requires_grad_()
    if ignore:
        t = t.clone()
        t[::3] = IGNORE
    fn = native_cross_entropy if native else F.cross_entropy
    loss = fn(x, t, ignore_index=IGNORE, reduction=reduction, label_smoothing=eps)
    out = (loss * g.to(dtype)).sum() if reduction == 'none' else loss * 0.37
    return loss.detach(), torch.autograd.grad(out, x)[0]


def _case(k, kind):
    """The case's inputs with the kind's fp64 reference and the library's fp32 result."""
    if k not in _DATA:
        wave_row_max, chunk4, chunk = _limits()
        sizes = {'W': wave_row_max, 'W+4': wave_row_max + 4, 'C+1': chunk + 1,
                 'C4+4': chunk4 + 4}
        r, v = (sizes.get(n, n) for n in CASES[k])
        torch.manual_seed(k)
        x = 4 * torch.randn(r, v, device='cuda') + 30
        t = torch.randint(v, (r,), device='cuda')
        if k == 1:
            x[:, MASKED] = float('-inf')
            x[2, 7] = x[2, 200:].max() + 80
            t[(t >= MASKED.start) & (t < MASKED.stop)] += 100  # no masked class is a target
        _DATA[k] = ((x, t, torch.randn(r, device='cuda')), {})
    inputs, refs = _DATA[k]
    if kind not in refs:
        refs[kind] = (_run(kind, *inputs, dtype=torch.float64), _run(kind, *inputs))
    return inputs, refs[kind]


def _check(got, ref, lib, what):
    for name, g, r, li in zip(('loss', 'dx'), got, ref, lib):
        assert g.shape == r.shape and g.dtype == torch.float32
        finite = torch.isfinite(r)
        assert torch.equal(g[~finite].double(), r[~finite]), (what, name)
        err, lib_err = rel_err(g[finite], r[finite]), rel_err(li[finite], r[finite])
        print(what, name, f'native {err:.3e} library {lib_err:.3e}')
        assert err <= max(3 * lib_err, FLOOR), (what, name, err, lib_err)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('k', range(len(CASES)), ids=[str(c) for c in CASES])
def test_against_fp64(k, kind):
    inputs, (ref, lib) = _case(k, kind)
    loss, dx = _run(kind, *inputs, native=True)
    _check((loss, dx), ref, lib, (CASES[k], kind))
    _, ignore, eps = KINDS[kind]
    if ignore:
        assert (dx[::3] == 0).all()
    if k == 1 and eps == 0:
        assert (dx[:, MASKED] == 0).all()


def test_all_rows_ignored():
    (x, t, g), _ = _case(1, 'mean')
    t = torch.full_like(t, IGNORE)
    x = x.clone().requires_grad_()
    assert native_cross_entropy(x, t).isnan() and F.cross_entropy(x, t).isnan()
    total = native_cross_entropy(x, t, reduction='sum')
    assert total.item() == 0
    assert (torch.autograd.grad(total, x)[0] == 0).all()


def test_is_reproducible():
    for k in (5, 2):
        inputs, _ = _case(k, 'mean+smooth')
        first, second = (_run('mean+smooth', *inputs, native=True) for _ in range(2))
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    inputs, (ref, lib) = _case(2, 'mean+smooth')
    try:
        for wide in (0, 1):
            _force_instance(wide)
            _check(_run('mean+smooth', *inputs, native=True), ref, lib, ('forced', wide))
    finally:
        _force_instance(-1)


def test_keeps_no_softmax():
    mib = 1 << 20
    x = torch.randn(2048, 8192, device='cuda').requires_grad_()  # 64 MiB
    t = torch.randint(8192, (2048,), device='cuda')
    before = torch.cuda.memory_allocated()
    loss = native_cross_entropy(x, t)
    assert torch.cuda.memory_allocated() - before < mib  # two floats a row, row losses, scalars
    loss.backward()
    assert 64 * mib <= torch.cuda.memory_allocated() - before < 65 * mib  # and dx
    library = F.cross_entropy(x, t)
    assert torch.cuda.memory_allocated() - before >= 128 * mib  # the library's log-softmax
    del library


def test_beyond_2gib():
    if torch.cuda.mem_get_info()[0] < 10 << 30:
        pytest.skip('needs 10 GiB of free device memory')
    r, v = 16400, 32768  # 2.15 GB of logits
    torch.manual_seed(3)
    x = torch.randn(r, v, device='cuda').mul_(4).add_(30).requires_grad_()
    t = torch.randint(v, (r,), device='cuda')
    g = torch.randn(r, device='cuda')
    loss = native_cross_entropy(x, t, reduction='none')
    want = torch.cat([F.cross_entropy(x.detach()[i:i + 1024], t[i:i + 1024], reduction='none')
                      for i in range(0, r, 1024)])
    torch.testing.assert_close(loss.detach(), want, rtol=1e-5, atol=0)
    dx, = torch.autograd.grad(loss, x, g)

    def library_dx(rows, dtype):
        xs = x.detach()[rows].to(dtype).requires_grad_()
        rows_loss = F.cross_entropy(xs, t[rows], reduction='none')
        return torch.autograd.grad(rows_loss, xs, g[rows].to(dtype))[0]

    for rows in (slice(0, 4), slice(r - 4, r)):
        ref, lib = library_dx(rows, torch.float64), library_dx(rows, torch.float32)
        err, lib_err = rel_err(dx[rows], ref), rel_err(lib, ref)
        print(rows, f'native {err:.3e} library {lib_err:.3e}')
        assert err <= max(3 * lib_err, FLOOR), (rows, err, lib_err)


def test_transformer_lm_with_the_native_loss(monkeypatch):
    calls = []
    apply = loss_ops._NativeCrossEntropy.apply
    monkeypatch.setattr(loss_ops._NativeCrossEntropy, 'apply',
                        lambda *args: calls.append(1) or apply(*args))
    torch.manual_seed(2)
    model = transformer_lm(vocab=50, d_model=64, heads=1, layers=1, seq_len=12).cuda()
    single = copy.deepcopy(model)
    tokens = torch.randint(50, (4, 12), device='cuda')
    target = torch.randint(50, (4 * 12,), device='cuda')
    want = F.cross_entropy(single(tokens).flatten(0, 1), target)
    want.backward()
    assert not calls
    pipe = GPipe(model, balance=[2, 2], devices=[0, 0], chunks=2, checkpoint='always')
    loss = NativeCrossEntropyLoss()(pipe(tokens).flatten(0, 1), target)
    loss.backward()
    assert len(calls) == 1
    torch.testing.assert_close(loss, want, rtol=1e-5, atol=1e-6)
    for (name, p), r in zip(model.named_parameters(), single.parameters()):
        torch.testing.assert_close(p.grad, r.grad, rtol=1e-4, atol=1e-6, msg=name)
