"""The native Linear kernels (csrc/linear.hip, ops/linear.py) on the GPU: every pass against
the fp64 oracle of the level's partial products on both tiles, the quad, dword and split
paths; the knob's reach; accumulation into .grad; and a pipeline through NativeLinear."""
import pytest
import torch
from torch import nn

from torchgpipe_amd import GPipe
from torchgpipe_amd.ops import _ext, precision
from torchgpipe_amd.ops.linear import NativeLinear, force_plan
from torchgpipe_amd.ops.precision import reference_linear, reference_linear_backward

pytestmark = pytest.mark.gpu

Y_TOL, DW_TOL = 2e-6, 5e-6            # y, dx, db / dw against the level's oracle
AWAY = {'high': 3e-6, 'medium': 1e-3}  # y, dx at least this far from the exact result


@pytest.fixture(autouse=True)
def need_gpu_and_restore():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()
    assert precision.get_conv_precision() == 'highest'
    try:
        yield
    finally:
        precision.set_conv_precision('highest')
        force_plan(-1, -1)


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# (x shape, O, forced splits): one staging / reduction path each
CASES = [
    ((3, 20), 12, -1),      # inside one tile, tails in all three dimensions, quad path
    ((130, 72), 136, -1),   # one past a 128 tile in M and N; K = two stages and a quarter
    ((5, 37), 10, -1),      # nothing a multiple of 4: dword staging of every operand
    ((64, 1024), 40, 4),    # split reduction with bias; accumulate on the split weight grad
    ((2, 7, 32), 24, -1),   # leading dimensions flattened
]
_DATA = {}


def _data(k):
    if k not in _DATA:
        shape, o, _ = CASES[k]
        torch.manual_seed(k)
        x = torch.randn(*shape, device='cuda')
        w = torch.randn(o, shape[-1], device='cuda') / shape[-1] ** 0.5
        b = 0.1 * torch.randn(o, device='cuda')
        dy = torch.randn(*shape[:-1], o, device='cuda')
        g0 = torch.randn(o, shape[-1], device='cuda')  # an existing weight gradient
        _DATA[k] = (x, w, b, dy, g0)
    return _DATA[k]


@pytest.mark.parametrize('tile', [64, 128])
@pytest.mark.parametrize('level', precision.LEVELS)
@pytest.mark.parametrize('k', range(len(CASES)), ids=[f'{c[0]}x{c[1]}' for c in CASES])
def test_products_of_the_level(k, level, tile):
    x, w, b, dy, g0 = _data(k)
    ops = torch.ops.tgpipe
    force_plan(tile, CASES[k][2])
    with precision.conv_precision(level):
        y = ops.linear_forward(x, w, b)
        dx = ops.linear_backward_data(dy, w)
        dw = ops.linear_backward_weight(dy, x, None, False)
        acc = ops.linear_backward_weight(dy, x, g0.clone(), True)
        db = ops.linear_bias_grad(dy, None, False)
    y_ref = reference_linear(x, w, b, level)
    dx_ref, dw_ref, db_ref = reference_linear_backward(dy, x, w, level)
    errs = {'y': rel_err(y, y_ref), 'dx': rel_err(dx, dx_ref), 'dw': rel_err(dw, dw_ref),
            'acc': rel_err(acc, g0.double() + dw_ref), 'db': rel_err(db, db_ref)}
    print(CASES[k], level, tile, errs)
    assert y.shape == y_ref.shape and dx.shape == x.shape and dw.shape == w.shape
    assert max(errs['y'], errs['dx'], errs['db']) < Y_TOL, errs
    assert max(errs['dw'], errs['acc']) < DW_TOL, errs
    if level != 'highest':
        exact = (rel_err(y, reference_linear(x, w, b)),
                 rel_err(dx, reference_linear_backward(dy, x, w)[0]))
        assert min(exact) > AWAY[level], exact


def test_highest_untouched_by_the_knob():
    x, w, b, _, _ = _data(1)
    ops = torch.ops.tgpipe
    first = ops.linear_forward(x, w, b)
    with precision.conv_precision('medium'):
        second = ops.linear_forward(x, w, b)
    third = ops.linear_forward(x, w, b)
    assert torch.equal(first, third)
    assert not torch.equal(first, second)


def test_accumulates_into_grad():
    torch.manual_seed(7)
    layer = NativeLinear(72, 136).cuda()
    xs = [torch.randn(130, 72, device='cuda') for _ in range(2)]
    dys = [torch.randn(130, 136, device='cuda') for _ in range(2)]
    refs = [reference_linear_backward(dy, x, layer.weight) for x, dy in zip(xs, dys)]
    assert layer.weight.grad is None
    layer(xs[0]).backward(dys[0])
    assert rel_err(layer.weight.grad, refs[0][1]) < DW_TOL
    assert rel_err(layer.bias.grad, refs[0][2]) < Y_TOL
    layer(xs[1]).backward(dys[1])  # no zero_grad: the epilogue adds into .grad
    assert rel_err(layer.weight.grad, refs[0][1] + refs[1][1]) < DW_TOL
    assert rel_err(layer.bias.grad, refs[0][2] + refs[1][2]) < Y_TOL


def test_through_the_pipeline():
    torch.manual_seed(3)
    model = nn.Sequential(NativeLinear(72, 136), nn.ReLU(), NativeLinear(136, 10))
    plain = nn.Sequential(nn.Linear(72, 136), nn.ReLU(), nn.Linear(136, 10))
    plain.load_state_dict(model.state_dict())  # the same keys, unchanged
    plain = plain.double().cuda()
    pipe = GPipe(model, balance=[3], devices=['cuda:0'], chunks=2, checkpoint='always')
    x = torch.randn(12, 72, device='cuda')
    loss = pipe(x).square().mean()
    loss.backward()
    ref = plain(x.double()).square().mean()
    ref.backward()
    assert rel_err(loss, ref) < Y_TOL
    for (name, p), q in zip(model.named_parameters(), plain.parameters()):
        assert rel_err(p.grad, q.grad) < (DW_TOL if p.dim() == 2 else Y_TOL), name
