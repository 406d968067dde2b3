"""The head-dim-128 attention kernels (csrc/attention128.hip) on the GPU, as
test_attention_gpu.py tests the head-dim-64 ones: forward and backward against the fp64 oracle
of the level's products at the shapes where the kernels can go wrong, determinism, and
NativeSelfAttention through a pipeline.

Measured on an MI355X: see profiles/r18/attention128/README.md."""
import pytest
import torch
import torch.nn.functional as F

from torchgpipe_amd import GPipe
from torchgpipe_amd.ops import _ext, precision
from torchgpipe_amd.ops.attention import NativeSelfAttention, eligible, native_attention
from torchgpipe_amd.ops.precision import reference_attention, reference_attention_backward

pytestmark = pytest.mark.gpu

D = 128
Y_TOL, DW_TOL = 2e-6, 5e-6             # test_attention_gpu.py: test_through_the_pipeline
AWAY = {'high': 3e-6, 'medium': 1e-3}  # test_attention_gpu.py: o at least this far from exact


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


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# (B, H, T): a single key; one past a wave's 32 queries and a 32-key block; one past the
# workgroup's 128 rows; strided views of one [B, T, 3, H, 128] tensor with q scaled by 8
CASES = [(1, 1, 1), (2, 3, 33), (1, 2, 130), (1, 2, 200)]
_DATA = {}


def _data(i):
    if i not in _DATA:
        b, h, t = CASES[i]
        torch.manual_seed(i)
        if i == 3:
            qkv = torch.randn(b, t, 3, h, D, device='cuda')
            qkv[:, :, 0] *= 8
            q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
            assert not q.is_contiguous()
        else:
            q, k, v = (torch.randn(b, h, t, D, device='cuda') for _ in range(3))
        _DATA[i] = (q, k, v, torch.randn(b, h, t, D, device='cuda'))
    return _DATA[i]


def _run(fn, q, k, v, do, causal):
    leaves = [t.detach().requires_grad_() for t in (q, k, v)]
    o = fn(*leaves, causal)
    return (o.detach(),) + torch.autograd.grad(o, leaves, do)


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('level', precision.LEVELS)
@pytest.mark.parametrize('i', range(len(CASES)), ids=[str(c) for c in CASES])
def test_products_of_the_level(i, level, causal):
    q, k, v, do = _data(i)
    with precision.conv_precision(level):
        got = _run(native_attention, q, k, v, do, causal)
    assert got[0].shape == q.shape and got[0].transpose(1, 2).is_contiguous()
    exact = (reference_attention(q, k, v, causal),) + \
        reference_attention_backward(do, q, k, v, causal)
    names = ('o', 'dq', 'dk', 'dv')
    if level == 'highest':
        lib = _run(lambda a, b, c, cs: F.scaled_dot_product_attention(a, b, c, is_causal=cs),
                   q, k, v, do, causal)
        errs = {n: (rel_err(g, e), rel_err(t, e)) for n, g, t, e in zip(names, got, lib, exact)}
        print(CASES[i], level, causal, errs)
        for n, (mine, torchs) in errs.items():
            assert mine <= 2 * torchs, (n, mine, torchs)
        return
    oracle = (reference_attention(q, k, v, causal, level=level),) + \
        reference_attention_backward(do, q, k, v, causal, level=level)
    errs = {n: (rel_err(g, r), rel_err(r, e), rel_err(g, e))
            for n, g, r, e in zip(names, got, oracle, exact)}
    print(CASES[i], level, causal, errs)
    if CASES[i][2] == 1:  # softmax over one key is 1: the levels differ in P V alone
        return
    for n, (to_oracle, oracle_to_exact, _) in errs.items():
        assert to_oracle < 0.5 * oracle_to_exact, (n, to_oracle, oracle_to_exact)
    assert errs['o'][2] > AWAY[level], errs['o']


def test_deterministic():
    q, k, v, do = _data(2)
    first, second = (_run(native_attention, q, k, v, do, True) for _ in range(2))
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_through_the_pipeline():
    torch.manual_seed(3)
    layer = NativeSelfAttention(256, 2, causal=True, native_linear=True)
    ref = NativeSelfAttention(256, 2, causal=True)
    ref.load_state_dict(layer.state_dict())
    ref = ref.double().cuda()  # fp64: F.scaled_dot_product_attention's math path
    pipe = GPipe(torch.nn.Sequential(layer), balance=[1], devices=['cuda:0'], chunks=2,
                 checkpoint='always')
    x = torch.randn(4, 40, 256, device='cuda')
    with torch.no_grad():
        qkv = layer.qkv(x).view(4, 40, 3, 2, D)
    assert eligible(*(qkv[:, :, j].transpose(1, 2) for j in range(3)))
    assert not eligible(*(torch.randn(1, 2, 40, 96, device='cuda') for _ in range(3)))
    loss = pipe(x).square().mean()
    loss.backward()
    want = ref(x.double()).square().mean()
    want.backward()
    assert rel_err(loss, want) < Y_TOL
    for (name, p), r in zip(layer.named_parameters(), ref.parameters()):
        assert rel_err(p.grad, r.grad) < (DW_TOL if p.dim() == 2 else Y_TOL), name
