"""Whole models in ``eval()`` under ``no_grad`` on the native eval-mode ops (ops/convbn.py
``conv_bn_eval``, ops/fusion.py ``bn_eval_act``): numerics against fp64 eager copies, which
layers dispatch where, and the same function through the pipeline engine."""
import copy

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd import GPipe
from torchgpipe_amd.ops import _ext, convbn, fusion

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _build(kind):
    if kind == 'amoebanet':
        from torchgpipe_amd.models import amoebanetd
        torch.manual_seed(4)
        model = amoebanetd(num_classes=10, num_layers=3, num_filters=64).cuda()
        x = torch.rand(8, 3, 224, 224, device='cuda')
    else:
        from torchgpipe_amd.models.resnet import build_resnet
        torch.manual_seed(0)
        model = build_resnet([1, 1, 1, 1], num_classes=10, fused=True).cuda()
        x = torch.randn(4, 3, 96, 96, device='cuda')
    return model, x


_TRAINED = {}  # kind -> (model after one training step, in eval mode; input; fp64 logits)


@pytest.fixture(scope='module', autouse=True)
def release_models():
    yield
    _TRAINED.clear()


def _trained(kind):
    """The tiny model after one training step (running statistics off their initial 0 / 1),
    switched to eval, with the logits of its fp64 eager copy: built once."""
    if kind not in _TRAINED:
        model, x = _build(kind)
        t = torch.randint(10, (x.shape[0],), device='cuda')
        F.cross_entropy(model(x), t).backward()
        model.zero_grad(set_to_none=True)
        model.eval()
        ref = copy.deepcopy(model).double()
        with torch.no_grad(), convbn.disabled():
            want = ref(x.double())
        _TRAINED[kind] = (model, x, want)
    return _TRAINED[kind]


@pytest.mark.parametrize('kind', ['amoebanet', 'resnet'])
def test_eval_logits_match_fp64_eager(kind):
    """Logits within 1e-4 of the fp64 eager copy: ten layers' worth of the per-op 1e-5.  The
    eager fp32 model's own distance from fp64 is printed beside it."""
    model, x, want = _trained(kind)
    with torch.no_grad():
        got = model(x)
        with convbn.disabled():
            eager = copy.deepcopy(model)(x)
    err, eager_err = rel_err(got, want), rel_err(eager, want)
    print(f'{kind}: eval logits vs fp64: native {err:.2e}, eager fp32 {eager_err:.2e}')
    assert err < 1e-4


def _count(monkeypatch, owner, name, calls):
    inner = getattr(owner, name)

    def counted(*args, **kwargs):
        calls.append((name, args[0] if name == 'forward' else None))
        return inner(*args, **kwargs)

    monkeypatch.setattr(owner, name, counted)


def test_resnet_eval_runs_every_linked_convolution_natively(monkeypatch):
    model, x, _ = _trained('resnet')
    linked = fusion.relink(model)
    assert linked > 0
    native, eager = [], []
    _count(monkeypatch, convbn, 'conv_bn_eval', native)
    _count(monkeypatch, fusion, 'bn_eval_act', native)
    _count(monkeypatch, nn.BatchNorm2d, 'forward', eager)
    with torch.no_grad():
        model(x)
    assert len(native) == linked, (len(native), linked)
    assert not eager
    names = {n for n, _ in native}
    assert names == {'conv_bn_eval', 'bn_eval_act'}  # (pointwise + joins; Winograd + strided)


def test_amoebanet_eval_reaches_no_eager_batchnorm_in_a_fused_chain(monkeypatch):
    model, x, _ = _trained('amoebanet')
    in_chains = {id(m) for chain in model.modules() if isinstance(chain, convbn.FusedChain)
                 for m in chain.children() if isinstance(m, nn.BatchNorm2d)}
    assert in_chains
    native, eager = [], []
    _count(monkeypatch, convbn, 'conv_bn_eval', native)
    _count(monkeypatch, nn.BatchNorm2d, 'forward', eager)
    with torch.no_grad():
        model(x)
    assert not [bn for _, bn in eager if id(bn) in in_chains]
    assert len(native) >= len(in_chains)


@pytest.mark.parametrize('kind', ['amoebanet', 'resnet'])
def test_gpipe_eval_equals_the_unpipelined_model(kind):
    """Two partitions on one GPU, two micro-batches: the same kernels on half the batch.
    Both partitions are on one device, so the copies go on the current stream (what
    ``Pipeline`` does without copy streams) and this test makes no stream of its own: a ring
    of new ones would move every later test's streams along the round-robin stream pool, and
    with that onto other hardware queues."""
    model, x, _ = _trained(kind)
    with torch.no_grad():
        want = model(x)
    piped = copy.deepcopy(model)
    n = len(piped)
    gpipe = GPipe(piped, [n // 2, n - n // 2], devices=[0, 0], chunks=2).eval()
    gpipe._copy_streams = [[torch.cuda.current_stream(d)] * gpipe.chunks for d in gpipe.devices]
    keys = list(gpipe.state_dict())
    with torch.no_grad():
        got = gpipe(x)
    assert list(gpipe.state_dict()) == keys
    err = rel_err(got, want)
    print(f'{kind}: pipelined eval vs unpipelined: {err:.2e}')
    assert err < 1e-6
