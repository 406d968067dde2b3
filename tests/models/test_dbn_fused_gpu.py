"""``deferred_batch_norm=True`` on the two BatchNorm benchmark models: the pipeline engines
train them on the fused native ops (DeferredBatchNorm accepted wherever a BatchNorm2d is),
judged against the same engine around an fp64 copy, whose layers run eagerly by construction."""
import collections
import copy
import statistics

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd import GPipe
from torchgpipe_amd.batchnorm import DeferredBatchNorm
from torchgpipe_amd.models import amoebanet as amoebanet_module
from torchgpipe_amd.ops import _ext, convbn, fusion
from torchgpipe_amd.parallel import PipelineStage

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


_MODELS = {}  # kind -> (model, input, target), built once and only ever copied


@pytest.fixture(scope='module', autouse=True)
def release_models():
    yield
    _MODELS.clear()


def _build(kind):
    """The tiny models of tests/models/test_eval_fused_gpu.py."""
    if kind not in _MODELS:
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
        t = torch.randint(10, (x.shape[0],), device='cuda')
        _MODELS[kind] = (model, x, t)
    model, x, t = _MODELS[kind]
    return copy.deepcopy(model), x, t


def _gpipe(model, checkpoint):
    gpipe = GPipe(model, [len(model)], devices=[0], chunks=2, checkpoint=checkpoint,
                  deferred_batch_norm=True)
    # One device: the copies go on the current stream and the test makes no stream of its
    # own.  GPipe has no public switch for this; it takes its copy streams from its pool on
    # the first forward only while this list is empty (``_ensure_copy_streams``), so filling
    # it before any forward is what tests/models/test_eval_fused_gpu.py does too.
    gpipe._copy_streams = [[torch.cuda.current_stream(d)] * gpipe.chunks for d in gpipe.devices]
    return gpipe


def _gpipe_step(model, x, t, checkpoint, prepare=None):
    gpipe = _gpipe(model, checkpoint)
    if prepare is not None:
        prepare(gpipe)
    loss = F.cross_entropy(gpipe(x), t)
    loss.backward()
    return gpipe, loss.detach()


def _record_relu_outputs(gpipe, seen):
    """Every ReLU layer's outputs in the forwards that autograd differentiates (under
    checkpointing: the recomputations), by layer name."""
    for name, m in gpipe.named_modules():
        if isinstance(m, nn.ReLU):
            m.register_forward_hook(
                lambda mod, args, out, name=name:
                seen.setdefault(name, []).append(out.detach()) if out.requires_grad else None)


def _follow_relu_decisions(ref, seen, flips):
    """Make the fp64 reference rectify as the fp32 model under test did.

    A pre-activation within fp32 rounding of zero may fall on either side of it, and each such
    element moves a whole gradient element for everything before it -- for any fp32
    implementation (tests/models/test_resnet_fused_gpu.py applies the forward's own decisions
    to its fp64 layers for the same reason).  Here one element of ``layer3_0_relu3`` is 0 in
    fp64 and 3e-7 .. 9e-7 in about half of the fused runs (the last bits of that forward are
    not reproducible), which alone puts the 39 parameters before ``layer4`` 3.5e-3 .. 5.5e-3
    off.  Decisions may differ only where both values are within 1e-5 of zero relative to the
    layer's largest (the per-operation output bound); anything else fails here."""
    for m in ref.modules():
        inner = getattr(m, 'module', m)
        if getattr(inner, 'fuses_relu', False):
            # (the residual join leaves its ReLU to the ReLU layer: the same function in fp64)
            inner.__dict__.pop('_tgpipe_relu_next', None)

    def hook(mod, args, out, name):
        pre = args[0]
        own = pre > 0
        outs = [y for y in seen[name] if y.shape == pre.shape]
        assert outs, name
        y = min(outs, key=lambda y: ((y > 0) != own).sum().item())
        diff = (y > 0) != own
        if diff.any():
            tiny = 1e-5 * pre.abs().max().item()
            assert pre[diff].abs().max().item() < tiny and y[diff].abs().max().item() < tiny, name
            flips.append((name, int(diff.sum())))
        return pre * (y > 0).to(pre.dtype)

    for name, m in ref.named_modules():
        if isinstance(m, nn.ReLU):
            m.register_forward_hook(lambda mod, args, out, name=name: hook(mod, args, out, name))


def _check_buffers(got, want):
    names = [n for n, _ in got.named_buffers()]
    assert names == [n for n, _ in want.named_buffers()]
    worst = 0.0
    for (name, a), b in zip(got.named_buffers(), want.buffers()):
        if not a.is_floating_point():
            assert torch.equal(a, b), (name, a, b)  # num_batches_tracked
        elif name.rsplit('.', 1)[-1] in ('running_mean', 'running_var'):
            err = rel_err(a, b)
            worst = max(worst, err)
            assert err < 1e-5, (name, err)
    return worst


@pytest.mark.parametrize('checkpoint', ['always', 'never'])
@pytest.mark.parametrize('kind', ['amoebanet', 'resnet'])
def test_gpipe_training_step_matches_the_fp64_wrap(kind, checkpoint):
    """One training step, two micro-batches.  Loss and gradients at the bounds of the plain
    fused models (tests/ops/test_convbn_gpu.py test_amoebanet_fused_matches_fp64_eager,
    tests/models/test_resnet_fused_gpu.py: the eager fp32 wrap is the yardstick for the
    ill-conditioned deep gradients), running buffers within 1e-5, and the batch counters
    equal -- under ``always`` every micro-batch is recomputed, which must not track.

    Measured (worst parameter, fused / eager fp32): ResNet 1.4e-05 / 5.2e-06, AmoebaNet
    1.3e-02 / 1.0e-02; worst running buffer 7.3e-07 / 4.7e-07.

    The fp64 ResNet rectifies with the fused run's decisions (``_follow_relu_decisions``)."""
    model, x, t = _build(kind)
    ref, plain = copy.deepcopy(model).double(), copy.deepcopy(model)
    seen, flips = {}, []
    fused, loss = _gpipe_step(model, x, t, checkpoint,
                              lambda g: _record_relu_outputs(g, seen))
    assert any(isinstance(m, DeferredBatchNorm) for m in fused.modules())
    with convbn.disabled():
        eager, _ = _gpipe_step(plain, x, t, checkpoint)
    # (ResNet's ReLUs are layers; AmoebaNet's are read by the fused ops and its bounds are
    # statistical for this very reason)
    follow = (lambda g: _follow_relu_decisions(g, seen, flips)) if kind == 'resnet' else None
    want, loss64 = _gpipe_step(ref, x.double(), t, checkpoint, follow)
    assert abs(loss.item() - loss64.item()) < 1e-5 * max(1.0, abs(loss64.item()))
    errs_f, errs_e = [], []
    for (name, p), q, r in zip(fused.named_parameters(), eager.parameters(), want.parameters()):
        assert p.grad is not None and r.grad is not None, name
        errs_f.append(rel_err(p.grad, r.grad))
        errs_e.append(rel_err(q.grad, r.grad))
        if kind == 'amoebanet':
            assert errs_f[-1] < 1e-1, (name, errs_f[-1], errs_e[-1])
        else:
            # (tests/models/test_resnet_fused_gpu.py: max(1e-3, 8 x eager); the eager figure
            # is printed only, so that an eager run deciding a ReLU otherwise widens nothing)
            assert errs_f[-1] < 1e-3, (name, errs_f[-1], errs_e[-1])
    med_f, med_e = statistics.median(errs_f), statistics.median(errs_e)
    if kind == 'amoebanet':
        assert med_f <= 2 * med_e + 1e-6, (med_f, med_e)
    worst = _check_buffers(fused, want)
    print(f'{kind} {checkpoint}: gradient error median fused {med_f:.2e} eager {med_e:.2e}, '
          f'worst fused {max(errs_f):.2e} eager {max(errs_e):.2e}; worst buffer {worst:.2e}; '
          f'ReLU decisions taken from the fused run: {flips}')
    for m in fused.modules():
        if isinstance(m, DeferredBatchNorm):
            assert m.num_batches_tracked.item() == 1 and m.tracked == 0


@pytest.mark.parametrize('kind', ['amoebanet', 'resnet'])
def test_pipeline_stage_statistics_after_three_steps(kind):
    model, x, t = _build(kind)
    ref = copy.deepcopy(model).double()
    dev = torch.device('cuda', 0)
    stage = PipelineStage(model, [len(model)], device=dev, chunks=2, deferred_batch_norm=True)
    want = PipelineStage(ref, [len(ref)], device=dev, chunks=2, deferred_batch_norm=True)
    for _ in range(3):
        loss = stage.train_step(x, t, F.cross_entropy)
        loss64 = want.train_step(x.double(), t, F.cross_entropy)
    torch.cuda.synchronize()
    assert abs(loss.item() - loss64.item()) < 1e-5 * max(1.0, abs(loss64.item()))
    worst = _check_buffers(stage.partition, want.partition)
    print(f'{kind}: worst running buffer after 3 steps {worst:.2e}')
    for m in stage.partition.modules():
        if isinstance(m, DeferredBatchNorm):
            assert m.num_batches_tracked.item() == 3


def _census(monkeypatch, model, x):
    """Calls of the fused ops (by name) and of the eager BatchNorm forwards in one forward."""
    calls = collections.Counter()

    def counted(owner, name, key):
        inner = getattr(owner, name)

        def wrapper(*args, **kwargs):
            calls[key] += 1
            return inner(*args, **kwargs)
        monkeypatch.setattr(owner, name, wrapper)

    for name in ('relu_conv_bn', 'group_relu_conv_bn', 'bn_act'):
        # (each module that calls the op holds its own reference to it)
        inner = getattr(convbn if hasattr(convbn, name) else fusion, name)
        for owner in (convbn, fusion, amoebanet_module):
            if getattr(owner, name, None) is inner:
                counted(owner, name, name)
    counted(F, 'batch_norm', 'eager')
    counted(nn.BatchNorm2d, 'forward', 'eager')
    model(x)
    return calls


@pytest.mark.parametrize('kind', ['amoebanet', 'resnet'])
def test_dispatch_census_is_the_plain_models(kind, monkeypatch):
    """One micro-batch through the model with the option on calls the fused ops exactly as
    often as with it off, and no eager BatchNorm."""
    off, x, _ = _build(kind)
    on = DeferredBatchNorm.convert_deferred_batch_norm(copy.deepcopy(off), chunks=2).cuda()
    fusion.relink(off)
    fusion.relink(on)
    with monkeypatch.context() as mp:
        want = _census(mp, off, x)
    with monkeypatch.context() as mp:
        got = _census(mp, on, x)
    print(f'{kind}: off {dict(want)} on {dict(got)}')
    fused_ops = ('relu_conv_bn', 'group_relu_conv_bn', 'bn_act')
    assert sum(want[k] for k in fused_ops) > 0
    assert [got[k] for k in fused_ops] == [want[k] for k in fused_ops]
    assert got['eager'] == 0  # neither F.batch_norm nor nn.BatchNorm2d.forward


def test_captured_cells_commit_like_the_eager_stage():
    """The small model of tests/test_segments.py
    ``test_graph_cells_deferred_batch_norm_commits`` on the fused layers: the commits inside
    the captured forwards leave the buffers the eager stage's have."""
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    base = nn.Sequential(fusion.ConvBN2d(3, 8, 3, padding=1, bias=False),
                         fusion.BatchNormAct2d(8), fusion.ReLU(),
                         fusion.ConvBN2d(8, 4, 3, padding=1, bias=False),
                         fusion.BatchNormAct2d(4), nn.Flatten(), nn.Linear(4 * 8 * 8, 3))
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    sa = PipelineStage(a, [len(a)], device=dev, chunks=4, deferred_batch_norm=True)
    sb = PipelineStage(b, [len(b)], device=dev, chunks=4, deferred_batch_norm=True,
                       graph_cells=True)
    for stage in (sa, sb):
        assert stage.partition[0].__dict__['_tgpipe_link'][0] is stage.partition[1]
        assert type(stage.partition[1]) is DeferredBatchNorm
    gen = torch.Generator(device=dev).manual_seed(3)
    for _ in range(5):
        x = torch.randn(8, 3, 8, 8, device=dev, generator=gen) * 2 + 1
        y = torch.randint(3, (8,), device=dev, generator=gen)
        sa.train_step(x, y, F.cross_entropy)
        sb.train_step(x, y, F.cross_entropy)
    torch.cuda.synchronize()
    assert sb.graph_phase == 'replay'
    for (name, ba), bb in zip(sa.partition.named_buffers(), sb.partition.buffers()):
        if ba.is_floating_point():
            torch.testing.assert_close(bb, ba, rtol=1e-5, atol=1e-6, msg=name)
        else:
            assert torch.equal(bb, ba), name
    assert sa.partition[1].num_batches_tracked.item() == 5
