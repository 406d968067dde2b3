"""``DeferredBatchNorm`` on the fused native Conv-BN ops (``relu_conv_bn``, the grouped op, the
``ops.fusion`` layers): every finalize route folds the micro-batch into the module's fp64
accumulator and leaves the running buffers to one commit per mini-batch.

A mini-batch of 16 images runs as 3 micro-batches (``chunk``: 6, 6, 4 -- uneven counts
exercise the Chan weights).  The oracle is fp64 eager: a training-mode batch normalisation per
micro-batch for ``y`` and the gradients, and one fp64 ``nn.BatchNorm2d`` over the concatenated
fp64 convolution outputs for the running statistics.
"""
import collections
import copy

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd.batchnorm import DeferredBatchNorm
from torchgpipe_amd.checkpoint import enable_recomputing
from torchgpipe_amd.ops import _ext, convbn, fusion
from torchgpipe_amd.ops.conv import conv_with_bn_stats

pytestmark = pytest.mark.gpu

CHUNKS = 3
BATCH = 16
# rel_err bounds: tests/ops/test_convbn_gpu.py (outputs and gradients, running statistics)
BOUND = {'y': 1e-5, 'dx': 1e-5, 'dadd': 1e-5, 'dW': 1e-5, 'dgamma': 1e-5, 'dbeta': 1e-5,
         'running_mean': 1e-6, 'running_var': 1e-6}
# (case, metric) -> allowed up to twice the error of the unfused DeferredBatchNorm path (an
# aten convolution, then the module's own native pass) on the same inputs against the same
# oracle; every entry carries both measured values
RELAXED = {
}


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()


def ops():
    return torch.ops.tgpipe


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


convert = DeferredBatchNorm.convert_deferred_batch_norm


def _init_bn(bn, seed=0):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.num_features, generator=gen) + 0.5)
        bn.bias.copy_(torch.rand(bn.num_features, generator=gen) - 0.5)
    return bn


class Case:
    """Modules with DeferredBatchNorms and how to run them: ``run(x, add)`` -> outputs (one
    per BatchNorm), ``zfn(x, weights)`` -> the BatchNorms' inputs from the convolution
    weights with plain PyTorch ops in x's precision (the oracle's and the unfused path's
    convolutions)."""

    def __init__(self, name, run, zfn, weights, bns, relu_out=False, grad_fn=None,
                 module=None):
        self.name, self.run, self.zfn, self.module = name, run, zfn, module
        self.weights, self.bns = list(weights), list(bns)
        self.relu_out, self.grad_fn = relu_out, grad_fn

    def unfused(self):
        """The same computation as an aten convolution followed by the unlinked module."""
        ws = [w.detach().clone().requires_grad_(True) for w in self.weights]
        bns = [copy.deepcopy(bn) for bn in self.bns]
        for bn in bns:
            bn.__dict__.pop('_tgpipe_relu_next', None)

        def run(x, add):
            ys = [bn(z) for bn, z in zip(bns, self.zfn(x, ws))]
            if add is not None:
                ys = [ys[0] + add]
            return [F.relu(y) for y in ys] if self.relu_out else ys

        return Case(self.name, run, self.zfn, ws, bns, self.relu_out)


def _measure(case, x, adds):
    """One mini-batch through ``case``; asserts the DeferredBatchNorm state after every
    micro-batch and returns the worst relative errors against the fp64 oracle."""
    bns, weights = case.bns, case.weights
    w64 = [w.detach().double().requires_grad_(True) for w in weights]
    gb64 = [(bn.weight.detach().double().requires_grad_(True),
             bn.bias.detach().double().requires_grad_(True)) for bn in bns]
    for p in weights + [p for bn in bns for p in (bn.weight, bn.bias)]:
        p.grad = None
    before = [(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns]
    errs = collections.defaultdict(float)
    z_all = [[] for _ in bns]
    gen = torch.Generator(device='cuda').manual_seed(99)
    for i, xi in enumerate(x.chunk(CHUNKS)):
        xi = xi.detach().clone().requires_grad_(True)
        add = adds[i].detach().clone().requires_grad_(True) if adds is not None else None
        ys = list(case.run(xi, add))
        if case.grad_fn is not None:
            for y in ys:
                assert type(y.grad_fn).__name__ == case.grad_fn + 'Backward', y.grad_fn
        x64 = xi.detach().double().requires_grad_(True)
        a64 = add.detach().double().requires_grad_(True) if add is not None else None
        y64s = []
        for k, (z, bn) in enumerate(zip(case.zfn(x64, w64), bns)):
            z_all[k].append(z.detach())
            y64 = F.batch_norm(z, None, None, gb64[k][0], gb64[k][1], True, 0.0, bn.eps)
            if a64 is not None:
                y64 = y64 + a64
            if case.relu_out:
                # the ReLU with the forward's own decisions: a value within rounding of zero
                # may fall on the other side in fp64 (tests/models/test_resnet_fused_gpu.py)
                y64 = y64 * (ys[k] > 0).double()
            y64s.append(y64)
            errs['y'] = max(errs['y'], rel_err(ys[k], y64))
        gs = [torch.randn(y.shape, device='cuda', generator=gen) for y in ys]
        torch.autograd.backward(ys, gs)
        torch.autograd.backward(y64s, [g.double() for g in gs])
        errs['dx'] = max(errs['dx'], rel_err(xi.grad, x64.grad))
        if add is not None:
            errs['dadd'] = max(errs['dadd'], rel_err(add.grad, a64.grad))
        for k, bn in enumerate(bns):
            count = z_all[k][-1].numel() // z_all[k][-1].size(1)
            if i == 0:
                assert torch.equal(bn.acc[0], torch.full_like(bn.acc[0], count)), case.name
            if i < CHUNKS - 1:
                # nothing but the accumulator moves before the mini-batch's last micro-batch
                assert torch.equal(bn.running_mean, before[k][0]), (case.name, i)
                assert torch.equal(bn.running_var, before[k][1]), (case.name, i)
                assert bn.num_batches_tracked.item() == 0 and bn.tracked == i + 1
    for k, bn in enumerate(bns):
        assert bn.num_batches_tracked.item() == 1 and bn.tracked == 0, case.name
        assert not bn.acc.any(), 'the commit zeroes the accumulator'
        ref = nn.BatchNorm2d(bn.num_features, eps=bn.eps, momentum=bn.momentum).cuda().double()
        ref.running_mean.copy_(before[k][0])
        ref.running_var.copy_(before[k][1])
        ref(torch.cat(z_all[k]))
        errs['running_mean'] = max(errs['running_mean'],
                                   rel_err(bn.running_mean, ref.running_mean))
        errs['running_var'] = max(errs['running_var'], rel_err(bn.running_var, ref.running_var))
        errs['dgamma'] = max(errs['dgamma'], rel_err(bn.weight.grad, gb64[k][0].grad))
        errs['dbeta'] = max(errs['dbeta'], rel_err(bn.bias.grad, gb64[k][1].grad))
    for w, w6 in zip(weights, w64):
        errs['dW'] = max(errs['dW'], rel_err(w.grad, w6.grad))
    return dict(errs)


def check(case, x, adds=None):
    unfused = case.unfused()  # (copied before the fused run moves the buffers)
    got = _measure(case, x, adds)
    print(f'{case.name}: ' + ' '.join(f'{m}={v:.2e}' for m, v in sorted(got.items())))
    bad = {m: v for m, v in got.items() if not v < BOUND[m]}
    if bad:
        base = _measure(unfused, x, adds)
        print(f'{case.name} unfused: ' + ' '.join(f'{m}={v:.2e}' for m, v in sorted(base.items())))
        for m, v in bad.items():
            assert (case.name, m) in RELAXED and v <= 2 * base[m], (case.name, m, v, base[m])
    return got


@pytest.fixture
def plan(request):
    """(cfg, splits) forced for every implicit-GEMM launch; -1: the tuned plans."""
    ops().conv_gemm_force_cfg(*request.param)
    try:
        yield request.param
    finally:
        ops().conv_gemm_force_cfg(-1)


def _plans(*cfgs):
    return pytest.mark.parametrize(
        'plan', cfgs, indirect=True,
        ids=['tuned' if c[0] < 0 else 'cfg%d-split%d' % (c[0], c[1] if len(c) > 1 else 1)
             for c in cfgs])


def _conv(kind, ci, co):
    if kind == '1x1':
        return nn.Conv2d(ci, co, 1, bias=False)
    return nn.Conv2d(ci, co, (1, 7), padding=(0, 3), bias=False)


def _chain_case(name, kind, ci, co, relu_in=True, relu_out=False, seed=0):
    """ReLU -> conv -> DeferredBatchNorm as a converted ``ReLUConvBN`` (``relu_out``: the
    ResNet form, conv -> BatchNorm (+ add) -> ReLU, through ``relu_conv_bn`` itself)."""
    torch.manual_seed(seed)
    conv = _conv(kind, ci, co)
    if relu_out:
        bn = _init_bn(DeferredBatchNorm(co, chunks=CHUNKS)).cuda()
        conv = conv.cuda()

        def run(x, add):
            assert convbn.fusable(x, [conv], bn)
            return [convbn.relu_conv_bn(x, [(conv, 0)], bn, relu=False, add=add, relu_out=True)]
    else:
        block = convert(convbn.ReLUConvBN(nn.ReLU(), conv, _init_bn(nn.BatchNorm2d(co))),
                        CHUNKS).cuda()
        bn = block[2]
        assert type(bn) is DeferredBatchNorm

        def run(x, add):
            return [block(x, add)]

    def zfn(x, ws):
        return [F.conv2d(F.relu(x) if relu_in and not relu_out else x, ws[0], None, 1,
                         conv.padding)]

    return Case(name, run, zfn, [conv.weight], [bn], relu_out, '_ConvBN',
                None if relu_out else block)


def _adds(shape, seed=5):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    full = torch.randn(shape, device='cuda', generator=gen)
    return list(full.chunk(CHUNKS))


def _x(*shape, seed=7):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(shape, device='cuda', generator=gen)


# -- relu_conv_bn: every finalize route of convbn_forward ---------------------------------

@_plans((-1,), (0,), (9,), (10,))
@pytest.mark.parametrize('kind', ['1x1', '1x7'])
def test_epilogue_statistics(kind, plan):
    """An unsplit GEMM's epilogue partials, finalized and applied in one launch."""
    case = _chain_case(f'epilogue-{kind}', kind, 32, 48)
    check(case, _x(BATCH, 32, 14, 14))


@_plans((9, 3), (0, 8))
@pytest.mark.parametrize('with_add', [False, True])
def test_split_small_plane(with_add, plan):
    """7x7 planes on a split-K plan: reduce + statistics + normalise in one launch."""
    case = _chain_case('split-small', '1x1', 256, 192)
    check(case, _x(BATCH, 256, 7, 7), _adds((BATCH, 192, 7, 7)) if with_add else None)


@_plans((9, 3), (0, 8))
@pytest.mark.parametrize('with_add', [False, True])
def test_split_small_plane_relu_out(with_add, plan):
    """ResNet's conv -> BatchNorm (+ identity) -> ReLU on the same route."""
    case = _chain_case('split-small-relu-out', '1x1', 256, 192, relu_out=True)
    check(case, _x(BATCH, 256, 7, 7), _adds((BATCH, 192, 7, 7)) if with_add else None)


@_plans((9, 3))
def test_split_large_plane(plan):
    """14x14 planes on a split-K plan: statistics from the split reduction, then the
    finalize + normalise launch."""
    case = _chain_case('split-large', '1x1', 256, 40)
    check(case, _x(BATCH, 256, 14, 14))


def _factorized_case():
    from torchgpipe_amd.models.amoebanet import FactorizedReduce
    torch.manual_seed(3)
    fr = FactorizedReduce(24, 40)
    _init_bn(fr.bn)
    fr = convert(fr, CHUNKS).cuda()
    assert type(fr.bn) is DeferredBatchNorm

    def zfn(x, ws):
        x = F.relu(x)
        return [torch.cat([F.conv2d(x, ws[0], None, 2),
                           F.conv2d(F.pad(x[:, :, 1:, 1:], (0, 1, 0, 1)), ws[1], None, 2)], 1)]

    return Case('factorized-reduce', lambda x, add: [fr(x)], zfn,
                [fr.conv1.weight, fr.conv2.weight], [fr.bn], False, '_ConvBN')


@_plans((-1,), (9, 3))
def test_two_convolutions_into_one_batch_norm(plan):
    """FactorizedReduce: both halves' statistics from a separate pass, one finalize."""
    check(_factorized_case(), _x(BATCH, 24, 15, 15))


# -- the grouped op: one accumulator per operation ----------------------------------------

GROUP_CHANNELS = (24, 40, 56)


def _group_case(middle_seed):
    torch.manual_seed(4)
    blocks = [convert(convbn.ReLUConvBN(nn.ReLU(), nn.Conv2d(40, co, 1, bias=False),
                                        _init_bn(nn.BatchNorm2d(co), seed=10 + k)), CHUNKS).cuda()
              for k, co in enumerate(GROUP_CHANNELS)]
    _init_bn(blocks[1][2], seed=middle_seed)
    triplets = [b._triplets()[0] for b in blocks]
    cache = convbn._GroupCache()

    def run(x, add):
        assert convbn.groupable(x, triplets)
        return list(convbn.group_relu_conv_bn(x, triplets, cache))

    def zfn(x, ws):
        return [F.conv2d(F.relu(x), w) for w in ws]

    return Case('grouped', run, zfn, [b[1].weight for b in blocks], [b[2] for b in blocks],
                False, '_GroupConvBN', triplets)


@pytest.mark.parametrize('middle_seed', [11, 77], ids=['', 'other-middle'])
@pytest.mark.parametrize('hw, plan', [(14, (-1,)), (7, (9, 3))], indirect=['plan'],
                         ids=['14x14-tuned', '7x7-split3'])
def test_grouped_operations_fold_into_their_own_accumulators(hw, plan, middle_seed):
    """Three ReLU -> 1x1 -> DeferredBatchNorm operations of one input with 24 / 40 / 56
    output channels (no multiples of 8, unequal: a part-offset or part-stride mistake moves
    another operation's statistics); each operation's accumulator and running statistics are
    checked on their own (``_measure``)."""
    check(_group_case(middle_seed), _x(BATCH, 40, hw, hw))


def test_groupable_mixes_neither_kinds_nor_chunks():
    case = _group_case(11)
    x = _x(6, 40, 14, 14)
    blocks = list(case.module)  # (the triplets)
    assert convbn.groupable(x, blocks)
    plain = (True, blocks[0][1], nn.BatchNorm2d(24).cuda())
    assert not convbn.groupable(x, [plain] + blocks[1:])
    assert not convbn.groupable(x, blocks[:2] + [plain])
    other = (True, blocks[0][1], DeferredBatchNorm(24, chunks=CHUNKS + 1).cuda())
    assert not convbn.groupable(x, [other] + blocks[1:])


# -- ops.fusion layers ---------------------------------------------------------------------

# (name, ci, hw, co, kernel, stride, padding, the function whose backward the output carries)
LAYERS = [
    ('1x1', 64, 28, 96, 1, 1, 0, '_ConvBN'),
    # the two Winograd routes of tests/models/test_resnet_fused_gpu.py: the fused F(4x4) and
    # the batched GEMM, whose output pass leaves the statistics partials
    ('3x3-f4', 64, 28, 64, 3, 1, 1, '_BNAct'),
    ('3x3-batched-gemm', 256, 14, 256, 3, 1, 1, '_BNAct'),
    ('3x3s2-strided-fused', 512, 14, 512, 3, 2, 1, '_ConvBN'),  # a STRIDED_FUSED member
    ('3x3s2-miopen', 32, 28, 32, 3, 2, 1, '_BNAct'),
]


def _layer_case(name, ci, co, k, stride, pad, grad_fn, relu=True):
    torch.manual_seed(6)
    mods = [fusion.ConvBN2d(ci, co, k, stride=stride, padding=pad, bias=False),
            _init_bn(DeferredBatchNorm(co, chunks=CHUNKS))]
    if relu:
        mods.append(fusion.ReLU())
    seq = nn.Sequential(*mods).cuda()
    assert fusion.relink(seq) == 1

    def run(x, add):
        if name in ('3x3-f4', '3x3-batched-gemm'):
            # which Winograd route this input takes: the batched GEMM's output pass leaves
            # the statistics partials, the fused F(4x4) kernel leaves none
            with torch.no_grad():
                stats = conv_with_bn_stats(seq[0], x)
            assert (stats is not None) == (name == '3x3-batched-gemm'), name
            if stats is not None:
                assert stats[1] is not None and stats[2] > 0
        y = seq(x)
        assert getattr(y, '_tgpipe_bn_done', None) == id(seq[1]), 'the fused path must run'
        return [y]

    def zfn(x, ws):
        return [F.conv2d(x, ws[0], None, stride, pad)]

    return Case(f'layer-{name}', run, zfn, [seq[0].weight], [seq[1]], relu, grad_fn, seq)


@pytest.mark.parametrize('layer', LAYERS, ids=[c[0] for c in LAYERS])
def test_linked_layers(layer):
    name, ci, hw, co, k, stride, pad, grad_fn = layer
    if name == '3x3s2-strided-fused':
        assert (ci, co, (k, k), (stride, stride), (pad, pad), hw) in fusion.STRIDED_FUSED
    case = _layer_case(name, ci, co, k, stride, pad, grad_fn)
    # The layers read rectified activations, as each of them does in ResNet (its previous
    # block's ReLU).  A zero-mean input gives every output channel a mean far below its
    # standard deviation, and the relative error of running_mean then shows the
    # convolution's rounding amplified by std / |mean| rather than the fold: measured with
    # plain randn inputs, 1.07e-06 (F(4x4)), 7.87e-06 (batched GEMM) and 1.86e-06 (strided
    # fused) against 2.24e-07 / 3.81e-07 / 4.88e-07 for an aten convolution, every other
    # figure within its bound (tests/models/test_resnet_fused_gpu.py allows the plain
    # BatchNorm 2e-5 there for the same reason).
    check(case, _x(BATCH, ci, hw, hw).relu())


def test_deferred_batch_norm_applies_its_linked_relu():
    """``DeferredBatchNorm -> ReLU`` without a convolution before it: one native pass."""
    torch.manual_seed(8)
    seq = nn.Sequential(_init_bn(DeferredBatchNorm(24, chunks=CHUNKS)), fusion.ReLU()).cuda()
    fusion.relink(seq)

    def run(x, add):
        y = seq(x)
        assert getattr(y, '_tgpipe_relu_done', False)
        return [y]

    check(Case('bn-relu', run, lambda x, ws: [x], [], [seq[0]], True, '_BNTrain'),
          _x(BATCH, 24, 9, 9))


# -- recomputation -------------------------------------------------------------------------

def _recompute_cases():
    yield 'epilogue', lambda: _chain_case('epilogue', '1x1', 32, 48), (6, 32, 14, 14), (-1,)
    yield 'split-small', lambda: _chain_case('split', '1x1', 256, 192), (6, 256, 7, 7), (9, 3)
    yield 'grouped', lambda: _group_case(11), (6, 40, 14, 14), (-1,)
    yield 'grouped-split', lambda: _group_case(11), (6, 40, 7, 7), (9, 3)
    yield 'winograd', lambda: _layer_case('3x3', 64, 64, 3, 1, 1, '_BNAct'), \
        (6, 64, 28, 28), (-1,)


@pytest.mark.parametrize('name, make, shape, plan', list(_recompute_cases()), indirect=['plan'],
                         ids=[c[0] for c in _recompute_cases()])
def test_recomputation_tracks_nothing(name, make, shape, plan):
    case = make()
    x = _x(*shape).requires_grad_(True)
    first = [y.detach().clone() for y in case.run(x, None)]
    state = [(bn.acc.clone(), bn.tracked, bn.counter, bn.running_mean.clone(),
              bn.running_var.clone(), bn.num_batches_tracked.clone()) for bn in case.bns]
    assert all(bn.tracked == 1 and bn.acc[0].ne(0).all() for bn in case.bns)
    with enable_recomputing():
        again = list(case.run(x, None))
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for bn, (acc, tracked, counter, rm, rv, nbt) in zip(case.bns, state):
        assert torch.equal(bn.acc, acc) and bn.tracked == tracked and bn.counter == counter
        assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
        assert torch.equal(bn.num_batches_tracked, nbt)


# -- evaluation ----------------------------------------------------------------------------

def _count(monkeypatch):
    calls = collections.Counter()
    for mod, name in ((convbn, 'conv_bn_eval'), (fusion, 'bn_eval_act')):
        def wrapped(*args, _f=getattr(mod, name), _n=name, **kwargs):
            calls[_n] += 1
            return _f(*args, **kwargs)
        monkeypatch.setattr(mod, name, wrapped)
    return calls


def _eval_cases():
    yield 'chain', lambda: _chain_case('chain', '1x7', 32, 48), (4, 32, 14, 14), 'conv_bn_eval'
    yield 'layer-1x1', lambda: _layer_case('1x1', 64, 96, 1, 1, 0, '_ConvBN'), \
        (4, 64, 28, 28), 'conv_bn_eval'
    yield 'layer-3x3', lambda: _layer_case('3x3', 64, 64, 3, 1, 1, '_BNAct'), \
        (4, 64, 28, 28), 'bn_eval_act'


@pytest.mark.parametrize('name, make, shape, called', list(_eval_cases()),
                         ids=[c[0] for c in _eval_cases()])
def test_eval_after_a_mini_batch_takes_the_native_eval_ops(name, make, shape, called,
                                                           monkeypatch):
    case = make()
    bn = case.bns[0]
    for xi in _x(BATCH, *shape[1:]).chunk(CHUNKS):  # one committed mini-batch
        case.run(xi, None)
    assert bn.num_batches_tracked.item() == 1
    bn.eval()
    buffers = (bn.running_mean.clone(), bn.running_var.clone())
    x = _x(*shape, seed=12)
    calls = _count(monkeypatch)
    with torch.no_grad():
        y = case.module(x)
    assert calls[called] == 1 and sum(calls.values()) == 1, calls
    z = case.zfn(x.double(), [w.detach().double() for w in case.weights])[0]
    want = F.batch_norm(z, bn.running_mean.double(), bn.running_var.double(),
                        bn.weight.double(), bn.bias.double(), False, 0.0, bn.eps)
    if case.relu_out:
        want = F.relu(want)
    assert rel_err(y, want) < 1e-5
    assert torch.equal(bn.running_mean, buffers[0]) and torch.equal(bn.running_var, buffers[1])
    assert bn.num_batches_tracked.item() == 1 and not bn.acc.any()
    # gradients enabled and required: the eval ops are forward-only, the layers fall back
    calls.clear()
    xg = x.clone().requires_grad_(True)
    y = case.module(xg)
    assert sum(calls.values()) == 0 and y.requires_grad
    assert rel_err(y, want) < 1e-5
    y.sum().backward()
    assert xg.grad is not None and case.weights[0].grad is not None
    assert torch.equal(bn.running_mean, buffers[0])
