"""``DeferredBatchNorm`` wherever the fused Conv-BN ops and layer links take a ``BatchNorm2d``
(CPU checks): the links ``relink`` makes survive the conversion, the chain predicates accept
the converted BatchNorms, converted modules compute what the plain modules compute, and the
bookkeeping interface the fused callers use commits once per mini-batch."""
import copy
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

from torchgpipe_amd.batchnorm import DeferredBatchNorm
from torchgpipe_amd.checkpoint import enable_recomputing
from torchgpipe_amd.models.resnet import build_resnet
from torchgpipe_amd.ops import convbn, fusion

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
convert = DeferredBatchNorm.convert_deferred_batch_norm


def _tiny_resnet():
    torch.manual_seed(0)
    return build_resnet([1, 1, 1, 1], num_classes=10, fused=True)


def test_relink_links_as_many_convolutions_after_conversion():
    model = _tiny_resnet()
    before = fusion.relink(model)
    assert before > 0
    model = convert(model, chunks=3)
    assert not any(type(m) is fusion.BatchNormAct2d for m in model.modules())
    assert fusion.relink(model) == before


def test_relink_keeps_the_join_and_relu_marks_after_conversion():
    plain = _tiny_resnet()
    fusion.relink(plain)
    model = convert(copy.deepcopy(plain), chunks=3)
    fusion.relink(model)

    def marks(m):
        joins = relus = bn_relus = 0
        for mod in m.modules():
            link = mod.__dict__.get('_tgpipe_link')
            if link is not None:
                joins += link[2] is not None
                relus += bool(link[1])
            if isinstance(mod, nn.modules.batchnorm._BatchNorm):
                bn_relus += bool(mod.__dict__.get('_tgpipe_relu_next', False))
        return joins, relus, bn_relus

    want = marks(plain)
    assert want[0] == 4 and want[1] > 0 and want[2] > 0  # one residual join per block
    assert marks(model) == want
    for mod in model.modules():
        link = mod.__dict__.get('_tgpipe_link')
        if link is not None:
            assert type(link[0]) is DeferredBatchNorm


def test_relink_links_a_deferred_batch_norm_to_its_relu():
    seq = nn.Sequential(DeferredBatchNorm(4, chunks=2), fusion.ReLU())
    fusion.relink(seq)
    assert seq[0].__dict__.get('_tgpipe_relu_next') is True
    seq = nn.Sequential(fusion.ConvBN2d(3, 4, 1, bias=False), DeferredBatchNorm(4, chunks=2),
                        fusion.ReLU())
    assert fusion.relink(seq) == 1
    assert seq[0].__dict__['_tgpipe_link'] == (seq[1], True, None)


def test_fused_triplets_accepts_a_converted_chain():
    chain = convbn.ReLUConvBN(nn.ReLU(), nn.Conv2d(4, 6, 1, bias=False), nn.BatchNorm2d(6))
    assert convbn.fused_triplets(chain) is not None
    chain = convert(chain, chunks=3)
    trip = convbn.fused_triplets(chain)
    assert trip is not None and len(trip) == 1
    assert trip[0][0] is True and type(trip[0][2]) is DeferredBatchNorm
    assert chain._triplets() is not None


def test_predicates_take_only_training_gpu_inputs_on_the_cpu():
    """CPU tensors keep the eager path, for a DeferredBatchNorm as for a BatchNorm2d."""
    bn = DeferredBatchNorm(6, chunks=3)
    conv = nn.Conv2d(4, 6, 1, bias=False)
    x = torch.randn(2, 4, 5, 5)
    assert not convbn.fusable(x, [conv], bn)
    assert not convbn.eval_fusable(x, [conv], bn.eval())
    assert not convbn.groupable(x, [(True, conv, bn), (True, conv, bn)])


def _running_stats_by_hand(inputs, momentum=0.1):
    """One mini-batch's running statistics from a BatchNorm's micro-batch inputs, in fp64:
    the mean and the unbiased variance over all of them, folded into buffers of (0, 1)."""
    z = torch.cat([t.double() for t in inputs])
    dims = [0] + list(range(2, z.dim()))
    mean, var = z.mean(dims), z.var(dims, unbiased=True)
    return momentum * mean, (1 - momentum) + momentum * var


def _check_against_plain(plain, x, chunks=3):
    """``convert(plain)`` normalises every micro-batch as ``plain`` does in training mode and
    commits, once, the statistics of the whole mini-batch."""
    model = convert(copy.deepcopy(plain), chunks=chunks)
    fusion.relink(model)
    fusion.relink(plain)
    seen = {}
    for name, m in plain.named_modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.register_forward_hook(
                lambda mod, args, out, name=name: seen.setdefault(name, []).append(
                    args[0].detach()))
    for xi in x.chunk(chunks):
        got, want = model(xi), plain(xi)
        assert torch.equal(got, want)
    dbns = {n: m for n, m in model.named_modules() if isinstance(m, DeferredBatchNorm)}
    assert dbns and set(dbns) == set(seen)
    for name, bn in dbns.items():
        assert len(seen[name]) == chunks
        mean, var = _running_stats_by_hand(seen[name])
        torch.testing.assert_close(bn.running_mean.double(), mean, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(bn.running_var.double(), var, rtol=1e-5, atol=1e-7)
        assert bn.num_batches_tracked.item() == 1
        assert bn.tracked == 0 and bn.counter == 0 and not bn.acc.any()


def test_converted_chain_matches_the_plain_chain_on_the_cpu():
    torch.manual_seed(1)
    chain = convbn.FusedChain(nn.ReLU(), nn.Conv2d(4, 6, (1, 7), padding=(0, 3), bias=False),
                              nn.BatchNorm2d(6), nn.ReLU(), nn.Conv2d(6, 5, 1, bias=False),
                              nn.BatchNorm2d(5))
    _check_against_plain(chain, torch.randn(8, 4, 9, 9))


def test_converted_resnet_matches_the_plain_resnet_on_the_cpu():
    _check_against_plain(_tiny_resnet(), torch.randn(6, 3, 32, 32))


def test_fold_interface_commits_once_per_mini_batch():
    bn = DeferredBatchNorm(3, chunks=2)
    x = torch.randn(4, 3, 5, 5)
    for k in range(2):
        acc = bn.fold_acc()
        assert acc is bn.acc
        # (what a fused op does: fold the micro-batch, then the bookkeeping call)
        from torchgpipe_amd.batchnorm import _chan_merge_
        _chan_merge_(acc, x)
        bn.fold_done(x.numel() // x.size(1))
        if k == 0:
            assert bn.tracked == 1 and bn.counter == 100
            assert bn.num_batches_tracked.item() == 0 and bn.acc[0].eq(100).all()
    assert bn.num_batches_tracked.item() == 1
    assert bn.tracked == 0 and bn.counter == 0 and not bn.acc.any()
    mean, var = _running_stats_by_hand([x, x])
    torch.testing.assert_close(bn.running_mean.double(), mean, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(bn.running_var.double(), var, rtol=1e-5, atol=1e-7)


def test_fold_interface_follows_expected_chunks_and_skips_recomputation():
    bn = DeferredBatchNorm(3, chunks=4)
    bn.expected_chunks = 1
    with enable_recomputing():
        assert bn.fold_acc() is None
        bn.fold_done(100)
    assert bn.tracked == 0 and bn.counter == 0 and bn.num_batches_tracked.item() == 0
    x = torch.randn(4, 3, 5, 5)
    before = bn.running_mean.clone()
    with enable_recomputing():
        bn(x)  # forward goes through the same two calls
    assert bn.tracked == 0 and not bn.acc.any() and torch.equal(bn.running_mean, before)
    bn(x)
    assert bn.num_batches_tracked.item() == 1 and bn.tracked == 0


def test_forward_passes_an_input_its_linked_convolution_normalised():
    bn = DeferredBatchNorm(3, chunks=1)
    x = torch.randn(2, 3, 4, 4)
    setattr(x, '_tgpipe_bn_done', id(bn))
    assert bn(x) is x
    assert bn.num_batches_tracked.item() == 0 and bn.tracked == 0
    other = DeferredBatchNorm(3, chunks=1)
    assert other(x) is not x


def test_schemas_keep_the_calls_without_the_new_arguments():
    """``acc`` / ``accs`` are trailing and default to absent (checked in a child process: a
    bad schema aborts at import)."""
    if not any(f.startswith('_C') and f.endswith('.so')
               for f in os.listdir(os.path.join(ROOT, 'torchgpipe_amd'))):
        pytest.fail('extension not built (python -m torchgpipe_amd._build): the schemas '
                    'cannot be checked')
    code = ('import torch, torchgpipe_amd._C; ops = torch.ops.tgpipe\n'
            'for op, name in ((ops.convbn_forward, "acc"), (ops.convbn_group_forward, "accs")):\n'
            '    args = op.default._schema.arguments\n'
            '    print(args[-1].name == name, args[-1].has_default_value(), '
            'args[-1].default_value is None)\n')
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-6:] == ['True'] * 6, out.stdout
