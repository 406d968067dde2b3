"""The eval-mode Conv-BN path's conditions (``ops.convbn.eval_fusable``) and its CPU
fall-backs; no GPU needed."""
import copy
import os

import pytest
import torch
from torch import nn

from torchgpipe_amd.ops import convbn, fusion

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _triplet(**conv_kwargs):
    conv_kwargs.setdefault('bias', False)
    return nn.Conv2d(8, 12, 1, **conv_kwargs), nn.BatchNorm2d(12).eval()


def test_eval_fusable_is_false_off_the_native_path():
    x = torch.randn(2, 8, 6, 6)
    conv, bn = _triplet()
    with torch.no_grad():
        assert not convbn.eval_fusable(x, [conv], bn)                         # CPU tensors
        assert not convbn.eval_fusable(x.double(), [copy.deepcopy(conv).double()],
                                       copy.deepcopy(bn).double())            # fp64
    if not torch.cuda.is_available():
        return
    x = x.cuda()
    with torch.no_grad():
        conv, bn = conv.cuda(), bn.cuda()
        assert not convbn.eval_fusable(x.double(), [copy.deepcopy(conv).double()],
                                       copy.deepcopy(bn).double())
        biased, _ = _triplet(bias=True)
        assert not convbn.eval_fusable(x, [biased.cuda()], bn)
        grouped, _ = _triplet(groups=2)
        assert not convbn.eval_fusable(x, [grouped.cuda()], bn)
        assert not convbn.eval_fusable(x, [conv], copy.deepcopy(bn).train())
        no_stats = nn.BatchNorm2d(12, track_running_stats=False).cuda().eval()
        assert not convbn.eval_fusable(x, [conv], no_stats)
    # gradients enabled: the weights (and x) require them
    assert not convbn.eval_fusable(x, [conv], bn)
    assert not convbn.eval_fusable(x.clone().requires_grad_(True),
                                   [copy.deepcopy(conv).requires_grad_(False)],
                                   copy.deepcopy(bn).requires_grad_(False))


def test_fused_chain_in_eval_on_cpu_equals_the_plain_modules():
    torch.manual_seed(0)
    chain = convbn.FusedChain(nn.ReLU(), nn.Conv2d(8, 12, 1, bias=False), nn.BatchNorm2d(12),
                              nn.ReLU(), nn.Conv2d(12, 8, (1, 7), padding=(0, 3), bias=False),
                              nn.BatchNorm2d(8))
    with torch.no_grad():
        for m in chain:
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.5)
                m.running_var.uniform_(0.5, 2)
    chain.eval()
    plain = nn.Sequential(*copy.deepcopy(chain).children()).eval()
    x = torch.randn(2, 8, 6, 6)
    add = torch.randn(2, 8, 6, 6)
    with torch.no_grad():
        assert torch.equal(chain(x), plain(x))
        assert torch.equal(chain(x, add), plain(x) + add)


def test_convbn2d_in_eval_on_cpu_equals_the_plain_modules():
    torch.manual_seed(0)
    seq = nn.Sequential(fusion.ConvBN2d(8, 12, 3, padding=1, bias=False),
                        fusion.BatchNormAct2d(12), fusion.ReLU())
    with torch.no_grad():
        seq[1].running_mean.normal_(0, 0.5)
        seq[1].running_var.uniform_(0.5, 2)
    assert fusion.relink(seq) == 1
    plain = nn.Sequential(nn.Conv2d(8, 12, 3, padding=1, bias=False), nn.BatchNorm2d(12),
                          nn.ReLU())
    plain.load_state_dict(seq.state_dict())
    seq.eval()
    plain.eval()
    x = torch.randn(2, 8, 6, 6)
    with torch.no_grad():
        assert torch.equal(seq(x), plain(x))


def test_eval_ops_are_registered():
    if not any(f.startswith('_C') and f.endswith('.so')
               for f in os.listdir(os.path.join(ROOT, 'torchgpipe_amd'))):
        pytest.skip('extension not built (python -m torchgpipe_amd._build)')
    import torchgpipe_amd._C  # noqa: F401
    schemas = {name: str(getattr(torch.ops.tgpipe, name).default._schema)
               for name in ('convbn_eval_forward', 'bn_eval_act')}
    assert 'Tensor? gamma, Tensor? beta, Tensor running_mean, Tensor running_var, float eps, ' \
           'Tensor? add, bool relu_out' in schemas['convbn_eval_forward']
    assert schemas['convbn_eval_forward'].endswith('-> Tensor')
    assert 'Tensor? add, bool relu, bool inplace' in schemas['bn_eval_act']
    assert schemas['bn_eval_act'].endswith('-> Tensor')
