"""Eval-mode Conv-BN(-ReLU)(+add) on the native forward-only ops (``convbn_eval_forward``:
the BatchNorm folded into the implicit GEMM's store loop or its split reduction;
``bn_eval_act``: the stand-alone pass) against fp64 eager references of the same layers."""
import copy
import itertools

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd.ops import _ext, convbn, fusion

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()


def ops():
    return torch.ops.tgpipe


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _eval_bn(c, affine=True, track=True):
    """gamma ~ U(0.5, 1.5), beta ~ U(-0.5, 0.5), running_mean ~ N(0, 0.5), running_var ~
    U(0.5, 2), in eval mode."""
    bn = nn.BatchNorm2d(c, affine=affine, track_running_stats=track).cuda()
    with torch.no_grad():
        if affine:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        if track:
            bn.running_mean.normal_(0, 0.5)
            bn.running_var.uniform_(0.5, 2)
    return bn.eval()


def _fp64(x, convs, bn, relu, add, relu_out):
    """bn(cat(conv_i(relu?(x) shifted by offset_i))) (+ add) (ReLU) in fp64, eagerly."""
    with torch.no_grad():
        x = x.double()
        x = F.relu(x) if relu else x
        outs = []
        for conv, offset in convs:
            xi = F.pad(x[:, :, offset:, offset:], (0, offset, 0, offset)) if offset else x
            outs.append(copy.deepcopy(conv).double()(xi))
        y = copy.deepcopy(bn).double()(torch.cat(outs, dim=1))
        if add is not None:
            y = y + add.double()
        return F.relu(y) if relu_out else y


# (n, ci, h, w, co, kernel, stride, padding): the smallest shapes reaching each store path
CASES = [
    (4, 32, 28, 28, 48, (1, 1), 1, (0, 0)),    # quad stores, row tail below 64
    (5, 24, 7, 7, 40, (1, 1), 1, (0, 0)),      # scalar stores, quads spanning images
    (3, 16, 14, 14, 20, (1, 7), 1, (0, 3)),    # gathered operand
    (4, 64, 28, 28, 128, (1, 1), 2, (0, 0)),   # strided
    (2, 3, 32, 32, 64, (7, 7), 2, (3, 3)),     # the stem
]
CASE_IDS = ['1x1_quad', '1x1_7x7plane', '1x7', '1x1s2', 'stem7x7s2']
_INPUTS = {}  # case index -> (x, conv, bn, add), built once
_WANT = {}    # (case index, relu, with_add, relu_out) -> fp64 reference, computed once


@pytest.fixture(scope='module', autouse=True)
def release_shared_tensors():
    yield
    for cache in (_INPUTS, _WANT, _SPLIT_INPUTS):
        cache.clear()


def _inputs(k):
    if k not in _INPUTS:
        n, ci, h, w, co, kernel, stride, pad = CASES[k]
        torch.manual_seed(10 + k)
        conv = nn.Conv2d(ci, co, kernel, stride=stride, padding=pad, bias=False).cuda()
        bn = _eval_bn(co)
        x = torch.randn(n, ci, h, w, device='cuda')
        with torch.no_grad():
            add = torch.randn_like(conv(x))
        _INPUTS[k] = (x, conv, bn, add)
    return _INPUTS[k]


def _want(k, relu, with_add, relu_out):
    key = (k, relu, with_add, relu_out)
    if key not in _WANT:
        x, conv, bn, add = _inputs(k)
        _WANT[key] = _fp64(x, [(conv, 0)], bn, relu, add if with_add else None, relu_out)
    return _WANT[key]


@pytest.fixture(params=[-1, 0, 1, 9, 10, 11],
                ids=['tuned', 'cfg0', 'cfg1', 'cfg9', 'cfg10', 'cfg11'])
def tile_cfg(request):
    """f32 64 x 64 and 128 x 128 tiles, the split-bf16 128 x 128 and the two single-buffered
    configurations, then the tuned plans."""
    ops().conv_gemm_force_cfg(request.param)
    yield request.param
    ops().conv_gemm_force_cfg(-1)


@pytest.mark.parametrize('relu_out', [False, True])
@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('k', range(len(CASES)), ids=CASE_IDS)
def test_conv_bn_eval_matches_fp64(k, relu, with_add, relu_out, tile_cfg):
    x, conv, bn, add = _inputs(k)
    want = _want(k, relu, with_add, relu_out)
    with torch.no_grad():
        assert convbn.eval_fusable(x, [conv], bn, add if with_add else None)
        got = convbn.conv_bn_eval(x, [(conv, 0)], bn, relu=relu, add=add if with_add else None,
                                  relu_out=relu_out)
    assert got.shape == want.shape
    err = rel_err(got, want)
    print(f'{CASE_IDS[k]} relu={relu} add={with_add} relu_out={relu_out} cfg={tile_cfg}: '
          f'{err:.2e}')
    assert err < 1e-5


@pytest.mark.parametrize('relu_out', [False, True])
@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('relu', [False, True])
def test_factorized_reduce_eval_matches_eager_fp64(relu, with_add, relu_out, tile_cfg):
    """Two strided 1x1 convolutions concatenated on channels, the second reading the input
    shifted by one pixel, on an odd plane: scale / shift / add indexed through co_off.  The
    module's own expression (ReLU in, no ReLU out) runs through the module, against the
    module under ``disabled()`` in fp64; the other crossings through the op."""
    from torchgpipe_amd.models.amoebanet import FactorizedReduce
    torch.manual_seed(3)
    fr = FactorizedReduce(24, 32).cuda()
    with torch.no_grad():
        fr.bn.weight.uniform_(0.5, 1.5)
        fr.bn.bias.uniform_(-0.5, 0.5)
        fr.bn.running_mean.normal_(0, 0.5)
        fr.bn.running_var.uniform_(0.5, 2)
    fr.eval()
    x = torch.randn(4, 24, 15, 15, device='cuda')
    add = torch.randn(4, 32, 8, 8, device='cuda') if with_add else None
    parts = [(fr.conv1, 0), (fr.conv2, 1)]
    with torch.no_grad():
        assert convbn.eval_fusable(x, [fr.conv1, fr.conv2], fr.bn, add)
        if relu and not relu_out:
            y = fr(x, add)
            with convbn.disabled():
                y64 = copy.deepcopy(fr).double()(x.double(),
                                                 None if add is None else add.double())
        else:
            y = convbn.conv_bn_eval(x, parts, fr.bn, relu=relu, add=add, relu_out=relu_out)
            y64 = _fp64(x, parts, fr.bn, relu, add, relu_out)
    assert rel_err(y, y64) < 1e-5


# forced (cfg, splits) x shapes whose reduction the forced plans split
SPLITS = [(7, 4), (10, 3), (0, 8)]
SPLIT_SHAPES = [(12, 128, 7, 7, 96),   # odd plane: scalar reduce
                (20, 256, 8, 8, 64),   # 8^2 plane: vector reduce
                (20, 384, 5, 5, 48)]
_SPLIT_INPUTS = {}


def _split_inputs(k):
    if k not in _SPLIT_INPUTS:
        n, ci, h, w, co = SPLIT_SHAPES[k]
        torch.manual_seed(20 + k)
        conv = nn.Conv2d(ci, co, 1, bias=False).cuda()
        bn = _eval_bn(co)
        x = torch.randn(n, ci, h, w, device='cuda')
        add = torch.randn(n, co, h, w, device='cuda')
        want = {(a, r): _fp64(x, [(conv, 0)], bn, True, add if a else None, r)
                for a, r in itertools.product([False, True], repeat=2)}
        _SPLIT_INPUTS[k] = (x, conv, bn, add, want)
    return _SPLIT_INPUTS[k]


@pytest.mark.parametrize('relu_out', [False, True])
@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('k', range(len(SPLIT_SHAPES)), ids=['7x7', '8x8', '5x5'])
@pytest.mark.parametrize('split_cfg', SPLITS, ids=[f'cfg{c}x{s}' for c, s in SPLITS])
def test_split_k_eval_applies_the_tail_in_the_reduction(split_cfg, k, with_add, relu_out):
    x, conv, bn, add, want = _split_inputs(k)
    ops().conv_gemm_force_cfg(*split_cfg)
    try:
        with torch.no_grad():
            got = convbn.conv_bn_eval(x, [(conv, 0)], bn, relu=True,
                                      add=add if with_add else None, relu_out=relu_out)
    finally:
        ops().conv_gemm_force_cfg(-1)
    assert rel_err(got, want[(with_add, relu_out)]) < 1e-5


def test_running_buffers_are_left_untouched():
    x, conv, bn, add = _inputs(0)
    before = [b.clone() for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    with torch.no_grad():
        convbn.conv_bn_eval(x, [(conv, 0)], bn, add=add, relu_out=True)
        fusion.bn_eval_act(add, bn, True)
    torch.cuda.synchronize()
    for b, was in zip((bn.running_mean, bn.running_var, bn.num_batches_tracked), before):
        assert torch.equal(b, was)


def test_affine_less_batchnorm_matches_fp64():
    x, conv, _, add = _inputs(1)
    torch.manual_seed(5)
    bn = _eval_bn(conv.out_channels, affine=False)
    with torch.no_grad():
        assert convbn.eval_fusable(x, [conv], bn)
        got = convbn.conv_bn_eval(x, [(conv, 0)], bn, add=add)
        act = fusion.bn_eval_act(add, bn, True)
    assert rel_err(got, _fp64(x, [(conv, 0)], bn, True, add, False)) < 1e-5
    with torch.no_grad():
        assert rel_err(act, F.relu(copy.deepcopy(bn).double()(add.double()))) < 1e-5


def test_two_calls_are_bitwise_equal(tile_cfg):
    x, conv, bn, add = _inputs(0)
    with torch.no_grad():
        a = convbn.conv_bn_eval(x, [(conv, 0)], bn, add=add, relu_out=True)
        b = convbn.conv_bn_eval(x, [(conv, 0)], bn, add=add, relu_out=True)
    assert torch.equal(a, b)


def test_captured_call_replays_bitwise():
    """One call captured on a side stream (after a warm-up call there, so the plan and the
    pre-split weights exist before the capture) and replayed twice equals the eager call.
    The side stream is ``torch.cuda.graph``'s own capture stream, which the process has
    anyway: a stream made here would move every later test's streams one place along the
    round-robin stream pool, and with that onto other hardware queues."""
    x, conv, bn, add = _inputs(0)
    with torch.no_grad():
        want = convbn.conv_bn_eval(x, [(conv, 0)], bn, add=add, relu_out=True)
        graph = torch.cuda.CUDAGraph()
        capture = torch.cuda.graph(graph)
        side = capture.capture_stream
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            convbn.conv_bn_eval(x, [(conv, 0)], bn, add=add, relu_out=True)
        torch.cuda.current_stream().wait_stream(side)
        with capture:
            out = convbn.conv_bn_eval(x, [(conv, 0)], bn, add=add, relu_out=True)
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('shape', [(3, 20, 7, 7), (2, 64, 16, 16)], ids=['scalar', 'vector'])
def test_bn_eval_act_matches_fp64(shape, with_add, relu):
    torch.manual_seed(6)
    bn = _eval_bn(shape[1])
    x = torch.randn(*shape, device='cuda')
    add = torch.randn(*shape, device='cuda') if with_add else None
    with torch.no_grad():
        want = copy.deepcopy(bn).double()(x.double())
        if add is not None:
            want = want + add.double()
        want = F.relu(want) if relu else want
        got = fusion.bn_eval_act(x, bn, relu, add)
        assert got.data_ptr() != x.data_ptr()
        assert rel_err(got, want) < 1e-5
        ptr = x.data_ptr()
        same = fusion.bn_eval_act(x, bn, relu, add, inplace=True)
        assert same.data_ptr() == ptr and same.untyped_storage().data_ptr() == \
            x.untyped_storage().data_ptr()
        assert torch.equal(same, got)


def test_bn_eval_act_robust_to_large_mean():
    """running_mean 1e3, running_var 1e-2, x = 1e3 + 0.1 N(0, 1): (x - mean) * k, not
    x * k - mean * k -- the looseness test_batchnorm_statistics_robust_to_large_mean grants
    the same cancellation."""
    torch.manual_seed(7)
    bn = _eval_bn(64)
    with torch.no_grad():
        bn.running_mean.fill_(1e3)
        bn.running_var.fill_(1e-2)
        x = 1e3 + 0.1 * torch.randn(2, 64, 16, 16, device='cuda')
        want = copy.deepcopy(bn).double()(x.double())
        got = fusion.bn_eval_act(x, bn, False)
    assert rel_err(got, want) < 1e-4


def _chain(track=True):
    torch.manual_seed(8)
    chain = convbn.ReLUConvBN(nn.ReLU(), nn.Conv2d(32, 48, 1, bias=False),
                              nn.BatchNorm2d(48, track_running_stats=track)).cuda()
    with torch.no_grad():
        chain[2].weight.uniform_(0.5, 1.5)
        chain[2].bias.uniform_(-0.5, 0.5)
        if track:
            chain[2].running_mean.normal_(0, 0.5)
            chain[2].running_var.uniform_(0.5, 2)
    return chain.eval()


def test_eval_with_gradients_falls_back_and_backpropagates():
    chain = _chain()
    ref = copy.deepcopy(chain).double()
    x = torch.randn(4, 32, 14, 14, device='cuda', requires_grad=True)
    assert not convbn.eval_fusable(x, [chain[1]], chain[2])
    y = chain(x)
    y.square().sum().backward()
    assert x.grad is not None
    x64 = x.detach().double().requires_grad_(True)
    with convbn.disabled():
        y64 = ref(x64)
    y64.square().sum().backward()
    assert rel_err(y, y64) < 1e-5
    assert rel_err(x.grad, x64.grad) < 1e-5


def test_eval_without_running_statistics_falls_back():
    chain = _chain(track=False)
    ref = copy.deepcopy(chain).double()
    x = torch.randn(4, 32, 14, 14, device='cuda')
    with torch.no_grad():
        assert not convbn.eval_fusable(x, [chain[1]], chain[2])
        y = chain(x)
        with convbn.disabled():
            y64 = ref(x.double())
    assert rel_err(y, y64) < 1e-5


def test_disabled_runs_the_eager_modules():
    chain = _chain()
    ref = copy.deepcopy(chain).double()
    x = torch.randn(4, 32, 14, 14, device='cuda')
    with torch.no_grad(), convbn.disabled():
        assert not convbn.eval_fusable(x, [chain[1]], chain[2])
        y = chain(x)
        y64 = ref(x.double())
    assert rel_err(y, y64) < 1e-5
