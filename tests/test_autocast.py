"""``torch.autocast`` through GPipe, checkpointing and PipelineStage.

CPU: the autocast state of the calling thread follows every micro-batch to the device
threads and into its recomputation, whichever thread recomputes and however long after the
``with`` block; caches keyed on the step's mode tell autocast steps from plain ones.
GPU: the dtype-following U-Net ops run their bf16 kernels with a bit-exact Philox replay,
and the native fp32 convolutions step aside for the library's under autocast.
"""
import copy

import pytest
import torch
from torch import nn

from torchgpipe_amd import GPipe
from torchgpipe_amd import checkpoint as chk
from torchgpipe_amd.parallel import PipelineStage
from torchgpipe_amd.parallel.loopback import LoopbackP2P
from torchgpipe_amd.parallel.stage import signature_of
from torchgpipe_amd.utils import autocast

BF16 = torch.bfloat16


def bf16_cpu(enabled=True):
    return torch.autocast('cpu', dtype=BF16, enabled=enabled)


class Probe(nn.Module):
    """Records ``(autocast enabled, autocast dtype, is_recomputing)`` per call, and its
    input where asked to."""

    def __init__(self, kind='cpu', keep_input=False):
        super().__init__()
        self.kind = kind
        self.keep_input = keep_input
        self.calls = []
        self.inputs = []

    def forward(self, x):
        self.calls.append((torch.is_autocast_enabled(self.kind),
                           torch.get_autocast_dtype(self.kind), chk.is_recomputing()))
        if self.keep_input:
            self.inputs.append((chk.is_recomputing(), x.detach().clone()))
        return x

    def passes(self):
        """The records of the forward passes and of the recomputations, without the flag."""
        fwd = [c[:2] for c in self.calls if not c[2]]
        rec = [c[:2] for c in self.calls if c[2]]
        return fwd, rec


def mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 4))


# -- GPipe ----------------------------------------------------------------------------------

@pytest.mark.parametrize('checkpoint', ['never', 'except_last', 'always'])
def test_gpipe_follows_autocast(checkpoint):
    model = mlp()
    direct = copy.deepcopy(model)
    gpipe = GPipe(model, balance=[2, 1], devices=['cpu', 'cpu'], chunks=2, checkpoint=checkpoint)
    x = torch.randn(4, 8)
    with bf16_cpu():
        y = gpipe(x)
    # the direct run: chunk by chunk, each under the same autocast (a block per chunk, as a
    # micro-batch's task has: a weight's bf16 cast is then made per micro-batch, and the
    # micro-batches' gradients meet in the fp32 ``.grad``, not in a shared bf16 cast)
    outs = []
    for c in x.chunk(2):
        with bf16_cpu():
            outs.append(direct[2](direct[1](direct[0](c))))
    want = torch.cat(outs)
    assert y.dtype == BF16 and want.dtype == BF16
    assert torch.equal(y, want)
    # backward after the block, the documented pattern
    y.float().sum().backward()
    want.float().sum().backward()
    for p, q in zip(gpipe.parameters(), direct.parameters()):
        assert p.grad.dtype == torch.float32
        assert torch.equal(p.grad, q.grad)
    # the worker threads are back to "off": the next call outside autocast is fp32
    assert gpipe(x).dtype == torch.float32


def test_gpipe_recomputes_under_the_forward_autocast_state():
    probe = Probe()
    model = nn.Sequential(nn.Linear(8, 8), probe, nn.Linear(8, 4))
    gpipe = GPipe(model, balance=[2, 1], devices=['cpu', 'cpu'], chunks=2, checkpoint='always')
    x = torch.randn(4, 8)
    with bf16_cpu():
        y = gpipe(x)
    y.float().sum().backward()
    fwd, rec = probe.passes()
    assert fwd == [(True, BF16)] * 2 and rec == fwd

    # outside autocast: (False, ...) in both passes, as before
    probe.calls.clear()
    gpipe(x).sum().backward()
    fwd, rec = probe.passes()
    assert [c[0] for c in fwd] == [False, False] and rec == fwd

    # an inner disabled region wins in both passes, even when backward() runs under autocast
    probe.calls.clear()
    with bf16_cpu():
        with bf16_cpu(enabled=False):
            y = gpipe(x)
        assert y.dtype == torch.float32
        y.sum().backward()
    fwd, rec = probe.passes()
    assert [c[0] for c in fwd] == [False, False] and rec == fwd


def test_checkpoint_function_recomputes_under_the_forward_autocast_state():
    probe = Probe()
    layer = nn.Sequential(nn.Linear(8, 8), probe)
    x = torch.randn(2, 8, requires_grad=True)
    with bf16_cpu():
        y = chk.checkpoint(layer, x)
    assert y.dtype == BF16
    y.float().sum().backward()
    fwd, rec = probe.passes()
    assert fwd == [(True, BF16)] and rec == fwd

    probe.calls.clear()
    chk.checkpoint(layer, x).sum().backward()
    fwd, rec = probe.passes()
    assert fwd[0][0] is False and rec == fwd

    probe.calls.clear()
    with bf16_cpu():
        with bf16_cpu(enabled=False):
            y = chk.checkpoint(layer, x)
        y.sum().backward()
    fwd, rec = probe.passes()
    assert fwd[0][0] is False and rec == fwd


def test_autocast_state_round_trip():
    """The one helper: capture here, re-enter elsewhere, and leave nothing behind."""
    off = autocast.capture()
    assert not off.any_enabled and off.entered() is off.entered()   # nothing to enter
    with bf16_cpu():
        on = autocast.capture()
    assert on.any_enabled and on != off and hash(on) != hash(off)
    with on.entered():
        assert torch.is_autocast_enabled('cpu') and torch.get_autocast_dtype('cpu') == BF16
        with off.entered():
            assert not torch.is_autocast_enabled('cpu')
        assert torch.is_autocast_enabled('cpu')
    assert autocast.capture() == off
    with on.entered(cache=False):
        assert not torch.is_autocast_cache_enabled()
    assert torch.is_autocast_cache_enabled()


# -- PipelineStage --------------------------------------------------------------------------

@pytest.mark.parametrize('backward_thread', [False, True], ids=['inline', 'helper-thread'])
def test_stage_recomputes_under_the_forward_autocast_state(backward_thread):
    probe = Probe()
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(8, 8), probe, nn.Linear(8, 4))
    stage = PipelineStage(model, [3], device=torch.device('cpu'), chunks=2, checkpoint='always',
                          backward_thread=backward_thread)
    x = torch.randn(4, 8)
    with bf16_cpu():
        outs = stage.forward(x)
    assert all(o.dtype == BF16 for o in outs)
    stage.backward([o.float().sum() for o in outs])
    fwd, rec = probe.passes()
    assert fwd == [(True, BF16)] * 2 and rec == fwd
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in model.parameters())

    probe.calls.clear()
    outs = stage.forward(x)
    assert all(o.dtype == torch.float32 for o in outs)
    stage.backward([o.sum() for o in outs])
    fwd, rec = probe.passes()
    assert [c[0] for c in fwd] == [False, False] and rec == fwd


@pytest.mark.parametrize('first', ['plain', 'autocast'])
def test_stage_message_metadata_is_keyed_on_the_autocast_state(first):
    """Rank 0 of 2 on the loopback transport: the gradient message of an autocast step is
    bf16, that of a plain step fp32, in either order -- neither reuses the other's."""
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 4))
    transport = LoopbackP2P(torch.device('cpu'), [torch.rand(2, 8)], True, {})
    stage = PipelineStage(model, [2, 1], rank=0, chunks=2, transport=transport)
    x = torch.randn(4, 8)
    sig = signature_of(x)

    def step(amp):
        with bf16_cpu(enabled=amp):
            stage.forward(x, signature=sig)
        sent = transport._sent[('act', 0, 1)][0].dtype
        stage.backward(None)      # outside the block
        return sent

    order = [False, True] if first == 'plain' else [True, False]
    assert [step(amp) for amp in order] == [BF16 if amp else torch.float32 for amp in order]
    gact = {key: bufs[0].dtype for key, bufs in transport._bufs.items() if key[3] == 'gact'}
    assert sorted(str(d) for d in gact.values()) == ['torch.bfloat16'] * 2 + ['torch.float32'] * 2
    assert all(len(key) == 7 for key in gact)


def test_op_modules_on_cpu_are_unchanged_by_autocast():
    """Off the GPU the op modules are the plain layers, with or without autocast."""
    from torchgpipe_amd.ops import fusion
    from torchgpipe_amd.ops.conv import WinogradConv2d
    from torchgpipe_amd.ops.convbn import GemmConv2d
    from torchgpipe_amd.ops.precision import autocast_lowp
    torch.manual_seed(0)
    x = torch.randn(2, 8, 8, 8)
    assert not autocast_lowp('cpu') and not autocast_lowp('cuda')
    for layer in (WinogradConv2d(8, 8, 3, padding=1), GemmConv2d(8, 4, 1, bias=False),
                  fusion.ConvBN2d(8, 8, 3, padding=1, bias=False)):
        plain = nn.Conv2d.forward(layer, x)
        assert torch.equal(layer(x), plain)
        with bf16_cpu():
            assert autocast_lowp('cpu')
            got, want = layer(x), nn.Conv2d.forward(layer, x)
        assert got.dtype == BF16 and torch.equal(got, want)
    lin = fusion.Linear(8, 4)
    with bf16_cpu():
        got, want = lin(x), nn.Linear.forward(lin, x)
    assert got.dtype == BF16 and torch.equal(got, want)


# -- GPU ------------------------------------------------------------------------------------

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from torchgpipe_amd.ops import _ext
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'
    return torch.device('cuda', 0)


def _epilogue_chain(probe):
    from torchgpipe_amd.models.unet import PopUpCat, Stash
    from torchgpipe_amd.ops.fused import DropNormAct
    from torchgpipe_amd.ops.unet_ops import MaxPool2x2
    from torchgpipe_amd.skip import Namespace
    ns = Namespace()
    return nn.Sequential(DropNormAct(p=0.3), Stash().isolate(ns), MaxPool2x2(), probe,
                         DropNormAct(p=0.3), PopUpCat().isolate(ns))


@pytest.mark.gpu
def test_bf16_epilogue_chain_through_gpipe_replays_philox():
    """No convolution, so nothing non-deterministic: the recomputation sees bit for bit the
    checkpointed pass's tensors (the Philox replay in bf16), and output and input gradient
    equal the direct micro-batch loop after the same seed."""
    dev = _need_gpu()
    probe = Probe('cuda', keep_input=True)
    model = _epilogue_chain(probe)
    gpipe = GPipe(model, balance=[6], devices=[dev], chunks=2, checkpoint='always')
    x0 = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(1)).bfloat16().to(dev)
    dy = torch.randn(4, 8, 8, 8, generator=torch.Generator().manual_seed(2)).bfloat16().to(dev)

    torch.cuda.manual_seed(1234)
    x = x0.clone().requires_grad_(True)
    y = gpipe(x)
    assert y.dtype == BF16 and y.shape == (4, 8, 8, 8)
    y.backward(dy)
    first = [t for rec, t in probe.inputs if not rec]
    again = [t for rec, t in probe.inputs if rec]
    assert len(first) == len(again) == 2
    # (recomputations run in reverse micro-batch order)
    for a in first:
        assert a.dtype == BF16 and any(torch.equal(a, b) for b in again)
    assert not torch.equal(first[0], first[1])

    torch.cuda.manual_seed(1234)
    direct = copy.deepcopy(gpipe.partitions[0]).to(dev)
    xd = x0.clone().requires_grad_(True)
    from torchgpipe_amd.skip.tracker import SkipTracker, use_skip_tracker
    outs = []
    for c in xd.chunk(2):
        with use_skip_tracker(SkipTracker()):
            outs.append(direct(c))
    yd = torch.cat(outs)
    yd.backward(dy)
    assert torch.equal(y, yd)
    assert x.grad.dtype == BF16 and torch.equal(x.grad, xd.grad)


@pytest.mark.gpu
def test_bf16_epilogue_chain_in_captured_cells():
    """``PipelineStage(graph_cells=True)`` past its capture step on bf16 tensors, as rank 1
    of 2 on the loopback transport (received activations require grad, so the captured
    backward graphs run the bf16 backward kernels): the captured recomputation reads the
    slot the captured forward read (bit-equal probe inputs), and outputs and input
    gradients equal an eager run under the very slot values."""
    from torchgpipe_amd.skip.tracker import SkipTracker, use_skip_tracker
    from torchgpipe_amd.utils import rng
    dev = _need_gpu()
    probe = Probe('cuda', keep_input=True)
    model = nn.Sequential(nn.Identity(), *_epilogue_chain(probe))
    gen = torch.Generator().manual_seed(1)
    template = torch.randn(2, 4, 8, 8, generator=gen).bfloat16().to(dev)
    weights = [torch.randn(2, 8, 8, 8, generator=gen).to(dev) for _ in range(2)]
    transport = LoopbackP2P(dev, [template], True, {})
    stage = PipelineStage(model, [1, 6], rank=1, device=dev, chunks=2, checkpoint='always',
                          graph_cells=True, transport=transport)
    assert stage.is_last and not stage.is_first
    sig = signature_of(torch.empty(4, 4, 8, 8, dtype=BF16))
    captured_from = None
    for step in range(5):
        mark = len(probe.inputs)
        outs = stage.forward(None, signature=sig)
        if stage.graph_phase == 'capture':
            captured_from = mark
        stage.backward([(o.float() * w).sum() for o, w in zip(outs, weights)])
    assert stage.graph_phase == 'replay'
    assert all(o.dtype == BF16 for o in outs)
    torch.cuda.synchronize()
    # the probe ran in the eager warm-up and in the capture step only; the tensors it cloned
    # inside the captures are rewritten by every replay: the last step's values
    assert captured_from is not None and len(probe.inputs) == captured_from + 4
    records = probe.inputs[captured_from:]
    first = [t for rec, t in records if not rec]
    again = [t for rec, t in records if rec]
    assert len(first) == len(again) == 2
    for a in first:
        assert a.dtype == BF16 and any(torch.equal(a, b) for b in again)
    slots = stage._segments.slots.clone()
    oracle = copy.deepcopy(stage.partition)
    for i in range(2):
        key = next(k for k in transport._bufs if k[3] == 'act' and k[4] == i)
        c = transport._bufs[key][0].detach().clone().requires_grad_(True)
        with rng.slot_scope(rng.PhiloxSlot(slots[i].clone())), use_skip_tracker(SkipTracker()):
            want = oracle(c)
        (want.float() * weights[i]).sum().backward()
        assert torch.equal(outs[i].detach(), want.detach())
        # the captured backward's static input gradient (what the stage ships upstream)
        gin = stage._segments.cells[i].gins[0]
        assert gin.dtype == BF16 and gin.abs().max() > 0
        assert torch.equal(gin, c.grad)


def _count_native_convs(monkeypatch):
    """Wrap the entry points of the native fp32 convolutions; returns the call counter."""
    from torchgpipe_amd.ops import conv, convbn
    calls = {'n': 0}

    def counted(fn):
        def wrapper(*args, **kwargs):
            calls['n'] += 1
            return fn(*args, **kwargs)
        return wrapper

    monkeypatch.setattr(conv._WinogradConv, 'apply', counted(conv._WinogradConv.apply))
    monkeypatch.setattr(convbn, 'gemm_conv2d', counted(convbn.gemm_conv2d))
    monkeypatch.setattr(convbn._GemmConv, 'apply', counted(convbn._GemmConv.apply))
    monkeypatch.setattr(convbn._ConvBN, 'apply', counted(convbn._ConvBN.apply))
    monkeypatch.setattr(convbn._GroupConvBN, 'apply', counted(convbn._GroupConvBN.apply))
    monkeypatch.setattr(convbn, 'conv_bn_eval', counted(convbn.conv_bn_eval))
    return calls


@pytest.mark.gpu
def test_unet_under_autocast_runs_bf16_epilogues_and_library_convolutions(monkeypatch):
    from torchgpipe_amd.models import unet
    from torchgpipe_amd.ops.fused import DropNormAct
    dev = _need_gpu()
    torch.manual_seed(0)
    model = unet(depth=2, num_convs=2, base_channels=8)
    gpipe = GPipe(model, balance=[len(model)], devices=[dev], chunks=2, checkpoint='always')
    seen = []
    for m in gpipe.modules():
        if isinstance(m, DropNormAct):
            m.register_forward_pre_hook(
                lambda mod, args: seen.append((chk.is_recomputing(), args[0].dtype)))
    calls = _count_native_convs(monkeypatch)
    x = torch.rand(2, 3, 16, 16, device=dev)

    with torch.autocast('cuda', dtype=BF16):
        y = gpipe(x)
    assert y.dtype == BF16
    y.float().mean().backward()       # outside the block
    for name, p in gpipe.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, name
        assert torch.isfinite(p.grad).all(), name
    assert calls['n'] == 0, 'a native fp32 convolution ran under autocast'
    assert {d for _, d in seen} == {BF16}
    assert sum(rec for rec, _ in seen) == sum(not rec for rec, _ in seen) > 0

    # outside autocast nothing changed: fp32 end to end on the native convolutions
    seen.clear()
    for p in gpipe.parameters():
        p.grad = None
    y = gpipe(x)
    assert y.dtype == torch.float32
    y.mean().backward()
    assert calls['n'] > 0
    assert {d for _, d in seen} == {torch.float32}


class _Grouped(nn.Module):
    """Two ReLU-Conv1x1-BN chains reading one input, grouped where the grouped op takes them
    (as AmoebaNet's cell does), one by one otherwise; the outputs concatenated."""

    def __init__(self, chain):
        super().__init__()
        self.chains = nn.ModuleList([
            chain(nn.ReLU(), nn.Conv2d(8, 8, 1, bias=False), nn.BatchNorm2d(8))
            for _ in range(2)])
        self.grouped = 0

    def forward(self, x):
        from torchgpipe_amd.ops import convbn
        outs = None
        if isinstance(self.chains[0], convbn.FusedChain):
            triplets = [c._triplets()[0] for c in self.chains]
            if convbn.groupable(x, triplets):
                if '_cache' not in self.__dict__:
                    self.__dict__['_cache'] = convbn._GroupCache()
                self.grouped += 1
                outs = convbn.group_relu_conv_bn(x, triplets, self.__dict__['_cache'])
        if outs is None:
            outs = [c(x) for c in self.chains]
        return torch.cat(list(outs), 1)


def _stepping_aside_modules():
    from torchgpipe_amd.models.resnet import bottleneck
    from torchgpipe_amd.ops import convbn, fusion
    from torchgpipe_amd.ops.conv import WinogradConv2d
    from torchgpipe_amd.ops.convbn import GemmConv2d
    torch.manual_seed(0)
    linked = nn.Sequential(fusion.ConvBN2d(8, 8, 3, padding=1, bias=False),
                           fusion.BatchNormAct2d(8), fusion.ReLU())
    fusion.relink(linked)
    plain_linked = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8),
                                 nn.ReLU())
    plain_linked.load_state_dict(linked.state_dict())
    pointwise = nn.Sequential(fusion.ConvBN2d(8, 16, 1, bias=False), fusion.BatchNormAct2d(16))
    fusion.relink(pointwise)
    plain_pointwise = nn.Sequential(nn.Conv2d(8, 16, 1, bias=False), nn.BatchNorm2d(16))
    plain_pointwise.load_state_dict(pointwise.state_dict())
    wino = WinogradConv2d(8, 8, 3, padding=1)
    few = WinogradConv2d(3, 8, 3, padding=1, bias=False)     # the gemm_conv2d branch
    gemm = GemmConv2d(8, 4, 1, bias=False)
    lin = fusion.Linear(8, 4)
    # FusedChain / ReLUConvBN: a 1x1 triplet, and a chain of a 3x3 and a 1x1 triplet
    chain1 = convbn.ReLUConvBN(nn.ReLU(), nn.Conv2d(8, 8, 1, bias=False), nn.BatchNorm2d(8))
    plain_chain1 = nn.Sequential(nn.ReLU(), nn.Conv2d(8, 8, 1, bias=False), nn.BatchNorm2d(8))
    plain_chain1.load_state_dict(chain1.state_dict())
    chain2 = convbn.FusedChain(nn.ReLU(), nn.Conv2d(8, 16, 3, padding=1, bias=False),
                               nn.BatchNorm2d(16), nn.Conv2d(16, 8, 1, bias=False),
                               nn.BatchNorm2d(8))
    plain_chain2 = nn.Sequential(nn.ReLU(), nn.Conv2d(8, 16, 3, padding=1, bias=False),
                                 nn.BatchNorm2d(16), nn.Conv2d(16, 8, 1, bias=False),
                                 nn.BatchNorm2d(8))
    plain_chain2.load_state_dict(chain2.state_dict())
    grouped = _Grouped(convbn.ReLUConvBN)
    plain_grouped = _Grouped(nn.Sequential)
    plain_grouped.load_state_dict(grouped.state_dict())
    # ResNet's bottleneck: conv3 / bn3 left pending for the residual join (pending_join)
    block = bottleneck(8, 2, fused=True)
    assert fusion.relink(block) == 3
    plain_block = bottleneck(8, 2, fused=False)
    plain_block.load_state_dict(block.state_dict())
    return [
        ('ReLUConvBN-1x1', chain1, plain_chain1, (2, 8, 8, 8)),
        ('FusedChain-3x3-1x1', chain2, plain_chain2, (2, 8, 8, 8)),
        ('grouped-ReLUConvBN', grouped, plain_grouped, (2, 8, 8, 8)),
        ('bottleneck-join', block, plain_block, (2, 8, 8, 8)),
        ('WinogradConv2d', wino, lambda m, x: nn.Conv2d.forward(m, x), (2, 8, 8, 8)),
        ('WinogradConv2d-few-channels', few, lambda m, x: nn.Conv2d.forward(m, x), (2, 3, 8, 8)),
        ('GemmConv2d', gemm, lambda m, x: nn.Conv2d.forward(m, x), (2, 8, 8, 8)),
        ('Linear', lin, lambda m, x: nn.Linear.forward(m, x), (2, 8, 8, 8)),
        ('ConvBN2d-3x3-relu', linked, plain_linked, (2, 8, 8, 8)),
        ('ConvBN2d-1x1', pointwise, plain_pointwise, (2, 8, 8, 8)),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_native_ops_step_aside_under_autocast(mode, monkeypatch):
    """Under autocast each module is its plain ``nn`` forward on the same weights: the same
    library call, so bit-equal, and bf16."""
    dev = _need_gpu()
    calls = _count_native_convs(monkeypatch)
    from torchgpipe_amd.skip.tracker import SkipTracker, use_skip_tracker
    for name, module, plain, shape in _stepping_aside_modules():
        module = module.to(dev).train(mode == 'train')
        x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(dev)
        if isinstance(plain, nn.Module):
            plain = plain.to(dev).train(mode == 'train')
            run_plain = plain
        else:
            run_plain = (lambda fn, m: lambda t: fn(m, t))(plain, module)
        with torch.autocast('cuda', dtype=BF16), torch.set_grad_enabled(mode == 'train'), \
                use_skip_tracker(SkipTracker()):
            want = run_plain(x)
            again = run_plain(x) if not isinstance(plain, nn.Module) else None
            got = module(x)
        # (the residual join adds the fp32 block input: fp32 out of both, by type promotion)
        assert got.dtype == want.dtype == (torch.float32 if name == 'bottleneck-join' else BF16), \
            name
        if again is not None:
            assert torch.equal(again, want), f'{name}: two plain calls differ'
        assert torch.equal(got, want), name
        assert getattr(module, 'grouped', 0) == 0, 'the grouped op ran under autocast'
        if mode == 'train':
            got.float().sum().backward()
            for pname, p in module.named_parameters():
                assert p.grad is not None and p.grad.dtype == torch.float32, (name, pname)
        assert calls['n'] == 0, f'{name}: a native fp32 op ran under autocast'
    # the guard is what kept them away: outside autocast the same modules run the native ops
    for name, module, plain, shape in _stepping_aside_modules():
        if name == 'Linear':
            continue  # (no fp32 convolution entry point to count)
        module = module.to(dev).train(mode == 'train')
        x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(dev)
        before = calls['n']
        with torch.set_grad_enabled(mode == 'train'), use_skip_tracker(SkipTracker()):
            out = module(x)
        assert out.dtype == torch.float32
        assert calls['n'] > before, f'{name}: no native op outside autocast'
