"""LoopbackP2P with a bf16 wire: the emulated stage receives what a real bf16 link would
deliver (the boundary tensors rounded through bfloat16 by the HIP encode / decode kernels)
and pays the two kernels per message, eagerly and between captured cells."""
import pytest
import torch
import torch.nn.functional as F

from torchgpipe_amd.microbatch import Batch
from torchgpipe_amd.parallel import PipelineStage
from torchgpipe_amd.parallel.loopback import LoopbackP2P
from torchgpipe_amd.parallel.stage import signature_of
from torchgpipe_amd.skip.tracker import SkipTracker, use_skip_tracker

pytestmark = pytest.mark.gpu

BALANCE = [11, None]  # the skips of the two top levels cross the boundary
SHAPE = (3, 16, 16)
BATCH, CHUNKS = 4, 2


def _stage(graph_cells: bool, dev: torch.device = torch.device('cuda', 0)):
    from torchgpipe_amd.models import unet
    torch.manual_seed(0)
    model = unet(depth=3, num_convs=1, base_channels=4, input_channels=3, output_channels=1)
    for m in model.modules():
        if isinstance(getattr(m, 'p', None), float):
            m.p = 0.0
    model = model.to(dev)
    balance = [BALANCE[0], len(model) - BALANCE[0]]
    tracker = SkipTracker()
    with torch.no_grad(), use_skip_tracker(tracker):
        b = Batch(torch.rand(BATCH // CHUNKS, *SHAPE, device=dev))
        for layer in list(model)[:balance[0]]:
            b = b.call(layer)
    acts = [t.detach().clone() for t in b]
    transport = LoopbackP2P(dev, acts, b.atomic, {}, wire_dtype=torch.bfloat16)
    stage = PipelineStage(model, balance, rank=1, device=dev, chunks=CHUNKS,
                          transport=transport, graph_cells=graph_cells, graph_warmup=1)
    skips = {}
    for src, key in stage.in_skips:
        skips.setdefault(src, []).append(tracker.tensors[key].detach().clone())
    transport.skips = skips
    return stage, transport, acts, skips


def _step(stage):
    dev = stage.device
    t = torch.rand(BATCH, 1, *SHAPE[1:], device=dev)
    sig = signature_of(torch.empty(BATCH, *SHAPE))
    for p in stage.parameters():
        p.grad = None
    loss = stage.train_step(None, t, F.binary_cross_entropy_with_logits, signature=sig)
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)
    assert loss is not None and torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in stage.parameters())


def _rounded(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _check_handed_out(transport, acts, skips):
    seen = {'act': 0, 'skip': 0, 'gact': 0, 'gskip': 0}
    for key, bufs in transport._bufs.items():
        kind, _, src, _ = transport._fields(key)
        seen[kind] += 1
        if kind == 'act':
            tmpl = acts
        elif kind == 'skip':
            tmpl = skips[src]
        else:  # random gradients: representable in bf16 after the round trip
            assert all(torch.equal(b, _rounded(b)) for b in bufs)
            continue
        assert len(bufs) == len(tmpl)
        for b, t in zip(bufs, tmpl):
            assert b.dtype == torch.float32 and b.shape == t.shape
            assert torch.equal(b, _rounded(t))
            assert not torch.equal(b, t)  # (the templates are not bf16 values already)
    assert seen['act'] == CHUNKS and seen['skip'] == CHUNKS


def test_eager_stage_receives_rounded_templates():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    stage, transport, acts, skips = _stage(graph_cells=False)
    captured = []
    first = stage.partition[0]
    handle = first.register_forward_pre_hook(lambda m, args: captured.append(args[0].detach()))
    _step(stage)
    handle.remove()
    _check_handed_out(transport, acts, skips)
    # the partition's first layer read the rounded activation
    assert captured and torch.equal(captured[0], _rounded(acts[0]))
    # what it sent (skip gradients to rank 0) was encoded too: the metas are the logical ones
    assert all(m.dtype == torch.float32 for metas in transport._sent.values() for m in metas)


def test_captured_cells_replay_on_the_decoded_buffers():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    stage, transport, acts, skips = _stage(graph_cells=True)
    phases = []
    addresses = []
    for _ in range(3):
        _step(stage)
        phases.append(stage.graph_phase)
        addresses.append({key: [b.data_ptr() for b in bufs]
                          for key, bufs in transport._bufs.items()})
    assert phases == ['eager', 'capture', 'replay'], phases
    assert addresses[0] == addresses[1] == addresses[2]
    _check_handed_out(transport, acts, skips)
