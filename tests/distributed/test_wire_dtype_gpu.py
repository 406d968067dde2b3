"""``wire_dtype=torch.bfloat16`` with device tensors, rehearsed on ONE GPU: the ranks share
``cuda:0`` and exchange host-staged wire buffers over gloo (as
``test_shared_gpu_rehearsal.py``), so the HIP encode runs ahead of the host copy, the decode
after the upload, the persistent wire / decoded buffers feed captured cells, and striped
pieces are pieces of the wire buffer.

The fp32 one-process reference on the GPU is the yardstick; the bound is four times the
gloo CPU ranks' measured error (``test_wire_dtype.py``): rounding dominates, and device
arithmetic only moves which elements sit on a tie.
"""
import pytest
import torch

from tests.distributed import parity
from tests.distributed.mp_util import run
from tests.distributed.test_wire_dtype import MEASURED_LOSS_ERROR, MEASURED_WIRE_ERROR

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
CHUNKS = 3
GPU_REL = {kind: 4 * err for kind, err in MEASURED_WIRE_ERROR.items()}
GPU_LOSS_REL = 4 * MEASURED_LOSS_ERROR
REL = 1e-4  # fp32 parity: a bf16 wire must exceed it

_reference = {}


def reference(kind):
    if kind not in _reference:
        _reference[kind] = parity.reference(kind, torch.device('cuda', 0), CHUNKS)
    return _reference[kind]


def _check(results, kind):
    grads, loss = reference(kind)
    got = [g for r in results for g in r['grads']]
    errs = [(a.double() - b.double()).norm().item() / (b.double().norm().item() + 1e-12)
            for a, b in zip(got, grads)]
    loss_err = abs(results[-1]['loss'] - loss) / max(1.0, abs(loss))
    print(f'wire parity {kind} on one GPU: gradient error {max(errs):.3e}, '
          f'loss error {loss_err:.3e}')
    assert max(errs) > REL, 'the wire was not rounded'
    parity.assert_parity(results, grads, loss, rel=GPU_REL[kind])
    assert loss_err <= GPU_LOSS_REL, loss_err


@pytest.mark.parametrize('kind', parity.MODELS)
def test_eager_two_ranks(tmp_path, kind):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    results = run(parity.stage_worker, 2, tmp_path, kind, CHUNKS, 'except_last', 'cuda-shared',
                  dict(wire_dtype=BF16), backend='gloo', timeout=120)
    _check(results, kind)


def test_captured_cells_read_the_decoded_buffers(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    results = run(parity.stage_worker, 2, tmp_path, 'unet', CHUNKS, 'except_last',
                  'cuda-shared', dict(wire_dtype=BF16, graph_cells=True, steps=5),
                  backend='gloo', timeout=120)
    _check(results, 'unet')
    want = ['eager', 'eager', 'capture', 'replay', 'replay']
    assert all(r['phases'] == want for r in results), [r['phases'] for r in results]


def test_striped_wire_buffers(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    results = run(parity.stage_worker, 4, tmp_path, 'amoebanet', CHUNKS, 'except_last',
                  'cuda-shared', dict(wire_dtype=BF16, stripes=1, steps=3),
                  backend='gloo', timeout=120)
    _check(results, 'amoebanet')
    assert results[0]['stripes'], 'nothing striped'
    assert any(r['relay_jobs'] for r in results)
