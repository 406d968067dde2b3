"""Host side of the fused split-bf16 F(4x4) kernel (variant 24), checked without a GPU: the
routing function of ops/conv.py and the plan of the new table row.

The plan cases load the extension in a child process, as tests/ops/test_winograd_plans.py
does; skipped when it has not been built in-tree.
"""
import json
import os
import subprocess
import sys

import pytest

from torchgpipe_amd.ops import conv, precision

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# ((N, R, H, W), output channels) -> the variant picked before the precision level played a
# part, written down from that dispatch: >= 512 output channels 14, or 15 on grids under
# 160 64-channel blocks; else 7 up to 32 output channels or under 160 blocks, else 16, which
# is 6 below W = 24.  U-Net(5,64) at micro-batch 40 (forward and backward-data), ResNet-101's
# 3x3s at 22 and 110 images.
HIGHEST = [
    ((40, 32, 192, 192), 32, 7), ((40, 32, 192, 192), 128, 16), ((40, 64, 192, 192), 64, 16),
    ((40, 64, 192, 192), 128, 16), ((40, 128, 192, 192), 32, 7), ((40, 128, 192, 192), 64, 16),
    ((40, 64, 96, 96), 128, 16), ((40, 64, 96, 96), 256, 16), ((40, 128, 96, 96), 64, 16),
    ((40, 128, 96, 96), 128, 16), ((40, 256, 96, 96), 64, 16), ((40, 64, 48, 48), 64, 16),
    ((40, 64, 48, 48), 256, 16), ((40, 256, 48, 48), 64, 16), ((40, 128, 24, 24), 128, 7),
    ((40, 512, 24, 24), 128, 7), ((40, 128, 24, 24), 512, 14),
    ((22, 64, 56, 56), 64, 7), ((110, 64, 56, 56), 64, 16), ((22, 128, 28, 28), 128, 7),
    ((110, 128, 28, 28), 128, 16), ((22, 256, 14, 14), 256, 7), ((110, 256, 14, 14), 256, 6),
    ((110, 512, 7, 7), 512, 15),
]


@pytest.fixture(autouse=True)
def restore_level():
    try:
        yield
    finally:
        precision.set_conv_precision('highest')


@pytest.mark.parametrize('shape,out_channels,variant', HIGHEST)
def test_routing_at_highest_is_the_exact_dispatch(shape, out_channels, variant):
    assert conv.f4_variant(shape, out_channels, 'highest') == variant
    assert conv.f4_variant(shape, out_channels) == variant  # (the default level)


@pytest.mark.parametrize('level', ['high', 'medium'])
def test_routing_at_the_reduced_levels(level):
    """Variant 24 on the measured classes (64-256 output channels, >= 32 input channels,
    planes from 24^2), the exact pick everywhere else."""
    for shape, out_channels, variant in HIGHEST:
        measured = (64 <= out_channels < 512 and shape[1] >= 32 and min(shape[2:]) >= 24)
        assert conv.f4_variant(shape, out_channels, level) == (24 if measured else variant)
    assert conv.f4_variant((1, 64, 24, 24), 64, level) == 24
    assert conv.f4_variant((1, 64, 24, 23), 64, level) == 7     # a narrower plane
    assert conv.f4_variant((1, 16, 24, 24), 64, level) == 7     # one chunk of input channels
    assert conv.f4_variant((1, 64, 24, 24), 48, level) == 7


def test_routing_reads_the_level_in_force():
    shape, out_channels = (40, 64, 192, 192), 64
    assert conv.f4_variant(shape, out_channels) == 16
    with precision.conv_precision('high'):
        assert conv.f4_variant(shape, out_channels) == 24
        assert conv.f4_variant(shape, out_channels, 'highest') == 16
    assert conv.f4_variant(shape, out_channels) == 16


_CHILD = r'''
import json, sys, torch, torchgpipe_amd._C
ops = torch.ops.tgpipe
print(json.dumps([list(ops.wino4_plan_info(*case)) for case in json.loads(sys.argv[1])]))
'''


def _plans(cases):
    if not any(f.startswith('_C') and f.endswith('.so')
               for f in os.listdir(os.path.join(ROOT, 'torchgpipe_amd'))):
        pytest.skip('extension not built (python -m torchgpipe_amd._build)')
    res = subprocess.run([sys.executable, '-c', _CHILD, json.dumps(cases)], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_plan_of_the_new_row():
    """(n, c, k, h, w, variant, splits) -> [variant, og, splits, workspace floats]: the
    reduction is divided in 16-channel chunks (24 channels are two), a requested split count
    is clamped to them, the workspace holds one output per split, and 23 stays unknown."""
    cases = [
        (2, 128, 64, 8, 8, 24, 1), (2, 128, 64, 8, 8, 24, 3), (2, 128, 64, 8, 8, 24, 1000),
        (3, 24, 48, 10, 14, 24, 1000), (1, 16, 32, 8, 24, 24, 5), (1, 17, 32, 8, 24, 24, 5),
        (3, 24, 48, 10, 14, 23, 1),
    ]
    got = _plans(cases)
    assert got[0] == [24, 4, 1, 0]
    assert got[1] == [24, 4, 3, 3 * 2 * 64 * 8 * 8]
    assert got[2] == [24, 4, 8, 8 * 2 * 64 * 8 * 8]
    assert got[3] == [24, 4, 2, 2 * 3 * 48 * 10 * 14]
    assert got[4] == [24, 4, 1, 0]
    assert got[5] == [24, 4, 2, 2 * 1 * 32 * 8 * 24]
    assert got[6][0] == 5


def test_modelled_split_counts_of_the_new_row():
    """The cost model with the fitted 5.2 us per chunk picks the swept best counts
    (profiles/r11/f4_emu/split_sweep_emu.json) on one-round grids and 1 on full ones."""
    cases = [(15, 128, 128, 28, 28, 24, 0), (22, 128, 128, 28, 28, 24, 0),
             (36, 128, 128, 28, 28, 24, 0), (40, 128, 128, 24, 24, 24, 0),
             (22, 64, 64, 56, 56, 24, 0), (40, 64, 64, 192, 192, 24, 0)]
    assert [p[2] for p in _plans(cases)] == [4, 3, 2, 2, 1, 1]
