"""Ids 25 (forward / backward-data) and 4 (weight gradient) keep the serial-step bodies of the
row-staged fused F(4x4) kernels and take the planning of ids 16 / 3 (CPU check): on the
shapes and split requests of ``data/winograd_plans.json`` their plans equal those of 16 / 3
-- the same og, split count and workspace, the same width fallback -- and differ in the
reported id only where the row-staged kernel itself runs.

The extension loads in a child process, as in test_winograd_plans.py; skipped when it has
not been built in-tree.
"""
import itertools
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, 'data', 'winograd_plans.json')

_CHILD = r'''
import itertools, json, sys, torch, torchgpipe_amd._C
ops = torch.ops.tgpipe
doc = json.load(open(sys.argv[1]))
f, g = doc['forward'], doc['wgrad']
out = {
    'forward': [[list(ops.wino4_plan_info(*s, v, sp)) for v in (16, 25)]
                for s, sp in itertools.product(f['shapes'], f['splits'])],
    'wgrad': [[list(ops.wino4_wgrad_plan_info(*s, v, sp)) for v in (3, 4)]
              for s, sp in itertools.product(g['shapes'], g['splits'])],
}
print(json.dumps(out))
'''


@pytest.fixture(scope='module')
def plans():
    if not any(f.startswith('_C') and f.endswith('.so')
               for f in os.listdir(os.path.join(ROOT, 'torchgpipe_amd'))):
        pytest.skip('extension not built (python -m torchgpipe_amd._build)')
    res = subprocess.run([sys.executable, '-c', _CHILD, FIXTURE], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(pairs, new_id, kept_id):
    assert pairs
    ran_rows = 0
    for new, kept in pairs:
        # [variant that runs, ...]: the id itself, or the shared width fallback
        assert new[1:] == kept[1:], (new, kept)
        if new[0] == new_id:
            assert kept[0] == kept_id, (new, kept)
            ran_rows += 1
        else:
            assert kept[0] == new[0], (new, kept)
    assert 0 < ran_rows < len(pairs)   # the fixture has both kinds of width


def test_forward_id_25_plans_as_16(plans):
    _check(plans['forward'], 16, 25)


def test_wgrad_id_4_plans_as_3(plans):
    _check(plans['wgrad'], 3, 4)
