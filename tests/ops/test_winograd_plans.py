"""The Winograd host plans match a recording of the hand-written dispatch (CPU check).

``data/winograd_plans.json`` holds what ``wino4_plan``, the ``wino4_wgrad`` binding's
split / workspace arithmetic and ``bg_plan`` returned at the commit named in it, before
their variant lists became tables (``kF4Variants``, ``kBgTiles``, ``kBgEmuTiles`` in
csrc/winograd_f4.hip): every forward variant id from -1 to 23, the weight-gradient
variants 0-3 and every batched-GEMM tile (with auto and invalid ones), over shapes that
take each width precondition, fallback and workspace layout, with requested and modelled
split counts.  The three ``*_plan_info`` ops must return the same numbers, case by case.

The extension loads in a child process (a bad schema aborts at import); skipped when it
has not been built in-tree.
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
f, g, b = doc['forward'], doc['wgrad'], doc['bg']
out = {
    'forward': [list(ops.wino4_plan_info(*s, v, sp)) for s, v, sp in
                itertools.product(f['shapes'], f['variants'], f['splits'])],
    'wgrad': [list(ops.wino4_wgrad_plan_info(*s, v, sp)) for s, v, sp in
              itertools.product(g['shapes'], g['variants'], g['splits'])],
    'bg': [list(ops.bg_plan_info(*s, t[1], sp, kind, t[0], t[2], emu))
           for s, kind, emu, t, sp in
           itertools.product(b['shapes'], b['kinds'], b['emus'], b['tiles'], b['splits'])],
    # wino4_splits stays for its callers, on top of the plan functions
    'splits': [[ops.wino4_splits(*s, v) for v in (0, 6, 7)] for s in g['shapes']],
}
print(json.dumps(out))
'''


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def plans():
    if not any(f.startswith('_C') and f.endswith('.so')
               for f in os.listdir(os.path.join(ROOT, 'torchgpipe_amd'))):
        pytest.skip('extension not built (python -m torchgpipe_amd._build)')
    # TGPIPE_BG_EMU must play no part: every batched-GEMM case names emu 0 or 1
    res = subprocess.run([sys.executable, '-c', _CHILD, FIXTURE], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _compare(cases, got, want):
    cases = list(cases)
    assert len(cases) == len(got) == len(want)
    wrong = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, f'{len(wrong)} of {len(cases)} plans differ; (case, got, recorded): ' \
                      f'{wrong[:5]}'


def test_fixture_covers_the_cases(recorded):
    """The recording has the variant ids, shapes and split requests the table rows need:
    W % 4 != 0, W = 8, W < 8, W >= 24, the non-fused workspace, a 1 x 1 plane."""
    f, g, b = recorded['forward'], recorded['wgrad'], recorded['bg']
    assert f['variants'] == list(range(-1, 24)) and f['splits'] == [0, 1, 3, 1000]
    for shape in ([2, 64, 64, 24, 24], [1, 24, 130, 14, 10], [2, 40, 64, 8, 8],
                  [2, 64, 64, 4, 4], [1, 4, 64, 12, 192], [1, 64, 192, 20, 36],
                  [22, 128, 128, 28, 28], [16, 512, 512, 12, 12], [1, 16, 8, 1, 1]):
        assert shape in f['shapes']
    assert g['variants'] == [0, 1, 2, 3] and g['splits'] == [0, 1, 2, 1000]
    for shape in ([22, 256, 256, 14, 14], [2, 64, 64, 24, 24], [3, 16, 96, 9, 12],
                  [1, 24, 130, 14, 10], [16, 512, 512, 12, 12], [1, 16, 8, 1, 1]):
        assert shape in g['shapes']
    assert b['kinds'] == [4, 2] and b['emus'] == [0, 1] and b['splits'] == [0, 1, 4, 1000]
    tiles = [[4, 48], [4, 64], [4, 96], [4, 128], [8, 64], [8, 96], [8, 128], [8, 144]]
    for tile in [[0, 0, 0], [8, 48, 1], [4, 144, 1], [4, 64, 3]] + \
            [[wv, bn, sub] for wv, bn in tiles for sub in (1, 2)]:
        assert tile in b['tiles']
    for shape in ([16, 256, 256, 12, 12], [2, 256, 512, 6, 6], [40, 512, 512, 24, 24],
                  [22, 256, 256, 14, 14], [1, 256, 256, 8, 8]):
        assert shape in b['shapes']
    assert len(recorded['recorded_at']) == 40
    assert os.path.getsize(FIXTURE) < 100 * 1024


def test_forward_plans_match_the_recording(recorded, plans):
    f = recorded['forward']
    _compare(itertools.product(f['shapes'], f['variants'], f['splits']), plans['forward'],
             f['results'])


def test_known_variants_match_the_recording(recorded, plans):
    """An id plans as itself or as its width fallback exactly when the hand-written check
    accepted it; every other id (and -1) plans as 5.  A known id other than 5 never
    becomes 5 (no fallback is 5), so this pins ``wino4_variant_known``."""
    f = recorded['forward']
    known = set(recorded['forward_known'])
    assert known == {4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16, 17, 18, 20, 21, 22}
    cases = itertools.product(f['shapes'], f['variants'], f['splits'])
    for (shape, variant, _), got in zip(cases, plans['forward']):
        if variant in known and variant != 5:
            assert got[0] != 5, (shape, variant, got)
        else:
            assert got[0] == 5, (shape, variant, got)
        assert got[1] == (2 if got[0] in (5, 7, 15, 17) else 4), (shape, variant, got)


def test_wgrad_plans_match_the_recording(recorded, plans):
    g = recorded['wgrad']
    cases = list(itertools.product(g['shapes'], g['variants'], g['splits']))
    _compare(cases, plans['wgrad'], g['results'])
    # wino4_splits(..., 0) is the fused weight gradient's modelled count, (..., 6 / 7) the
    # forward variants'
    f = recorded['forward']
    fcases = list(itertools.product(f['shapes'], f['variants'], f['splits']))
    for shape, picks in zip(g['shapes'], plans['splits']):
        assert picks[0] == g['results'][cases.index((shape, 0, 0))][1]
        if shape in f['shapes']:
            for variant, pick in zip((6, 7), picks[1:]):
                assert pick == f['results'][fcases.index((shape, variant, 0))][2]


def test_bg_plans_match_the_recording(recorded, plans):
    b = recorded['bg']
    _compare(itertools.product(b['shapes'], b['kinds'], b['emus'], b['tiles'], b['splits']),
             plans['bg'], b['results'])
