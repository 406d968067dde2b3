"""Preconditions of the DropNormAct edge tests (``epilogue_cases.py``), checked on the CPU."""
import pytest
import torch

from tests.ops import epilogue_cases as ec

IDS = [case.name for case in ec.ALL_CASES]


def test_case_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize('case', ec.ALL_CASES, ids=IDS)
def test_leaky_relu_margin(case):
    x, dy = ec.make_input(case)
    assert x.dtype == dy.dtype == torch.float32 and x.shape == dy.shape == case.shape
    assert torch.isfinite(x).all() and torch.isfinite(dy).all()
    for training in (False, True):
        margin = ec.min_margin(case, x, training)
        print(f'{case.name} training={training}: min |z| = {margin:.3e}')
        assert margin >= ec.MARGIN
    # the planes keep the offset and spread the case asks for
    flat = x.double().view(case.num_planes, -1)
    assert (flat.mean(1) - case.mean).abs().max() < 2.0 * case.std
    assert (flat.std(1) / case.std - 1).abs().max() < 0.5


@pytest.mark.parametrize('case', ec.ALL_CASES, ids=IDS)
def test_inputs_are_reproducible(case):
    x, dy = ec.make_input(case)
    ec.make_input.cache_clear()
    x2, dy2 = ec.make_input(case)
    assert torch.equal(x, x2) and torch.equal(dy, dy2)


@pytest.mark.parametrize('case', ec.ALL_CASES, ids=IDS)
def test_kept_and_dropped_planes(case):
    scale = ec.plane_scale(case, True)
    assert set(scale.tolist()) <= {0.0, torch.tensor(1.0 / (1.0 - ec.P)).item()}
    if case.num_planes >= 2:
        assert (scale == 0).any(), 'no dropped plane'
        assert (scale > 0).any(), 'no kept plane'
    assert torch.equal(ec.plane_scale(case, False), torch.ones(case.num_planes))


def test_tables_cover_every_instance():
    """Every register tile as float4 and as scalar, and the streaming kernel from both
    tables; each tier at its upper edge and just past it."""
    tiles = [(16, 1), (64, 1), (64, 3), (64, 9), (256, 9), (1024, 9)]
    for table, kind, step in ((ec.FLOAT4_TIERS, 'float4', 4), (ec.SCALAR_TIERS, 'scalar', 1)):
        got = [ec.instance(case.s) for case in table]
        for group, v in tiles:
            assert f'({group},{v})-{kind}' in got
        assert 'streaming' in got
        sizes = {case.s for case in table}
        for group, v in tiles:
            cap = group * v * 4
            below = cap if kind == 'float4' else cap - 1
            assert below in sizes and cap + step in sizes
    assert {case.planes for case in ec.TABLE if case.s <= 64} >= {(1, 17)}
    for case in ec.FLOAT4_TIERS + ec.SCALAR_TIERS:
        assert case.planes == ec.planes_for(case.s)
    assert [case.s for case in ec.ALIGNMENT] == [64, 576, 9216]
    assert all(ec.instance(case.s).endswith('float4') for case in ec.ALIGNMENT)
    assert [case.s for case in ec.LARGE_OFFSET] == [576, 36864]
    assert [len(case.shape) for case in ec.OTHER_RANKS] == [3, 5]
