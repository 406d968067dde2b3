"""Preconditions of the bf16 DropNormAct kernel tests (``bf16_cases.py``), on the CPU."""
import pytest
import torch

from tests.ops import bf16_cases as bc
from tests.ops import epilogue_cases as ec

IDS = [case.name for case in bc.ALL_CASES]


def test_case_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize('case', bc.ALL_CASES, ids=IDS)
def test_inputs_are_bf16_with_the_leaky_relu_margin(case):
    x, dy = bc.make_input(case)
    assert x.dtype == dy.dtype == torch.bfloat16 and x.shape == dy.shape == case.shape
    assert case.planes == (2, 3)
    assert torch.isfinite(x).all() and torch.isfinite(dy).all()
    for training in (False, True):
        margin = ec.min_margin(case, x.float(), training)
        print(f'{case.name} training={training}: min |z| = {margin:.3e}')
        assert margin >= bc.MARGIN
    flat = x.double().view(case.num_planes, -1)
    assert (flat.mean(1) - case.mean).abs().max() < 2.0 * case.std
    if case.s >= 36:
        assert (flat.std(1) / case.std - 1).abs().max() < 0.5


@pytest.mark.parametrize('case', bc.ALL_CASES, ids=IDS)
def test_inputs_are_reproducible(case):
    x, dy = bc.make_input(case)
    bc.make_input.cache_clear()
    x2, dy2 = bc.make_input(case)
    assert torch.equal(x, x2) and torch.equal(dy, dy2)


@pytest.mark.parametrize('case', bc.ALL_CASES, ids=IDS)
def test_kept_and_dropped_planes(case):
    scale = ec.plane_scale(case, True)
    assert (scale == 0).any(), 'no dropped plane'
    assert (scale > 0).any(), 'no kept plane'


def test_tables_cover_every_instance():
    """First and last size of every tile as a vector case, last - 1 as a scalar case, the
    streaming kernel's first size (odd) and first slot-sized one, and every U-Net plane as a
    whole-slot vector case."""
    vector = {case.s for case in bc.VECTOR}
    scalar = {case.s for case in bc.SCALAR}
    first = 4
    for group, v in bc.TILES:
        cap = group * v * 4
        assert {first, cap} <= vector and cap - 1 in scalar
        assert bc.plan(first) == bc.plan(cap) == (group, v, 1)
        assert bc.plan(cap - 1) == (group, v, 0)
        first = cap + 4
    assert [case.s for case in bc.STREAMING] == [bc.MAX_TILE + 1, bc.MAX_TILE + 4]
    assert bc.plan(bc.MAX_TILE + 1)[2] == bc.plan(bc.MAX_TILE + 4)[2] == 2
    assert bc.plan(bc.MAX_TILE)[2] == 1
    for s in bc.UNET_SIZES:
        assert s in vector and s % 4 == 0 and bc.plan(s)[2] == 1
    assert [case.s for case in bc.ALIGNMENT] == [64, 576, 9216]
    for case in bc.ALIGNMENT:
        assert bc.plan(case.s)[2] == 1 and bc.plan(case.s, aligned=False)[2] == 0
