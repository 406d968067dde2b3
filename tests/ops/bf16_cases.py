"""Inputs and case tables for the bf16 DropNormAct kernel tests (no tests here).

The bf16 instances of kernels K3 / K3b (``csrc/kernels.hip``) share the fp32 tile table: a
slot is 4 elements, so a bf16 lane's vector access is 8 bytes and the vector form needs
``S % 4 == 0`` and 8-byte aligned pointers.  :func:`instance` restates the dispatch
(``TGPIPE_DNA_DISPATCH`` and ``dna_vec_ok``); ``test_bf16_kernels_gpu.py`` checks the claim
against the host's own plan query (``torch.ops.tgpipe.dna_plan_info``).  Forward and
backward dispatch alike.

    tile (GROUP, V)   vector cases (first, last [, U-Net])   scalar case (last - 1)
    (16, 1)           vec-S4, vec-S64, vec-S36               scalar-S63
    (64, 1)           vec-S68, vec-S256, vec-S144            scalar-S255
    (64, 3)           vec-S260, vec-S768, vec-S576           scalar-S767
    (64, 9)           vec-S772, vec-S2304                    scalar-S2303
    (256, 9)          vec-S2308, vec-S9216                   scalar-S9215
    (1024, 9)         vec-S9220, vec-S36864                  scalar-S36863
    streaming         stream-S36865 (its first size, odd), stream-S36868

The U-Net plane sizes 36, 144, 576, 2304, 9216 and 36864 are all vector cases with whole
slots.  Every case has (2, 3) planes: 6 planes leave the last workgroup partial wherever a
workgroup holds 4 or 16 planes.  The ``ALIGNMENT`` cases run the scalar instances on
vector-sized planes through an ``x`` or ``dy`` that starts one element (2 bytes) off.

Preconditions, asserted on the CPU by ``test_bf16_cases.py`` (as ``epilogue_cases.py`` does
for fp32):

* the inputs are bf16 values (drawn from a CPU generator, rounded first);
* every fp64 pre-activation ``|z|`` of the upcast input is at least ``MARGIN``, at the eval
  scale and at the kept-plane dropout scale: elements too close to their plane's mean are
  pushed away and *re-rounded to bf16* until none is left, so no element is ever excluded
  from a comparison;
* each training case keeps one plane and drops one at ``p = 0.3`` (``PHILOX_PAIRS``).
"""
import functools
from typing import List, Tuple

import torch
from torch import Tensor

from tests.ops import epilogue_cases as ec
from tests.ops.epilogue_cases import EPS, MARGIN, P, PHILOX_PAIRS, SLOPE, Case  # noqa: F401

TILES = [(16, 1), (64, 1), (64, 3), (64, 9), (256, 9), (1024, 9)]
MAX_TILE = 1024 * 9 * 4
UNET_SIZES = [36, 144, 576, 2304, 9216, 36864]
PLANES = (2, 3)


def plan(s: int, aligned: bool = True) -> Tuple[int, int, int]:
    """``(GROUP, V, form)`` as ``dna_plan_info`` reports it: form 0 scalar, 1 vector,
    2 streaming (``aligned``: every pointer of the launch is 8-byte aligned)."""
    if s > MAX_TILE:
        return (1024, 0, 2)
    form = 1 if s % 4 == 0 and aligned else 0
    for group, v in TILES:
        if s <= group * v * 4:
            return (group, v, form)
    raise AssertionError(s)


def instance(s: int, aligned: bool = True) -> str:
    group, v, form = plan(s, aligned)
    if form == 2:
        return 'streaming'
    return f'({group},{v})-{"vec" if form else "scalar"}'


def _spatial(s: int) -> Tuple[int, int]:
    """A 2-D extent of ``s`` elements (square where ``s`` is one)."""
    root = int(round(s ** 0.5))
    if root * root == s:
        return (root, root)
    for h in (4, 3, 2):
        if s % h == 0:
            return (h, s // h)
    return (1, s)


def _cases(prefix: str, sizes: List[int], start: int) -> List[Case]:
    out = []
    for k, s in enumerate(sizes):
        seed, offset = PHILOX_PAIRS[(start + k) % len(PHILOX_PAIRS)]
        out.append(Case(f'{prefix}-S{s}', PLANES, _spatial(s), seed, offset))
    return out


_FIRST_LAST = [4, 64, 68, 256, 260, 768, 772, 2304, 2308, 9216, 9220, 36864]
VECTOR = _cases('vec', _FIRST_LAST + [s for s in UNET_SIZES if s not in _FIRST_LAST], 0)
SCALAR = _cases('scalar', [group * v * 4 - 1 for group, v in TILES], 3)
STREAMING = _cases('stream', [MAX_TILE + 1, MAX_TILE + 4], 5)
TABLE = VECTOR + SCALAR + STREAMING

# vector-sized planes for the misaligned-pointer runs (the scalar instance of the same tile)
ALIGNMENT = [
    Case('align-S64', PLANES, (8, 8), *PHILOX_PAIRS[5]),
    Case('align-S576', PLANES, (24, 24), *PHILOX_PAIRS[6]),
    Case('align-S9216', PLANES, (96, 96), *PHILOX_PAIRS[7]),
]
ISOLATION = [
    Case('isolate-S36', PLANES, (6, 6), *PHILOX_PAIRS[0]),
    Case('isolate-S576', PLANES, (24, 24), *PHILOX_PAIRS[2]),
]
ALL_CASES = TABLE + ALIGNMENT + ISOLATION


@functools.lru_cache(maxsize=None)
def make_input(case: Case) -> Tuple[Tensor, Tensor]:
    """``(x, dy)`` of ``case``: bf16 on the CPU, ``x`` with the LeakyReLU branch margin.
    Cached: treat both as read-only."""
    index = ALL_CASES.index(case)
    gen = torch.Generator().manual_seed(31000 + index)
    x = (torch.randn(case.shape, generator=gen) * case.std + case.mean).bfloat16()
    dy = torch.randn(case.shape, generator=gen).bfloat16()
    planes = case.num_planes
    flat = x.view(planes, -1)
    scales = (torch.ones(planes), torch.full((planes,), 1.0 / (1.0 - P)))
    for attempt in range(50):
        wide = flat.double()
        bad = torch.zeros_like(flat, dtype=torch.bool)
        for scale in scales:
            bad |= ec.preactivation(wide, scale).abs() < 1.5 * MARGIN
        if not bad.any():
            break
        # push away from the mean, farther every round: a bf16 step near the mean can be
        # larger than the margin, so the re-rounding may land an element inside it again
        mean = wide.mean(1, keepdim=True)
        std = wide.std(1, unbiased=False, keepdim=True)
        side = torch.where(wide >= mean, 1.0, -1.0)
        pushed = (mean + side * (3.0 + attempt) * MARGIN * std).bfloat16()
        flat[bad] = pushed.expand_as(flat)[bad]
    else:
        raise AssertionError(f'{case.name}: no LeakyReLU margin after 50 rounds')
    return x, dy


def reference(case: Case, x: Tensor, dy: Tensor, training: bool):
    """The fp64 composite on the upcast bf16 inputs (exact), and the fp32 composite on the
    same values, whose error against fp64 sizes the fp32 part of the bound:
    ``(y64, dx64, y32, dx32)``."""
    assert x.dtype == dy.dtype == torch.bfloat16
    return ec.reference(case, x.float(), dy.float(), training)
