"""Inputs and case tables for the DropNormAct edge tests (no tests here).

Everything is drawn from a CPU generator, so a case is the same tensor on every machine.
``test_epilogue_cases.py`` asserts, without a GPU, the two preconditions the GPU tests in
``test_epilogue_kernels_gpu.py`` rely on:

* **LeakyReLU branch margin.**  The kernel picks the LeakyReLU branch by ``z > 0`` in fp32.
  Where the fp64 pre-activation is within fp32 rounding of 0 the two precisions take
  different branches and ``dx`` differs by ``0.99 * g * rstd``: no kernel error, but no
  tolerance survives it either.  :func:`make_input` therefore pushes every element whose
  fp64 ``|z|`` is below :data:`MARGIN` away from its plane's mean until none is left (in
  eval mode and with the kept-plane dropout scale).  1e-3 is over 100x the fp32 error of
  ``z`` (at most 6.4e-6, on the planes whose mean is 100 standard deviations).
* **Kept and dropped planes.**  ``(seed, offset)`` of every training case with at least two
  planes keeps one plane and drops one at ``p = 0.3`` (found by a CPU search with
  ``fused.plane_scale_reference``; all of :data:`PHILOX_PAIRS` differ in planes 0 and 1).

Which kernel instance a case runs follows from ``TGPIPE_DNA_DISPATCH`` and the ``vec``
condition of ``launch_dna_forward`` / ``launch_dna_backward`` (``csrc/kernels.hip``):
:func:`instance` restates it, for the test ids and the reader.  Forward and backward
dispatch alike, so one case runs the same instance of both:

    tile (GROUP, V)   float4 cases            scalar cases
    (16, 1)           float4-S64              scalar-S63
    (64, 1)           float4-S68, -S256       scalar-S65, -S255
    (64, 3)           float4-S260, -S768      scalar-S257, -S767
    (64, 9)           float4-S772, -S2304     scalar-S769, -S2303
    (256, 9)          float4-S2308, -S9216    scalar-S2305, -S9215
    (1024, 9)         float4-S9220, -S36864   scalar-S9217, -S36863
    streaming         float4-S36868           scalar-S36865

The ``ALIGNMENT`` cases run the scalar instances of (16, 1), (64, 3) and (256, 9) on
float4-sized planes through a misaligned ``x`` (forward and backward) or ``dy`` (float4
forward, scalar backward).
"""
import functools
from typing import NamedTuple, Tuple

import torch
from torch import Tensor
import torch.nn.functional as F

from torchgpipe_amd.ops import fused

P = 0.3
EPS = 1e-5
SLOPE = 1e-2
MARGIN = 1e-3

# (seed, offset): plane 0 and plane 1 get different fates at p = 0.3 under each of them
PHILOX_PAIRS = [
    (987654321, 64),
    (987654321, 2 ** 33),
    (2 ** 40 + 3, 64),
    (2 ** 63 + 11, 5),
    (12345, 0),
    (42, 16),
    (7, 0),
    (42, 2 ** 32 - 3),
]


class Case(NamedTuple):
    name: str
    planes: Tuple[int, int]        # (n, c)
    spatial: Tuple[int, ...]
    seed: int
    offset: int
    mean: float = 1.0              # the planes' offset ...
    std: float = 3.0               # ... and spread: x = randn * std + mean

    @property
    def shape(self) -> Tuple[int, ...]:
        return self.planes + self.spatial

    @property
    def s(self) -> int:
        out = 1
        for d in self.spatial:
            out *= d
        return out

    @property
    def num_planes(self) -> int:
        return self.planes[0] * self.planes[1]


def planes_for(s: int) -> Tuple[int, int]:
    """A plane count that leaves the last workgroup partial (idle groups): 16 planes share
    a workgroup up to S = 64, 4 up to S = 2304, one above."""
    if s <= 64:
        return (1, 17)
    if s <= 2304:
        return (1, 5)
    return (1, 2)


def instance(s: int, aligned: bool = True) -> str:
    """The kernel instance ``launch_dna_forward`` / ``launch_dna_backward`` pick for plane
    size ``s`` (``aligned``: every pointer of the launch is 16-byte aligned)."""
    if s > 1024 * 9 * 4:
        return 'streaming'
    kind = 'float4' if s % 4 == 0 and aligned else 'scalar'
    for group, v in ((16, 1), (64, 1), (64, 3), (64, 9), (256, 9), (1024, 9)):
        if s <= group * v * 4:
            return f'({group},{v})-{kind}'
    raise AssertionError(s)


def _tier_cases(prefix: str, spatials) -> list:
    cases = []
    for k, spatial in enumerate(spatials):
        s = spatial[0] * spatial[1]
        seed, offset = PHILOX_PAIRS[k % len(PHILOX_PAIRS)]
        cases.append(Case(f'{prefix}-S{s}', planes_for(s), spatial, seed, offset))
    return cases


# Both edges of every tier: S = 4 * GROUP * V and the next size the same path takes.
FLOAT4_TIERS = _tier_cases('float4', [
    (8, 8), (4, 17), (16, 16), (4, 65), (24, 32), (4, 193), (48, 48), (4, 577), (96, 96),
    (4, 2305), (192, 192), (4, 9217)])          # S = 36868: the streaming kernel
SCALAR_TIERS = _tier_cases('scalar', [
    (7, 9), (5, 13), (15, 17), (1, 257), (13, 59), (1, 769), (47, 49), (5, 461), (97, 95),
    (13, 709), (193, 191), (5, 7373)])          # S = 36865: the streaming kernel
SINGLE_PLANE = [Case('single-plane-S144', (1, 1), (12, 12), *PHILOX_PAIRS[1])]   # (kept)
OTHER_RANKS = [
    Case('rank3-S40', (2, 3), (40,), *PHILOX_PAIRS[1]),
    Case('rank5-S120', (2, 3), (4, 5, 6), *PHILOX_PAIRS[2]),
]
# mean = 100 sigma: E[x^2] - mean^2 loses seven digits here, the two-pass variance none
LARGE_OFFSET = [
    Case('offset100-S576', (1, 5), (24, 24), *PHILOX_PAIRS[3], mean=100.0, std=1.0),
    Case('offset100-S36864', (1, 2), (192, 192), *PHILOX_PAIRS[4], mean=100.0, std=1.0),
]
TABLE = FLOAT4_TIERS + SCALAR_TIERS + SINGLE_PLANE + OTHER_RANKS + LARGE_OFFSET

# float4-sized planes for the misaligned-pointer runs (the scalar instance of the same tile)
ALIGNMENT = [
    Case('align-S64', (1, 17), (8, 8), *PHILOX_PAIRS[5]),
    Case('align-S576', (1, 5), (24, 24), *PHILOX_PAIRS[6]),
    Case('align-S9216', (1, 2), (96, 96), *PHILOX_PAIRS[7]),
]
ISOLATION = [
    Case('isolate-S36', (1, 17), (6, 6), *PHILOX_PAIRS[0]),
    Case('isolate-S576', (1, 5), (24, 24), *PHILOX_PAIRS[2]),
]
ALL_CASES = TABLE + ALIGNMENT + ISOLATION


def plane_scale(case: Case, training: bool) -> Tensor:
    """fp32 per-plane dropout scale of ``case`` (all ones in eval mode)."""
    if not training:
        return torch.ones(case.num_planes)
    return fused.plane_scale_reference(case.num_planes, P, case.seed, case.offset,
                                       torch.device('cpu'))


def preactivation(x: Tensor, scale: Tensor) -> Tensor:
    """fp64 ``instance_norm(x * scale)`` as ``[planes, S]``, before the LeakyReLU."""
    planes = scale.numel()
    d = x.double().reshape(planes, -1) * scale.double().view(-1, 1)
    mean = d.mean(1, keepdim=True)
    var = d.var(1, unbiased=False, keepdim=True)
    return (d - mean) / torch.sqrt(var + EPS)


def min_margin(case: Case, x: Tensor, training: bool) -> float:
    """Smallest fp64 ``|z|`` over the planes ``training`` keeps (a dropped plane's z is 0
    in every precision: the tests want exact zeros there)."""
    scale = plane_scale(case, training)
    z = preactivation(x, scale).abs()
    kept = scale > 0
    return z[kept].min().item() if kept.any() else float('inf')


@functools.lru_cache(maxsize=None)
def make_input(case: Case) -> Tuple[Tensor, Tensor]:
    """``(x, dy)`` of ``case``, fp32 on the CPU, ``x`` with the LeakyReLU branch margin.
    Cached: treat both as read-only."""
    index = ALL_CASES.index(case)
    gen = torch.Generator().manual_seed(20240 + index)
    x = torch.randn(case.shape, generator=gen) * case.std + case.mean
    dy = torch.randn(case.shape, generator=gen)
    planes = case.num_planes
    flat = x.view(planes, -1)
    # the margin has to hold at both scales a plane can be normalised at
    scales = (torch.ones(planes), torch.full((planes,), 1.0 / (1.0 - P)))
    for _ in range(50):
        bad = torch.zeros_like(flat, dtype=torch.bool)
        for scale in scales:
            bad |= preactivation(flat, scale).abs() < 1.5 * MARGIN
        if not bad.any():
            break
        wide = flat.double()
        mean = wide.mean(1, keepdim=True)
        std = wide.std(1, unbiased=False, keepdim=True)
        side = torch.where(wide >= mean, 1.0, -1.0)
        pushed = (mean + side * 3.0 * MARGIN * std).float()
        flat[bad] = pushed.expand_as(flat)[bad]
    else:
        raise AssertionError(f'{case.name}: no LeakyReLU margin after 50 rounds')
    return x, dy


def reference(case: Case, x: Tensor, dy: Tensor, training: bool):
    """The fp64 oracle (Philox plane scale, ``F.instance_norm``, ``F.leaky_relu``) and the
    project's fp32 composite on the same CPU inputs, with their input gradients:
    ``(y64, dx64, y32, dx32)``."""
    n, c = case.planes
    ones = [1] * len(case.spatial)
    x64 = x.detach().double().requires_grad_(True)
    d = x64 * plane_scale(case, training).double().view(n, c, *ones) if training else x64
    y64 = F.leaky_relu(F.instance_norm(d, eps=EPS), SLOPE)
    y64.backward(dy.double())
    x32 = x.detach().clone().requires_grad_(True)
    y32 = fused._composite(x32, P, EPS, SLOPE, case.seed, case.offset, training)
    y32.backward(dy)
    return y64.detach(), x64.grad, y32.detach(), x32.grad


def reference_stats(case: Case, x: Tensor, training: bool):
    """Saved statistics: fp64 and plain fp32 ``(mean, rstd)`` of the *undropped* ``x``, with
    ``rstd = (scale^2 * var + eps)^-1/2``: ``(mean64, rstd64, mean32, rstd32)``."""
    scale = plane_scale(case, training)
    flat = x.reshape(case.num_planes, -1)
    wide = flat.double()
    mean64 = wide.mean(1)
    rstd64 = (scale.double() ** 2 * wide.var(1, unbiased=False) + EPS) ** -0.5
    mean32 = flat.mean(1)
    rstd32 = (scale ** 2 * flat.var(1, unbiased=False) + EPS) ** -0.5
    return mean64, rstd64, mean32, rstd32
