"""The bf16 instances of the U-Net epilogue and resampling kernels (GPU only): DropNormAct
(``csrc/kernels.hip`` K3 / K3b), ``up2x_cat`` and ``MaxPool2x2`` (``csrc/unet_ops.hip``).

The oracle is the fp64 composite on the upcast bf16 inputs, which is exact; never the kernel
under test and never a bf16 composite.  Bound per element of ``y`` and ``dx``:

    |got - ref| <= 2^-8 * |ref| + tol_f32

``2^-8`` is the round-to-nearest half-ulp of bf16's 8-bit significand (the one rounding of
the store).  ``tol_f32`` is what the fp32 test of the same case allows against fp64
(``test_epilogue_kernels_gpu.py``): 8 x the largest error of the project's fp32 composite on
the same values, plus 1e-7 -- an f32 error can at most shift a value across a rounding
boundary by its own size.  The saved statistics are fp32 and held to the fp32 test's bound.
Run with ``-s`` to see every case's figures.
"""
import types

import pytest
import torch
import torch.nn.functional as F

from tests.ops import bf16_cases as bc
from tests.ops import epilogue_cases as ec
from torchgpipe_amd.ops import _ext, fused
from torchgpipe_amd.ops.fused import _signed64
from torchgpipe_amd.ops.unet_ops import MaxPool2x2, up2x_cat
from torchgpipe_amd.utils.rng import PhiloxSlot, slot_scope

pytestmark = pytest.mark.gpu

cuda = torch.device('cuda', 0)
BF16 = torch.bfloat16
HALF_ULP = 2.0 ** -8
FACTOR = 8.0
FLOOR = 1e-7


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


def ops():
    return torch.ops.tgpipe


def misaligned(t):
    """A contiguous GPU copy of ``t`` that starts one element past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=cuda)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == t.element_size()
    return view


def dna(case, training, x, dy):
    y, mean, rstd, scale = ops().dna_forward(x, bc.P, bc.EPS, bc.SLOPE, _signed64(case.seed),
                                             _signed64(case.offset), training, None)
    dx = ops().dna_backward(dy, x, mean, rstd, scale, bc.SLOPE)
    return y, dx, mean, rstd, scale


def within(label, name, got, want64, plain32):
    """``|got - want| <= 2^-8 |want| + tol_f32`` element by element; prints the figures."""
    assert got.dtype == BF16
    got = got.detach().double().cpu().reshape(want64.shape)
    tol = FACTOR * (plain32.detach().double().reshape(want64.shape) - want64).abs().max().item() \
        + FLOOR
    excess = ((got - want64).abs() - HALF_ULP * want64.abs()).max().item()
    print(f'bf16 DNA {label} {name}: max(|err| - 2^-8 |ref|) = {excess:.3e}, '
          f'tol_f32 = {tol:.3e}')
    return excess <= tol, f'{label} {name}: {excess:.3e} > {tol:.3e}'


def check_against_fp64(case, training, label, y, dx, mean, rstd, scale, x, dy):
    want_scale = ec.plane_scale(case, training)
    y64, dx64, y32, dx32 = bc.reference(case, x, dy, training)
    mean64, rstd64, mean32, rstd32 = ec.reference_stats(case, x.float(), training)
    label = f'{case.name} {"train" if training else "eval"} {label}'
    results = [within(label, 'y', y, y64, y32), within(label, 'dx', dx, dx64, dx32)]
    # the saved statistics stay fp32: the fp32 test's bound
    assert mean.dtype == rstd.dtype == scale.dtype == torch.float32
    for name, got, want, plain in (('mean', mean, mean64, mean32), ('rstd', rstd, rstd64, rstd32)):
        err = (got.double().cpu() - want).abs().max().item()
        tol = FACTOR * (plain.double() - want).abs().max().item() + FLOOR
        print(f'bf16 DNA {label} {name}: err = {err:.3e}, tol = {tol:.3e}')
        results.append((err <= tol, f'{label} {name}: {err:.3e} > {tol:.3e}'))
    assert torch.equal(scale.cpu(), want_scale)
    dropped = want_scale == 0
    planes = case.num_planes
    assert (y.cpu().view(planes, -1)[dropped] == 0).all()
    assert (dx.cpu().view(planes, -1)[dropped] == 0).all()
    for ok, message in results:
        assert ok, message


IDS = [c.name for c in bc.TABLE]


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('case', bc.TABLE, ids=IDS)
def test_drop_norm_act_matches_fp64(case, training):
    x, dy = bc.make_input(case)
    seed, offset = _signed64(case.seed), _signed64(case.offset)
    xg = x.to(cuda).requires_grad_(True)
    y = fused._DropNormAct.apply(xg, bc.P, bc.EPS, bc.SLOPE, seed, offset, training)
    assert y.dtype == BF16
    y.backward(dy.to(cuda))
    assert xg.grad.dtype == BF16
    _, mean, rstd, scale = ops().dna_forward(xg.detach(), bc.P, bc.EPS, bc.SLOPE, seed, offset,
                                             training, None)
    check_against_fp64(case, training, bc.instance(case.s), y.detach(), xg.grad, mean, rstd,
                       scale, x, dy)


def test_module_takes_bf16():
    """``DropNormAct`` on a bf16 tensor runs the kernel, in eval mode and with p = 0."""
    case = bc.VECTOR[-1]
    x = bc.make_input(case)[0].to(cuda)
    want = ops().dna_forward(x, 0.0, 1e-5, 1e-2, 0, 0, False, None)[0]
    for module in (fused.DropNormAct(p=0.0), fused.DropNormAct(p=0.3).eval()):
        y = module(x)
        assert y.dtype == BF16 and torch.equal(y, want)


@pytest.mark.parametrize('which', ['x', 'dy'])
@pytest.mark.parametrize('case', bc.ALIGNMENT, ids=[c.name for c in bc.ALIGNMENT])
def test_drop_norm_act_misaligned_pointer(case, which):
    """``x`` one element off: the scalar instance forward and backward on a plane size that
    otherwise takes the vector form.  Only ``dy`` off: vector forward, scalar backward."""
    x, dy = bc.make_input(case)
    xa, dya = x.to(cuda), dy.to(cuda)
    assert xa.data_ptr() % 16 == 0 and dya.data_ptr() % 16 == 0
    xk = misaligned(xa) if which == 'x' else xa
    dyk = misaligned(dya) if which == 'dy' else dya
    y, dx, mean, rstd, scale = dna(case, True, xk, dyk)
    label = f'{which}-misaligned {bc.instance(case.s, aligned=False)}'
    check_against_fp64(case, True, label, y, dx, mean, rstd, scale, x, dy)


@pytest.mark.parametrize('case', bc.ISOLATION, ids=[c.name for c in bc.ISOLATION])
def test_drop_norm_act_nan_stays_in_its_plane(case):
    x, dy = bc.make_input(case)
    planes, s = case.num_planes, case.s
    scale = ec.plane_scale(case, True)
    index = int(torch.nonzero(scale > 0)[0])
    x2, dy2 = x.clone(), dy.clone()
    x2.view(planes, s)[index, s // 2] = float('nan')
    dy2.view(planes, s)[index, 1] = float('nan')
    before = dna(case, True, x.to(cuda), dy.to(cuda))
    after = dna(case, True, x2.to(cuda), dy2.to(cuda))
    others = torch.arange(planes) != index
    for name, a, b in zip(('y', 'dx', 'mean', 'rstd', 'scale'), before, after):
        a, b = a.cpu().view(planes, -1), b.cpu().view(planes, -1)
        assert torch.equal(a[others], b[others]), f'{name} of another plane changed'
        assert torch.isfinite(a.float()).all()
    assert torch.isnan(after[0].cpu().view(planes, s)[index].float()).all()
    assert torch.isnan(after[1].cpu().view(planes, s)[index].float()).all()


def test_drop_norm_act_p_zero_keeps_every_plane():
    x = torch.randn(3, 7, 5, 5, device=cuda).bfloat16()
    for seed, offset in bc.PHILOX_PAIRS:
        scale = ops().dna_forward(x, 0.0, bc.EPS, bc.SLOPE, _signed64(seed), _signed64(offset),
                                  True, None)[3]
        assert torch.equal(scale, torch.ones(21, device=cuda))


@pytest.mark.parametrize('shape', [(0, 3, 4, 4), (2, 0, 4, 4), (2, 3, 0, 4)])
def test_drop_norm_act_empty(shape):
    """No planes, or planes without spatial extent: empty outputs, nothing launched."""
    x = torch.empty(shape, device=cuda, dtype=BF16, requires_grad=True)
    y = fused._DropNormAct.apply(x, bc.P, bc.EPS, bc.SLOPE, 1, 2, True)
    assert y.shape == x.shape and y.dtype == BF16
    y.backward(torch.empty_like(y))
    assert x.grad.shape == x.shape
    outs = ops().dna_forward(x.detach(), bc.P, bc.EPS, bc.SLOPE, 1, 2, True, None)
    planes = shape[0] * shape[1]
    assert [tuple(t.shape) for t in outs] == [shape, (planes,), (planes,), (planes,)]


@pytest.mark.parametrize('case', [bc.VECTOR[1], bc.SCALAR[2], bc.STREAMING[0]],
                         ids=lambda c: c.name)
def test_drop_norm_act_philox_slot(case):
    """rng = [seed, base] with the call's offset = delta draws what (seed, base + delta)
    draws, in the vector, scalar and streaming kernels."""
    x = bc.make_input(case)[0].to(cuda)
    delta = 5
    rng = torch.tensor([_signed64(case.seed), _signed64(case.offset) - delta],
                       dtype=torch.int64, device=cuda)
    want = ops().dna_forward(x, bc.P, bc.EPS, bc.SLOPE, _signed64(case.seed),
                             _signed64(case.offset), True, None)
    got = ops().dna_forward(x, bc.P, bc.EPS, bc.SLOPE, 0x5EEDBAD, delta, True, rng)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert (want[3] == 0).any() and (want[3] > 0).any()


def test_drop_norm_act_in_a_slot_scope():
    """``drop_norm_act`` inside a captured cell's slot scope no longer raises for bf16, and
    still does for a dtype the kernel does not take."""
    slots = torch.tensor([[12345, 64]], dtype=torch.int64, device=cuda)
    x = torch.randn(2, 3, 6, 6, device=cuda)
    with slot_scope(PhiloxSlot(slots[0])):
        y = fused.drop_norm_act(x.bfloat16(), 0.3)
    want = ops().dna_forward(x.bfloat16(), 0.3, 1e-5, 1e-2, 12345, 64, True, None)[0]
    assert torch.equal(y, want)
    with slot_scope(PhiloxSlot(slots[0])), pytest.raises(RuntimeError, match='Philox slot'):
        fused.drop_norm_act(x.half(), 0.3)


def test_backwards_cast_a_gradient_of_another_dtype():
    """The three Functions cast a ``dy`` whose dtype is not the forward's before the op sees
    it.  The autograd engine coerces gradients itself, so the cast is reached only through
    a direct ``backward`` call, as here."""
    from torchgpipe_amd.ops import unet_ops
    x = bc.make_input(bc.VECTOR[2])[0].to(cuda)              # (2, 3, 4, 17) bf16
    dy = bc.make_input(bc.VECTOR[2])[1].to(cuda)
    y, mean, rstd, scale = ops().dna_forward(x, 0.0, bc.EPS, bc.SLOPE, 0, 0, False, None)
    ctx = types.SimpleNamespace(saved_tensors=(x, mean, rstd, scale), slope=bc.SLOPE)
    want = ops().dna_backward(dy, x, mean, rstd, scale, bc.SLOPE)
    got = fused._DropNormAct.backward(ctx, dy.float())[0]
    assert got.dtype == BF16 and torch.equal(got, want)

    xp = _bf16((2, 3, 4, 6), 11).to(cuda)
    dp = _bf16((2, 3, 2, 3), 12).to(cuda)
    ctx = types.SimpleNamespace(saved_tensors=(xp,), has_add=True)
    dx, dadd = unet_ops._MaxPool2x2.backward(ctx, dp.float())
    assert dx.dtype == BF16 and torch.equal(dx, ops().maxpool2x2_backward(xp, dp))
    assert dadd.dtype == BF16 and torch.equal(dadd, dp)

    dcat = _bf16((2, 8, 4, 4), 13).to(cuda)
    ctx = types.SimpleNamespace(c1=3, dtype=BF16)
    dx, dskip = unet_ops._Up2xCat.backward(ctx, dcat.float())
    assert dx.dtype == BF16 and torch.equal(dx, ops().up2x_backward(dcat, 3))
    assert dskip.dtype == BF16 and torch.equal(dskip, dcat[:, 3:])


def test_every_case_reaches_its_instance():
    """The host's own plan for each case (``dna_plan_info``, the dispatch table and the
    vector condition of the launchers) is the instance the case table claims."""
    for case in bc.TABLE:
        assert tuple(ops().dna_plan_info(case.s, 2, 0)) == bc.plan(case.s), case.name
    for case in bc.ALIGNMENT:
        x = misaligned(bc.make_input(case)[0].to(cuda))
        assert tuple(ops().dna_plan_info(case.s, 2, x.data_ptr())) == \
            bc.plan(case.s, aligned=False), case.name
    # (8-byte slots: a pointer 8 bytes off a 16-byte boundary still takes the vector form)
    assert tuple(ops().dna_plan_info(64, 2, 8)) == (16, 1, 1)
    assert tuple(ops().dna_plan_info(64, 4, 8)) == (16, 1, 0)


# ---------------------------------------------------------------------------------------------
# up2x_cat
# ---------------------------------------------------------------------------------------------
def _bf16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


def _up2x_reference(x, skip, dy):
    """fp64: the block sums of ``dy``'s first channels and the sum of their magnitudes."""
    c1 = x.shape[1]
    g = dy[:, :c1].double()
    n, c, hh, ww = g.shape
    blocks = g.view(n, c, hh // 2, 2, ww // 2, 2)
    return blocks.sum((3, 5)), blocks.abs().sum((3, 5))


@pytest.mark.parametrize('shapes,off', [
    (((2, 3, 2, 2), (2, 5, 4, 4)), False), (((1, 1, 1, 1), (1, 1, 2, 2)), False),
    (((2, 3, 2, 2), (2, 5, 4, 4)), True)], ids=['2x3+5', '1x1+1', 'misaligned'])
def test_up2x_cat_bf16(shapes, off):
    x, skip = _bf16(shapes[0], 1), _bf16(shapes[1], 2)
    xg, sg = x.to(cuda), skip.to(cuda)
    if off:
        xg, sg = misaligned(xg), misaligned(sg)
    xg.requires_grad_(True)
    sg.requires_grad_(True)
    want = torch.cat((F.interpolate(x.to(cuda), scale_factor=2), skip.to(cuda)), 1)
    direct = ops().up2x_cat_forward(xg.detach(), sg.detach())
    assert direct.dtype == BF16 and torch.equal(direct, want)
    out = up2x_cat(xg, sg)
    assert out.dtype == BF16 and torch.equal(out, want)
    dy = _bf16(out.shape, 3)
    out.backward(dy.to(cuda))
    assert sg.grad.dtype == BF16 and torch.equal(sg.grad.cpu(), dy[:, shapes[0][1]:])
    ref, mass = _up2x_reference(x, skip, dy)
    err = (xg.grad.double().cpu() - ref).abs()
    bound = HALF_ULP * ref.abs() + 3 * 2.0 ** -24 * mass
    print(f'bf16 up2x dx: max err {err.max().item():.3e}')
    assert xg.grad.dtype == BF16 and (err <= bound).all()


def test_up2x_backward_reads_a_channel_slice():
    """The gradient as the first channels of a larger, 16-byte aligned tensor: read in
    place, the same result as from a dense copy."""
    big = _bf16((2, 8, 4, 4), 4).to(cuda)
    c = 3
    got = ops().up2x_backward(big, c)
    dense = ops().up2x_backward(big[:, :c].contiguous(), c)
    assert got.dtype == BF16 and torch.equal(got, dense)
    ref, mass = _up2x_reference(torch.empty(2, c, 2, 2), None, big.cpu())
    assert ((got.double().cpu() - ref).abs() <= HALF_ULP * ref.abs() + 3 * 2.0 ** -24 * mass).all()


# ---------------------------------------------------------------------------------------------
# MaxPool2x2
# ---------------------------------------------------------------------------------------------
def _pool_input():
    x = _bf16((2, 3, 7, 9), 5)
    x[0, 0, 0:2, 0:2] = 1.5                      # a four-way tie: the first wins
    x[0, 1, 2:4, 4:6] = torch.tensor([[1.0, 3.0], [3.0, 2.0]])   # two maxima
    x[1, 0, 0, 1] = float('nan')                 # a NaN window
    x[1, 1, 2:4, 2:4] = float('-inf')            # a window of -inf
    x[1, 2, 4, 6] = float('nan')
    x[1, 2, 5, 7] = float('nan')                 # two NaNs: the last wins
    return x


def test_maxpool2x2_bf16_matches_aten():
    x = _pool_input()
    xg = x.to(cuda).requires_grad_(True)
    xr = x.to(cuda).requires_grad_(True)
    y = MaxPool2x2()(xg)
    yr = F.max_pool2d(xr, 2, 2)
    assert y.dtype == BF16 and y.shape == (2, 3, 3, 4)
    torch.testing.assert_close(y, yr, rtol=0, atol=0, equal_nan=True)
    torch.testing.assert_close(ops().maxpool2x2_forward(x.to(cuda), None), yr.detach(), rtol=0,
                               atol=0, equal_nan=True)
    dy = _bf16(y.shape, 6).to(cuda)
    y.backward(dy)
    yr.backward(dy)
    assert xg.grad.dtype == BF16
    torch.testing.assert_close(xg.grad, xr.grad, rtol=0, atol=0, equal_nan=True)
    # odd H / W: the trailing row and column get no gradient
    assert (xg.grad[:, :, 6, :] == 0).all() and (xg.grad[:, :, :, 8] == 0).all()


def test_maxpool2x2_bf16_add_is_rounded_once():
    x = _pool_input()
    add = _bf16((2, 3, 3, 4), 7, scale=3.0)
    y = MaxPool2x2()(x.to(cuda), add.to(cuda))
    want = (F.max_pool2d(x.to(cuda), 2, 2).float() + add.to(cuda).float()).bfloat16()
    assert y.dtype == BF16
    torch.testing.assert_close(y, want, rtol=0, atol=0, equal_nan=True)
    xg = x.to(cuda).requires_grad_(True)
    ag = add.to(cuda).requires_grad_(True)
    dy = _bf16(y.shape, 8).to(cuda)
    MaxPool2x2()(xg, ag).backward(dy)
    assert torch.equal(ag.grad, dy)
    xr = x.to(cuda).requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(dy)
    torch.testing.assert_close(xg.grad, xr.grad, rtol=0, atol=0, equal_nan=True)


def test_maxpool2x2_fp32_still_takes_the_fp32_kernel():
    x = _pool_input().float()
    y = MaxPool2x2()(x.to(cuda))
    assert y.dtype == torch.float32
    torch.testing.assert_close(y, F.max_pool2d(x.to(cuda), 2, 2), rtol=0, atol=0,
                               equal_nan=True)
    # mixed dtypes are nobody's kernel: the composite
    mixed = MaxPool2x2()(x.to(cuda), torch.ones(2, 3, 3, 4, device=cuda, dtype=BF16))
    assert mixed.dtype == torch.float32
