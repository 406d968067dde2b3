"""The conv precision levels on the GPU (ops/precision.py; csrc/conv_gemm.hip CFG 7-11 and
csrc/winograd_f4.hip bg_gemm_emu_kernel): every split-bf16 kernel against the fp64 oracle of
the level's partial products, the proof that the knob acts (the distance from the exact
result), `highest` untouched, and the fused ops that inherit the level."""
import copy

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from torchgpipe_amd.ops import _ext, convbn, fusion, precision
from torchgpipe_amd.ops.precision import (reference_conv2d, reference_conv2d_backward,
                                          split_bf16)

pytestmark = pytest.mark.gpu

REDUCED = ('high', 'medium')
EMU_CFGS = [7, 8, 9, 10, 11]


@pytest.fixture(autouse=True)
def need_gpu_and_restore():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), _ext.load_error()
    assert precision.get_conv_precision() == 'highest'
    try:
        yield
    finally:
        precision.set_conv_precision('highest')
        ops().conv_gemm_force_cfg(-1)
        ops().conv_gemm_presplit(-1)


def ops():
    return torch.ops.tgpipe


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# (n, ci, h, w, co, kh, kw, stride, pad, offset, forced splits): one staging path each
# (tests/ops/test_convbn_gpu.py::CASES)
CASES = [
    (4, 32, 28, 28, 48, 1, 1, 1, 0, 0, 1),      # quad path
    (5, 24, 7, 7, 40, 1, 1, 1, 0, 0, 1),        # scalar path, K not a multiple of 16
    (3, 16, 14, 14, 20, 1, 7, 1, 3, 0, 1),      # 1x7: gathered operand
    (2, 24, 15, 15, 16, 1, 1, 2, 0, 1, 1),      # strided 1x1 reading the shifted input
    (4, 1024, 7, 7, 256, 1, 1, 1, 0, 0, 4),     # split reduction
    (2, 3, 32, 32, 16, 3, 3, 1, 1, 0, 1),       # K = 27
    (3, 16, 15, 15, 24, 3, 3, 2, 1, 0, 1),      # stride-phase backward-data (in-kernel split)
]
CASE_IDS = [f'{c[5]}x{c[6]}s{c[7]}o{c[9]}_{c[0]}x{c[1]}x{c[2]}' for c in CASES]
_DATA = {}  # case index -> (x, w, dz, geo, stride, padding, offset), built once
_REFS = {}  # (case index, relu, level) -> (z, dx, dw) in fp64, computed once


@pytest.fixture(scope='module', autouse=True)
def release_shared_tensors():
    yield
    _DATA.clear()
    _REFS.clear()


def _shift(x, offset):
    return F.pad(x[:, :, offset:, offset:], (0, offset, 0, offset)) if offset else x


def _data(k):
    if k not in _DATA:
        n, ci, h, w, co, kh, kw, stride, pad, offset, _ = CASES[k]
        torch.manual_seed(k)
        x = torch.randn(n, ci, h, w, device='cuda')
        wt = torch.randn(co, ci, kh, kw, device='cuda') / (ci * kh * kw) ** 0.5
        padding = (pad if kh > 1 else 0, pad if kw > 1 else 0)
        geo = [kh, kw, stride, stride, padding[0], padding[1], offset, offset]
        z = F.conv2d(_shift(x, offset), wt, stride=stride, padding=padding)
        dz = torch.randn_like(z)
        _DATA[k] = (x, wt, dz, geo, stride, padding, offset)
    return _DATA[k]


def _refs(k, relu, level):
    """(z, dx, dw) of case k in fp64 with the partial products of `level`."""
    key = (k, relu, level)
    if key not in _REFS:
        x, wt, dz, _, stride, padding, offset = _data(k)
        xs = _shift(x, offset)  # (the shift commutes with the ReLU and with the split)
        z = reference_conv2d(xs, wt, stride, padding, level, relu)
        dxs, dw = reference_conv2d_backward(dz, xs, wt, stride, padding, level, relu)
        dx = F.pad(dxs[:, :, :x.shape[2] - offset, :x.shape[3] - offset],
                   (offset, 0, offset, 0)) if offset else dxs
        _REFS[key] = (z, dx, dw)
    return _REFS[key]


def _run(k, relu, x=None, wt=None, dz=None):
    x0, w0, dz0, geo = _data(k)[:4]
    x = x0 if x is None else x
    wt = w0 if wt is None else wt
    dz = dz0 if dz is None else dz
    z = ops().conv_gemm_forward(x, wt, geo, relu)
    dx = ops().conv_gemm_backward_data(dz, x, wt, geo, relu)
    dw = ops().conv_gemm_backward_weight(dz, x, wt, geo, relu)
    return z, dx, dw


@pytest.mark.parametrize('level', REDUCED)
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'plain'])
@pytest.mark.parametrize('presplit', [False, True], ids=['kernel-split', 'pre-split'])
@pytest.mark.parametrize('cfg', EMU_CFGS)
@pytest.mark.parametrize('k', range(len(CASES)), ids=CASE_IDS)
def test_split_bf16_gemm_computes_the_products_of_the_level(k, cfg, presplit, relu, level):
    """Forward, backward-data and weight gradient of every split-bf16 tile configuration hold
    the f32 bounds of tests/ops/test_convbn_gpu.py against the oracle of the level (what
    remains is the f32 accumulation), and lie where the level puts them from the exact
    result: beyond 3e-6 at `high`, beyond 1e-3 at `medium` (the kernels at `highest` are
    within 2e-6)."""
    ops().conv_gemm_force_cfg(cfg, CASES[k][10])
    ops().conv_gemm_presplit(-1 if presplit else 0)
    want = _refs(k, relu, level)
    exact = _refs(k, relu, 'highest')
    with precision.conv_precision(level):
        got = _run(k, relu)
    if presplit:
        assert ops().conv_gemm_presplit(-1, False) > 0  # the forward ran on the cached planes
    err = [rel_err(g, w) for g, w in zip(got, want)]
    away = [rel_err(g, e) for g, e in zip(got, exact)]
    print(f'{CASE_IDS[k]} cfg{cfg} presplit={presplit} relu={relu} {level}: '
          f'vs level z {err[0]:.2e} dx {err[1]:.2e} dw {err[2]:.2e}; '
          f'vs exact z {away[0]:.2e} dx {away[1]:.2e} dw {away[2]:.2e}')
    assert got[0].shape == want[0].shape
    assert err[0] < 2e-6
    assert err[1] < 2e-6
    assert err[2] < 5e-6
    floor = 3e-6 if level == 'high' else 1e-3
    assert away[0] > floor
    assert away[1] > floor
    if level == 'medium':
        assert away[2] > 1e-3


@pytest.mark.parametrize('cfg', EMU_CFGS)
@pytest.mark.parametrize('k', [0, 4, 6], ids=[CASE_IDS[0], CASE_IDS[4], CASE_IDS[6]])
def test_highest_set_explicitly_is_bit_identical_to_the_default(k, cfg):
    ops().conv_gemm_force_cfg(cfg, CASES[k][10])
    default = _run(k, True)
    with precision.conv_precision('medium'):
        other = _run(k, True)
    precision.set_conv_precision('highest')
    again = _run(k, True)
    for a, b, c in zip(default, again, other):
        assert torch.equal(a, b)
        assert not torch.equal(a, c)


@pytest.mark.parametrize('presplit', [False, True], ids=['kernel-split', 'pre-split'])
@pytest.mark.parametrize('cfg', EMU_CFGS)
@pytest.mark.parametrize('k', range(len(CASES)), ids=CASE_IDS)
def test_medium_is_highest_on_the_hi_parts(k, cfg, presplit):
    """`medium` on (x, w, dz) runs the one product that `highest` has left on their hi parts
    (the other five are exact zeros there, added first), under the same plan: bit-identical."""
    ops().conv_gemm_force_cfg(cfg, CASES[k][10])
    ops().conv_gemm_presplit(-1 if presplit else 0)
    x, wt, dz = _data(k)[:3]
    with precision.conv_precision('medium'):
        got = _run(k, True)
    hi = _run(k, True, split_bf16(x)[0], split_bf16(wt)[0], split_bf16(dz)[0])
    for a, b in zip(got, hi):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


# -- the fused ops inherit the level ---------------------------------------------------------

def _init_bn(bn):
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    return bn


def _emulated_step(x, convs, bns, adds, grads, level):
    """One training step of [bn_i(conv_i(relu(x))) (+ add_i)] in fp64 with the convolutions'
    products at `level`: the outputs, dx, and per operation (dW, dgamma, dbeta, the updated
    BatchNorm)."""
    ys, dx, per_op = [], 0, []
    for conv, bn, add, g in zip(convs, bns, adds, grads):
        z = reference_conv2d(x, conv.weight, conv.stride, conv.padding, level, relu=True)
        z.requires_grad_(True)
        b64 = copy.deepcopy(bn).double()
        y = b64(z)
        if add is not None:
            y = y + add.detach().double()
        y.backward(g.double())
        # the backward GEMMs split the fp32 gradient the BatchNorm backward hands them
        dxi, dw = reference_conv2d_backward(z.grad.float(), x, conv.weight, conv.stride,
                                            conv.padding, level, relu=True)
        dx = dx + dxi
        ys.append(y.detach())
        per_op.append((dw, b64.weight.grad, b64.bias.grad, b64))
    return ys, dx, per_op


def _check_step(x, convs, bns, ys, per_op_want, dx_want, ys_want):
    print('y', ' '.join(f'{rel_err(y, want):.2e}' for y, want in zip(ys, ys_want)),
          f'dx {rel_err(x.grad, dx_want):.2e}', 'dW / dgamma / dbeta / mean / var',
          ' '.join(f'{rel_err(c.weight.grad, dw):.2e} {rel_err(b.weight.grad, dg):.2e} '
                   f'{rel_err(b.bias.grad, db):.2e} {rel_err(b.running_mean, q.running_mean):.2e}'
                   f' {rel_err(b.running_var, q.running_var):.2e};'
                   for c, b, (dw, dg, db, q) in zip(convs, bns, per_op_want)))
    for y, want in zip(ys, ys_want):
        assert rel_err(y, want) < 1e-5
    assert rel_err(x.grad, dx_want) < 1e-5
    for conv, bn, (dw, dgamma, dbeta, b64) in zip(convs, bns, per_op_want):
        assert rel_err(conv.weight.grad, dw) < 1e-5
        assert rel_err(bn.weight.grad, dgamma) < 1e-5
        assert rel_err(bn.bias.grad, dbeta) < 1e-5
        assert rel_err(bn.running_mean, b64.running_mean) < 1e-6
        assert rel_err(bn.running_var, b64.running_var) < 1e-6
        assert bn.num_batches_tracked.item() == b64.num_batches_tracked.item() == 1


@pytest.mark.parametrize('level', REDUCED)
@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'node-sum'])
def test_fused_relu_conv_bn_training_step_at_a_reduced_level(with_add, level):
    """relu_conv_bn (1x1, 32 -> 48 at 14^2): y, dx, dW, dgamma, dbeta and the running
    statistics against the fp64 emulation of the level, at the tolerances of
    test_fused_relu_conv_bn_matches_fp64_training_step."""
    torch.manual_seed(1)
    ops().conv_gemm_force_cfg(7)
    conv = nn.Conv2d(32, 48, 1, bias=False).cuda()
    bn = _init_bn(nn.BatchNorm2d(48).cuda())
    x = torch.randn(6, 32, 14, 14, device='cuda', requires_grad=True)
    add = torch.randn(6, 48, 14, 14, device='cuda', requires_grad=True) if with_add else None
    g = torch.randn(6, 48, 14, 14, device='cuda')
    ys_want, dx_want, per_op = _emulated_step(x.detach(), [conv], [bn], [add], [g], level)
    with precision.conv_precision(level):
        y = convbn.relu_conv_bn(x, [(conv, 0)], bn, relu=True, add=add)
        y.backward(g)
    if with_add:
        assert torch.equal(add.grad, g)
    _check_step(x, [conv], [bn], [y], per_op, dx_want, ys_want)


@pytest.mark.parametrize('level', REDUCED)
def test_grouped_training_step_at_a_reduced_level(level):
    """The grouped op on a small shape: three column blocks with a ragged last one, K below
    one stage.  Small on purpose: the backward GEMMs split the BatchNorm backward's fp32 dZ,
    which differs from the oracle's by its rounding (1e-7), and at `medium` ONE element of dZ
    whose hi part rounds to the other bf16 neighbour moves dX by 2^-8 / sqrt(dZ.numel()) --
    1.2e-5 on the 6 x 96 x 14^2 of tests/ops/test_group_convbn_gpu.py, where a handful of
    elements do (3.2e-5 measured): beyond the 1e-5 this test holds the op to.  On 1800
    elements none does."""
    torch.manual_seed(0)
    ops().conv_gemm_force_cfg(7)
    n, ci, hw, cos = 3, 24, 5, (8, 16)
    convs = [nn.Conv2d(ci, co, 1, bias=False).cuda() for co in cos]
    bns = [_init_bn(nn.BatchNorm2d(co).cuda()) for co in cos]
    triplets = [(True, c, b) for c, b in zip(convs, bns)]
    x = torch.randn(n, ci, hw, hw, device='cuda', requires_grad=True)
    grads = [torch.randn(n, co, hw, hw, device='cuda') for co in cos]
    ys_want, dx_want, per_op = _emulated_step(x.detach(), convs, bns, [None] * len(cos), grads,
                                              level)
    assert convbn.groupable(x, triplets)
    with precision.conv_precision(level):
        ys = convbn.group_relu_conv_bn(x, triplets, convbn._GroupCache())
        sum((y * g).sum() for y, g in zip(ys, grads)).backward()
    _check_step(x, convs, bns, ys, per_op, dx_want, ys_want)


@pytest.mark.parametrize('level', REDUCED)
@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'add'])
def test_conv_bn_eval_at_a_reduced_level(with_add, level):
    torch.manual_seed(2)
    ops().conv_gemm_force_cfg(7)
    conv = nn.Conv2d(32, 48, 1, bias=False).cuda()
    bn = _init_bn(nn.BatchNorm2d(48).cuda())
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.5, 2)
    bn.eval()
    x = torch.randn(6, 32, 14, 14, device='cuda')
    add = torch.randn(6, 48, 14, 14, device='cuda') if with_add else None
    with torch.no_grad():
        z = reference_conv2d(x, conv.weight, 1, 0, level, relu=True)
        want = copy.deepcopy(bn).double()(z)
        want = F.relu(want + add.double() if with_add else want)
        exact = F.relu(copy.deepcopy(bn).double()(reference_conv2d(x, conv.weight, 1, 0,
                                                                   'highest', relu=True))
                       + (add.double() if with_add else 0))
        assert convbn.eval_fusable(x, [conv], bn, add)
        with precision.conv_precision(level):
            got = convbn.conv_bn_eval(x, [(conv, 0)], bn, relu=True, add=add, relu_out=True)
    assert rel_err(got, want) < 1e-5
    if level == 'medium':
        # the level reached the eval op: z is 2e-3 from exact there, and the folded BatchNorm
        # (scales of 0.35 .. 2.1) and the ReLU leave that within a factor of 20
        assert rel_err(got, exact) > 1e-4


def test_context_manager_changes_a_linked_layer_and_restores_the_level():
    torch.manual_seed(3)
    ops().conv_gemm_force_cfg(7)
    seq = nn.Sequential(fusion.ConvBN2d(32, 48, 1, bias=False), fusion.BatchNormAct2d(48),
                        fusion.ReLU()).cuda()
    assert fusion.relink(seq) == 1
    x = torch.randn(4, 32, 14, 14, device='cuda')
    with torch.no_grad():
        plain = seq(x)
        with precision.conv_precision('medium'):
            assert precision.get_conv_precision() == 'medium'
            assert ops().conv_precision() == 2
            reduced = seq(x)
        assert precision.get_conv_precision() == 'highest'
        assert ops().conv_precision() == 0
        again = seq(x)
    assert torch.equal(plain, again)
    assert not torch.equal(plain, reduced)
    assert rel_err(reduced, plain) > 1e-4  # (2e-3 on z, through the BatchNorm and the ReLU)


# -- batched-GEMM Winograd --------------------------------------------------------------------

_MATS = {
    4: ([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
         [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
        [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
         [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
        [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
    2: ([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
        [[1, 0, 0], [1 / 2, 1 / 2, 1 / 2], [1 / 2, -1 / 2, 1 / 2], [0, 0, 1]],
        [[1, 1, 1, 0], [0, 1, -1, -1]]),
}


def _mats(kind, device):
    return [torch.tensor(m, dtype=torch.float64, device=device) for m in _MATS[kind]]


def _three_products(eq, a, b, level):
    """einsum over the fp32 operands a, b: exact, or the three `high` products."""
    if level == 'highest':
        return torch.einsum(eq, a.double(), b.double())
    ah, am, _ = split_bf16(a)
    bh, bm, _ = split_bf16(b)
    return (torch.einsum(eq, ah.double() + am.double(), bh.double())
            + torch.einsum(eq, ah.double(), bm.double()))


def _patches(x, kind):
    m = kind
    n, c, h, wd = x.shape
    th, tw = -(-h // m), -(-wd // m)
    xp = F.pad(x.double(), (1, m * tw + 1 - wd, 1, m * th + 1 - h))
    return xp.unfold(2, m + 2, m).unfold(3, m + 2, m), th, tw      # n c th tw a a


def wino_conv_emulated(x, w, kind, level):
    """tests/ops/test_winograd_f4_ref.py::f4_conv (and its F(2x2) twin) with the kernel's
    roundings: transforms in fp64, U and V rounded to fp32, split, the products of the
    level, output transform."""
    bt, g, at = _mats(kind, x.device)
    n, _, h, wd = x.shape
    d, th, tw = _patches(x, kind)
    v = torch.einsum('ia,nctwab,jb->nctwij', bt, d, bt).float()
    u = torch.einsum('ia,kcab,jb->kcij', g, w.double(), g).float()
    m = _three_products('kcij,nctwij->nktwij', u, v, level)
    y = torch.einsum('pi,nktwij,qj->nktwpq', at, m, at)
    y = y.permute(0, 1, 2, 4, 3, 5).reshape(n, w.shape[0], kind * th, kind * tw)
    return y[:, :, :h, :wd]


def wino_wgrad_emulated(x, dy, level):
    """F(4x4) weight gradient: dW = G^T [sum over tiles (A dy A^T) . (B^T d B)] G."""
    bt, g, at = _mats(4, x.device)
    n, _, h, wd = x.shape
    d, th, tw = _patches(x, 4)
    v = torch.einsum('ia,nctwab,jb->nctwij', bt, d, bt).float()
    dyp = F.pad(dy.double(), (0, 4 * tw - wd, 0, 4 * th - h))
    t = dyp.unfold(2, 4, 4).unfold(3, 4, 4)                          # n k th tw 4 4
    dm = torch.einsum('pi,nktwpq,qj->nktwij', at, t, at).float()
    du = _three_products('nktwij,nctwij->kcij', dm, v, level)
    return torch.einsum('ia,kcij,jb->kcab', g, du, g)


def _dyadic(shape, step, bound, gen):
    """Multiples of `step` (a power of two times an odd constant) up to `bound` steps: few
    significant bits, so that the Winograd transforms of these tensors are exact in fp32."""
    return torch.randint(-bound, bound + 1, shape, device='cuda', generator=gen).float() * step


def _wino_inputs(hw, seed):
    """x, dy, w on grids that make the transforms exact in fp32: x and dy of 10 bits (the
    integer matrices B^T . B and A . A^T add 11 and 9: all three bf16 parts are in use), w
    multiples of 24 / 65536 (G's 1/4 .. 1/24 turn them into integers over 65536).  The
    kernels' fp32 transforms and the oracle's fp64 ones then give the same V and A dy A^T
    bit for bit, U up to the fused multiply-adds of cancelling terms, and the split sees
    the same numbers.  With randn inputs the operands differ by an fp32 rounding, in a few of
    them a part rounds to its other bf16 neighbour, and the products a level leaves out --
    amplified 40-fold at the weight gradient's corner taps -- then differ by 3x this test's
    tolerance between two roundings of the oracle's own operands (measured on the CPU:
    47 of 589824 elements of dW, 3.3e-3 against 1.1e-3 allowed)."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = _dyadic((2, 256, hw, hw), 1 / 128, 512, gen)
    dy = _dyadic((2, 256, hw, hw), 1 / 128, 512, gen)
    wt = _dyadic((256, 256, 3, 3), 24 / 65536, 63, gen)
    return x, dy, wt


def _close(got, want):
    torch.testing.assert_close(got.double(), want, rtol=1e-4,
                               atol=2e-5 * (want.abs().max().item() + 1))


@pytest.mark.parametrize('hw', [8, 14])
@pytest.mark.parametrize('flip', [False, True], ids=['forward', 'backward-data'])
@pytest.mark.parametrize('kind', [4, 2])
def test_batched_gemm_winograd_runs_the_high_products_at_both_levels(kind, flip, hw):
    x, _, wt = _wino_inputs(hw, 4)
    conv_w = wt.flip(2, 3).transpose(0, 1).contiguous() if flip else wt
    a = ops().bg_weight(wt, flip, kind, emu=1)  # (the image keeps its three planes)

    def run():
        return ops().bg_conv(x, a, None, 256, 0, 0, kind, 0, 0, emu=1)

    got = {'highest': run()}
    for level in REDUCED:
        with precision.conv_precision(level):
            got[level] = run()
    _close(got['highest'], wino_conv_emulated(x, conv_w, kind, 'highest'))
    _close(got['high'], wino_conv_emulated(x, conv_w, kind, 'high'))
    assert torch.equal(got['high'], got['medium'])
    assert not torch.equal(got['high'], got['highest'])
    print(f'F({kind}x{kind}) flip={flip} {hw}^2: high vs highest '
          f'{rel_err(got["high"], got["highest"]):.2e}')


@pytest.mark.parametrize('hw', [8, 14])
def test_batched_gemm_weight_gradient_runs_the_high_products_at_both_levels(hw):
    x, dy, _ = _wino_inputs(hw, 5)

    def run():
        return ops().wino4_wgrad(x, dy, 0, 2, None)  # variant 2: the split-bf16 batched GEMM

    got = {'highest': run()}
    for level in REDUCED:
        with precision.conv_precision(level):
            got[level] = run()
    want = torch.ops.aten.convolution_backward(
        dy.double(), x.double(), torch.zeros(256, 256, 3, 3, device='cuda', dtype=torch.float64),
        None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    _close(wino_wgrad_emulated(x, dy, 'highest'), want)  # (the emulation is the convolution)
    _close(got['highest'], wino_wgrad_emulated(x, dy, 'highest'))
    _close(got['high'], wino_wgrad_emulated(x, dy, 'high'))
    assert torch.equal(got['high'], got['medium'])
    assert not torch.equal(got['high'], got['highest'])
