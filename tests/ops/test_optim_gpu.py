"""The fused optimizer kernels (``csrc/optim.hip``) on the GPU.  Sizes come from the build
(``optim_info``).

Accuracy is judged against ``torch.optim`` in fp64 on CPU copies of the same fp32 inputs, by
what fp32 ``torch.optim(foreach=False)`` on the CPU itself loses against that oracle: per
tensor, the kernels' largest absolute error -- parameters and every state tensor, after each
of five steps -- may be at most twice the reference's.  Why 2: a kernel may contract a
multiply-add that torch rounds twice, or round where torch's vector code fuses; each moves an
element by at most the roundings torch already commits.  (The kernels spell out torch's CPU
roundings: the measured ratio is 1 for every SGD configuration and 1.31 to 1.64 for RMSprop,
``profiles/r14/optim/README.md``.)
"""
import math

import pytest
import torch

from tests.ops import optim_cases as cases
from torchgpipe_amd import optim
from torchgpipe_amd.ops import _ext, gradclip

pytestmark = pytest.mark.gpu

cuda = torch.device('cuda', 0)
EPS = 1e-6


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


def _boundary_numels():
    c = optim.optim_info()[0]
    return [1, 3, 63, 64, 65, 255, 256, 257, c - 1, c, c + 1, 2 * c + 5]


_shared = {}


def _inputs():
    """The boundary-size inputs, made once and never modified."""
    if 'inputs' not in _shared:
        _shared['inputs'] = cases.make_values(_boundary_numels())
    return _shared['inputs']


def _errors(history, oracle):
    """Per step and tensor: {name: max abs error} of a run against the fp64 oracle."""
    out = []
    for got, want in zip(history, oracle):
        row = []
        for (gp, gs), (wp, ws) in zip(got, want):
            assert gs.keys() == ws.keys()
            errs = {'param': float((gp.double() - wp).abs().max())}
            for key in gs:
                errs[key] = float((gs[key].double() - ws[key]).abs().max())
            row.append(errs)
        out.append(row)
    return out


@pytest.mark.parametrize('config', list(cases.CONFIGS))
def test_five_steps_within_twice_torchs_fp32_error(config):
    kind = cases.CONFIGS[config][0]
    inits, grads = _inputs()
    assert sum(v.numel() for v in inits) < 2 ** 20
    # the oracle takes the LR the fp32 runs use: the fp32 value of the nominal rate
    lr32 = float(torch.tensor(cases.LR[kind], dtype=torch.float32))
    oracle, _, _ = cases.run(cases.TORCH[kind], config, inits, grads, dtype=torch.float64,
                             lr=lr32)
    reference, _, _ = cases.run(cases.TORCH[kind], config, inits, grads)
    native, opt, params = cases.run(cases.NATIVE[kind], config, inits, grads, device=cuda)
    assert all(p.is_cuda for p in params)
    ref_err, got_err = _errors(reference, oracle), _errors(native, oracle)
    worst = 0.0
    for step, (ref_row, got_row) in enumerate(zip(ref_err, got_err)):
        for i, (ref, got) in enumerate(zip(ref_row, got_row)):
            for key in ref:
                if got[key] > 0:
                    worst = max(worst, got[key] / ref[key] if ref[key] > 0 else math.inf)
                assert got[key] <= 2 * ref[key], (step, inits[i].numel(), key, got[key],
                                                  ref[key])
    print(f'{config}: largest native / reference error ratio {worst:.3f}')


@pytest.mark.parametrize('config', ['sgd_weight_decay', 'rmsprop_all'])
@pytest.mark.parametrize('big_first', [True, False])
def test_more_tensors_than_one_launch(config, big_first):
    """A list that takes two tables gives, bit for bit, what one launch per tensor gives."""
    kind = cases.CONFIGS[config][0]
    chunk, per_launch, _ = optim.optim_info()
    big, ones = [2 * chunk + 5], [1] * (per_launch + 1)
    inits, grads = cases.make_values(big + ones if big_first else ones + big, seed=1)
    want, _, _ = cases.run(cases.NATIVE[kind], config, inits, grads, device=cuda, steps=2,
                           grouped=True)
    got, _, _ = cases.run(cases.NATIVE[kind], config, inits, grads, device=cuda, steps=2)
    for (gp, gs), (wp, ws), init in zip(got[-1], want[-1], inits):
        assert torch.equal(gp, wp) and not torch.equal(gp, init)
        assert gs.keys() == ws.keys() and len(gs) > 0
        for key in gs:
            assert torch.equal(gs[key], ws[key]), key


PAD = 16


def _padded(values, offset):
    """``values`` in an ``offset``-element view of a sentinel-padded GPU buffer."""
    n = values.numel()
    buf = torch.full((n + 2 * PAD,), 7.0, device=cuda)
    view = buf[PAD + offset:PAD + offset + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return buf, view


def _sentinels_intact(buf, offset, n):
    ahead, behind = buf[:PAD + offset], buf[PAD + offset + n:]
    return bool((ahead == 7.0).all()) and bool((behind == 7.0).all())


def _offset_cases():
    """(param, grad, buf) offsets: each pointer over its 4 offsets alone, then all together."""
    out = [(0, 0, 0)]
    for which in range(3):
        for off in (1, 2, 3):
            out.append(tuple(off if i == which else 0 for i in range(3)))
    out += [(1, 1, 1), (3, 3, 3), (1, 2, 3)]
    return out


@pytest.mark.parametrize('op', ['sgd', 'rmsprop'])
def test_offset_views_are_bitwise_alike_and_stay_in_bounds(op):
    n = optim.optim_info()[0] + 37  # a full chunk and a ragged one
    gen = torch.Generator().manual_seed(2)
    p0, g0, b0 = (torch.randn(n, generator=gen) for _ in range(3))
    b0 = b0.abs()  # also a valid square_avg
    lr = torch.tensor(0.05, device=cuda)
    results = []
    for offsets in _offset_cases():
        (pb, p), (gb, g), (bb, b) = (_padded(v, o) for v, o in zip((p0, g0, b0), offsets))
        if op == 'sgd':
            torch.ops.tgpipe.sgd_step_([p], [g], [b], lr, 0.9, 0.1, True, 1e-3, False,
                                       None, 0.0, EPS)
        else:
            torch.ops.tgpipe.rmsprop_step_([p], [g], [b], [], [], lr, 0.99, 1e-8, 1e-3, 0.0,
                                           False, None, 0.0, EPS)
        results.append((p.cpu().clone(), b.cpu().clone()))
        assert torch.equal(g.cpu(), g0)
        for buf, off in zip((pb, gb, bb), offsets):
            assert _sentinels_intact(buf, off, n), offsets
    for offsets, (p, b) in zip(_offset_cases(), results):
        assert torch.equal(p, results[0][0]), offsets
        assert torch.equal(b, results[0][1]), offsets
    assert not torch.equal(results[0][0], p0) and not torch.equal(results[0][1], b0)


def _gpu_run(kind, config, inits, grads, clip, bound_scale):
    """Three steps on the GPU.  clip: 'fused' (step(grad_sumsq=)), 'scale' (grad_scale_ then
    the plain step) or None.  Returns the snapshots and whether .grad was left alone."""
    params = cases.as_params(inits, cuda)
    opt = cases.build(cases.NATIVE[kind], config, params)
    untouched = True
    for step in range(3):
        cases.set_grads(params, grads, step)
        gs = [p.grad for p in params]
        before = [g.clone() for g in gs]
        sumsq = torch.ops.tgpipe.grad_sumsq(gs)
        bound = bound_scale * math.sqrt(float(sumsq))
        if clip == 'fused':
            opt.step(grad_sumsq=sumsq, max_norm=bound)
            untouched = untouched and all(torch.equal(g, b) for g, b in zip(gs, before))
        elif clip == 'scale':
            torch.ops.tgpipe.grad_scale_(gs, sumsq, bound, EPS)
            opt.step()
        else:
            opt.step()
    return cases.snapshot(opt, params), untouched


def _assert_bitwise(got, want):
    for (gp, gs), (wp, ws) in zip(got, want):
        assert torch.equal(gp, wp)
        for key in gs:
            assert torch.equal(gs[key], ws[key]), key


@pytest.mark.parametrize('config', ['sgd_weight_decay', 'sgd_nesterov', 'rmsprop', 'rmsprop_all'])
def test_fused_clip_is_bitwise_scale_then_step(config):
    kind = cases.CONFIGS[config][0]
    inits, grads = _inputs()
    # active: the bound is half the norm
    fused, untouched = _gpu_run(kind, config, inits, grads, 'fused', 0.5)
    scaled, _ = _gpu_run(kind, config, inits, grads, 'scale', 0.5)
    plain, _ = _gpu_run(kind, config, inits, grads, None, 0.5)
    assert untouched
    _assert_bitwise(fused, scaled)
    # the clip took part: every tensor's state differs from the unclipped run's (RMSprop's
    # parameters alone need not: its update is nearly invariant to the gradient's scale)
    for (fp, fs), (pp, ps) in zip(fused, plain):
        assert not torch.equal(fp, pp) or any(not torch.equal(fs[k], ps[k]) for k in fs)
        assert all(not torch.equal(fs[k], ps[k]) for k in fs)
    # inactive: twice the norm
    fused, untouched = _gpu_run(kind, config, inits, grads, 'fused', 2.0)
    assert untouched
    _assert_bitwise(fused, plain)


def test_lr_is_read_on_the_device_and_versions_advance():
    n = optim.optim_info()[0] + 5
    p = torch.zeros(n, device=cuda)
    g = torch.ones(n, device=cuda)
    lr = torch.tensor(0.5, device=cuda)
    args = ([p], [g], [], lr, 0.0, 0.0, False, 0.0, False, None, 0.0, EPS)
    version = p._version
    torch.ops.tgpipe.sgd_step_(*args)
    assert p._version > version and bool((p == -0.5).all())
    version = p._version
    lr.fill_(0.125)  # the same Python arguments: only the device scalar changed
    torch.ops.tgpipe.sgd_step_(*args)
    assert p._version > version and bool((p == -0.625).all())
    # through the optimizer class: every written tensor's version advances each step
    param = torch.nn.Parameter(torch.zeros(n, device=cuda))
    opt = optim.RMSprop([param], lr=0.01, momentum=0.9, centered=True)
    seen = None
    for _ in range(3):
        param.grad = torch.ones(n, device=cuda)
        opt.step()
        now = [param._version] + [opt.state[param][k]._version for k in cases.STATE_KEYS]
        assert seen is None or all(a > b for a, b in zip(now, seen))
        seen = now


def test_empty_lists_and_empty_tensors():
    lr = torch.tensor(0.5, device=cuda)
    empty = torch.zeros(0, device=cuda)
    torch.ops.tgpipe.sgd_step_([], [], [], lr, 0.0, 0.0, False, 0.0, False, None, 0.0, EPS)
    torch.ops.tgpipe.sgd_step_([empty], [empty], [empty], lr, 0.9, 0.0, False, 0.0, False,
                               None, 0.0, EPS)
    torch.ops.tgpipe.rmsprop_step_([], [], [], [], [], lr, 0.99, 1e-8, 0.0, 0.0, False,
                                   None, 0.0, EPS)
    p, g = torch.ones(3, device=cuda), torch.full((3,), 2.0, device=cuda)
    sq = torch.zeros(3, device=cuda)
    flat = empty.reshape(0, 4)
    torch.ops.tgpipe.rmsprop_step_([empty, p, flat], [empty, g, flat], [empty, sq, flat], [], [],
                                   lr, 0.75, 0.0, 0.0, 0.0, False, None, 0.0, EPS)
    assert bool((sq == 1.0).all()) and bool((p == 0.0).all())  # 1 - 0.5 * 2 / sqrt(1)
    # the optimizer classes on parameters without elements or without gradients
    params = cases.as_params([torch.zeros(0), torch.ones(2)], cuda)
    params[0].grad = torch.zeros(0, device=cuda)
    optim.SGD(params, lr=0.1, momentum=0.9).step()
    assert bool((params[1] == 1.0).all())


def test_native_ops_refuse_what_the_python_layer_routes_away():
    lr = torch.tensor(0.5, device=cuda)

    def sgd(p, g, lr=lr):
        torch.ops.tgpipe.sgd_step_([p], [g], [], lr, 0.0, 0.0, False, 0.0, False, None, 0.0, EPS)

    ok = torch.ones(4, 6, device=cuda)
    with pytest.raises(RuntimeError, match='float32'):
        sgd(ok.half(), ok.half())
    with pytest.raises(RuntimeError, match='float32'):
        sgd(ok, ok.bfloat16())
    with pytest.raises(RuntimeError, match='dense'):
        sgd(ok[:, :3], ok[:, :3])
    with pytest.raises(RuntimeError, match='GPU'):
        sgd(ok.cpu(), ok.cpu())
    with pytest.raises(RuntimeError, match='numel'):
        sgd(ok, torch.ones(4, 5, device=cuda))
    with pytest.raises(RuntimeError, match='layout'):
        sgd(ok, ok.t().contiguous().t())
    with pytest.raises(RuntimeError, match='one length'):
        torch.ops.tgpipe.sgd_step_([ok], [], [], lr, 0.0, 0.0, False, 0.0, False, None, 0.0, EPS)
    with pytest.raises(RuntimeError, match='lr must be'):
        sgd(ok, ok, lr=torch.tensor(0.5, device=cuda, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='sumsq must be'):
        torch.ops.tgpipe.sgd_step_([ok], [ok], [], lr, 0.0, 0.0, False, 0.0, False,
                                   torch.ones(1, device=cuda), 1.0, EPS)
    assert bool((ok == 1.0).all())


def test_mixed_parameters_take_both_paths():
    """fp32 dense parameters go to the kernel, others (fp64 here) through PyTorch operations
    on the GPU, in one step with one fused clip."""
    gen = torch.Generator().manual_seed(4)
    values = [torch.randn(300, generator=gen), torch.randn(40, dtype=torch.float64, generator=gen)]
    grads = [[torch.randn(v.shape, dtype=v.dtype, generator=gen) for _ in range(2)]
             for v in values]
    got, want = cases.as_params(values, cuda), cases.as_params(values)
    a = optim.SGD(got, lr=0.0625, momentum=0.9, weight_decay=1e-3)
    b = optim.SGD(want, lr=0.0625, momentum=0.9, weight_decay=1e-3)
    for step in range(2):
        cases.set_grads(got, grads, step)
        cases.set_grads(want, grads, step)
        total = gradclip.grad_sumsq([p.grad for p in want])
        bound = 0.5 * math.sqrt(float(total))
        a.step(grad_sumsq=total, max_norm=bound)  # the sum lives on the CPU: copied over
        b.step(grad_sumsq=total, max_norm=bound)
    torch.testing.assert_close(got[0].cpu(), want[0], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(got[1].cpu(), want[1], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop'])
def test_nan_gradient_and_nan_sumsq_propagate_as_in_torch(kind):
    c = optim.optim_info()[0]
    inits, grads = cases.make_values([5, 2 * c + 5, 300], seed=5)
    grads[1][0][c + 11] = float('nan')
    config = 'sgd_weight_decay' if kind == 'sgd' else 'rmsprop_all'
    want, _, _ = cases.run(cases.TORCH[kind], config, inits, grads, steps=1)
    got, _, _ = cases.run(cases.NATIVE[kind], config, inits, grads, device=cuda, steps=1)
    for (gp, gs), (wp, ws) in zip(got[0], want[0]):
        assert torch.equal(gp.isnan(), wp.isnan())
        for key in gs:
            assert torch.equal(gs[key].isnan(), ws[key].isnan()), key
    assert bool(got[0][1][0][c + 11].isnan()) and int(got[0][1][0].isnan().sum()) == 1
    # a NaN sum of squares is a NaN coefficient: every element it reaches becomes NaN
    inits, grads = cases.make_values([5, c + 3], seed=6)
    params = cases.as_params(inits, cuda)
    opt = cases.build(cases.NATIVE[kind], config, params)
    cases.set_grads(params, grads, 0)
    before = [p.grad.clone() for p in params]
    opt.step(grad_sumsq=torch.tensor(float('nan'), dtype=torch.float64, device=cuda),
             max_norm=1.0)
    assert all(bool(p.isnan().all()) for p in params)
    assert all(torch.equal(p.grad, b) for p, b in zip(params, before))
