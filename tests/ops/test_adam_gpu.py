"""The fused Adam / AdamW kernels (``csrc/optim.hip``) on the GPU.  Accuracy is judged as in
``test_optim_gpu.py``: against ``torch.optim`` in fp64, a tensor's largest error may be at most
twice that of fp32 ``torch.optim(foreach=False)`` on the CPU, plus half an ulp of its largest
oracle value (the reference error of a one-element tensor can be exactly zero by luck, while a
correctly rounded result may be half an ulp off)."""
import copy
import functools
import math

import pytest
import torch
from torch import nn
import torch.nn.functional as F

from tests.ops.optim_cases import as_params, make_values, set_grads
from tests.ops.test_adam import CONFIGS, LR, assert_same, build, numels, run, snapshot
from torchgpipe_amd import optim
from torchgpipe_amd.ops import _ext
from torchgpipe_amd.parallel import PipelineStage, StepGraph

pytestmark = pytest.mark.gpu

cuda = torch.device('cuda', 0)
EPS = 1e-6


@pytest.fixture(autouse=True)
def need_ext():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    assert _ext.available(), f'HIP extension must load on a GPU box: {_ext.load_error()!r}'


@functools.lru_cache(None)
def _inputs():
    """The boundary-size inputs, made once and never modified."""
    return make_values(numels(optim.optim_info()[0]))


def _worst_ratio(native, reference, oracle):
    """Asserts the module docstring's bound on three snapshots; the largest error ratio."""
    worst = 0.0
    for (gp, gs), (rp, rs), (wp, ws) in zip(native, reference, oracle):
        assert gs.keys() == ws.keys()
        for got, ref, want in [(gp, rp, wp)] + [(gs[k], rs[k], ws[k]) for k in gs]:
            got_err = float((got.double() - want).abs().max())
            ref_err = float((ref.double() - want).abs().max())
            if got_err > 0:
                worst = max(worst, got_err / ref_err if ref_err > 0 else math.inf)
            assert got_err <= 2 * ref_err + 2.0 ** -24 * float(want.abs().max()), (
                want.numel(), got_err, ref_err)
    return worst


@pytest.mark.parametrize('config', list(CONFIGS))
def test_five_steps_within_twice_torchs_fp32_error(config):
    inits, grads = _inputs()
    assert sum(v.numel() for v in inits) < 2 ** 20
    lr32 = float(torch.tensor(LR, dtype=torch.float32))
    oracle, _, _ = run(False, config, inits, grads, dtype=torch.float64, lr=lr32)
    reference, _, _ = run(False, config, inits, grads)
    native, opt, params = run(True, config, inits, grads, device=cuda)
    assert all(p.is_cuda and opt.state[p]['step'].is_cuda for p in params)
    worst = max(_worst_ratio(*rows) for rows in zip(native, reference, oracle))
    print(f'{config}: largest native / reference error ratio {worst:.3f}')


@pytest.mark.parametrize('config', ['adam_wd', 'adamw_amsgrad'])
@pytest.mark.parametrize('big_first', [True, False])
def test_each_tensor_of_a_launch_has_its_own_step_count(config, big_first):
    """Two tables' worth of tensors, a third of which sit out the first step."""
    chunk, per_launch, _ = optim.optim_info()
    big, ones = [2 * chunk + 5], [1] * (per_launch + 1)
    inits, grads = make_values(big + ones if big_first else ones + big, seed=1)
    kwargs = dict(device=cuda, steps=3, skip=lambda step, i: step == 0 and i % 3 == 0)
    want, _, _ = run(True, config, inits, grads, grouped=True, **kwargs)
    got, opt, params = run(True, config, inits, grads, **kwargs)
    assert_same(got[-1], want[-1])
    for i, p in enumerate(params):
        step = opt.state[p]['step']
        assert step.device == p.device and step.dtype == torch.float32 and step.dim() == 0
        assert float(step) == (2 if i % 3 == 0 else 3)
        assert not torch.equal(got[-1][i][0], inits[i])


def _clip_run(config, clip, bound_scale):
    """Three steps with the clip 'fused', as grad_scale_ ('scale') or without (None); the
    snapshot and whether .grad was left alone."""
    inits, grads = _inputs()
    params = as_params(inits, cuda)
    opt = build(True, config, params)
    untouched = True
    for step in range(3):
        set_grads(params, grads, step)
        gs = [p.grad for p in params]
        before = [g.clone() for g in gs]
        sumsq = torch.ops.tgpipe.grad_sumsq(gs)
        bound = bound_scale * math.sqrt(float(sumsq))
        if clip == 'scale':
            torch.ops.tgpipe.grad_scale_(gs, sumsq, bound, EPS)
        opt.step(**({'grad_sumsq': sumsq, 'max_norm': bound} if clip == 'fused' else {}))
        untouched = untouched and all(torch.equal(g, b) for g, b in zip(gs, before))
    return snapshot(opt, params), untouched


@pytest.mark.parametrize('config', ['adam_wd', 'adamw_amsgrad'])
def test_fused_clip_is_bitwise_scale_then_step(config):
    fused, untouched = _clip_run(config, 'fused', 0.5)  # half the norm: active
    plain, _ = _clip_run(config, None, 0.5)
    assert untouched
    assert_same(fused, _clip_run(config, 'scale', 0.5)[0])
    for (_, fs), (_, ps) in zip(fused, plain):  # the clip took part
        assert all(not torch.equal(fs[k], ps[k]) for k in fs)
    fused, untouched = _clip_run(config, 'fused', 2.0)  # twice the norm: inactive
    assert untouched
    assert_same(fused, plain)


def test_offset_views_are_bitwise_alike_and_stay_in_bounds():
    n, pad = optim.optim_info()[0] + 37, 16  # a full chunk and a ragged one
    gen = torch.Generator().manual_seed(2)
    values = [torch.randn(n, generator=gen) for _ in range(5)]  # p, g, m, v, vmax
    values[3], values[4] = values[3].abs(), values[4].abs()
    lr = torch.tensor(0.05, device=cuda)
    # each pointer over its offsets alone, then all together
    cases = [(0,) * 5] + [tuple(off if i == which else 0 for i in range(5))
                          for which in range(5) for off in (1, 2, 3)]
    cases += [(1,) * 5, (3,) * 5, (1, 2, 3, 1, 2)]
    first = None
    for offsets in cases:
        bufs = [torch.full((n + 2 * pad,), 7.0, device=cuda) for _ in values]  # sentinels
        p, g, m, v, vmax = views = [b[pad + o:pad + o + n] for b, o in zip(bufs, offsets)]
        for view, value, o in zip(views, values, offsets):
            view.copy_(value)
            assert view.data_ptr() % 16 == 4 * o
        step = torch.tensor(2.0, device=cuda)
        torch.ops.tgpipe.adam_step_([p], [g], [m], [v], [vmax], [step], lr, 0.9, 0.999, 1e-8,
                                    1e-2, True, True, None, 0.0, EPS)
        assert float(step) == 3.0 and torch.equal(g.cpu(), values[1])
        got = [t.cpu() for t in (p, m, v, vmax)]
        first = first or got
        assert all(torch.equal(a, b) for a, b in zip(got, first)), offsets
        for buf, o in zip(bufs, offsets):
            assert bool((buf[:pad + o] == 7.0).all() and (buf[pad + o + n:] == 7.0).all())
    assert all(not torch.equal(a, values[i]) for a, i in zip(first, (0, 2, 3, 4)))


def test_captured_step_advances_the_device_step_counts():
    """Warm-ups, the capture and three replays against the same steps run eagerly.  Linear
    layers: their gradients are the same bits in every run, which the convolutions' weight
    gradients (accumulated with atomics) are not, eagerly or captured."""
    lr, clip, steps = 2.0 ** -7, 0.01, 6
    torch.manual_seed(0)
    base = nn.Sequential(nn.Linear(24, 40), nn.ReLU(), nn.Linear(40, 7))
    gen = torch.Generator().manual_seed(1)
    batches = [(torch.randn(8, 24, generator=gen).to(cuda),
                torch.randn(8, 7, generator=gen).to(cuda)) for _ in range(steps)]
    ends = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        stage = PipelineStage(model, [len(model)], device=cuda, chunks=2,
                              checkpoint='except_last')
        opt = optim.AdamW(stage.parameters(), lr=lr, amsgrad=True)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        graph = StepGraph(stage, F.mse_loss, opt, warmup=2, max_grad_norm=clip)
        for x, y in batches:
            if graphed:
                graph.step(x, y)  # the other run leaves its StepGraph unused
            else:
                opt.zero_grad(set_to_none=True)
                stage.train_step(x, y, F.mse_loss)
                assert float(stage.optimizer_step(opt, clip)) > clip  # every step clips
            sched.step()
        torch.cuda.synchronize()
        params = list(stage.parameters())
        assert graph.captured == graphed
        assert all(float(opt.state[p]['step']) == steps for p in params)
        ends.append(snapshot(opt, params))
    assert_same(ends[1], ends[0])
    assert not torch.equal(ends[0][0][0], base[0].weight)


def test_state_dicts_move_between_torch_and_native_with_a_mixed_model():
    """Mid-run; the fp64 parameter takes the PyTorch-operation path under the same clip."""
    config = 'adamw_amsgrad'
    inits, grads = make_values([3, optim.optim_info()[0] + 5, 40], seed=3)
    mixed = [v.double() if i == 2 else v for i, v in enumerate(inits)]

    def clipped_step(opt, step):
        params = opt.param_groups[0]['params']
        set_grads(params, grads, step)
        total = sum(p.grad.double().square().sum() for p in params).reshape(1)
        bound = 0.5 * math.sqrt(float(total))
        if optim.is_native(opt):
            opt.step(grad_sumsq=total, max_norm=bound)
        else:  # clip_grad_norm_ on the same fp64 norm (torch's own adds fp32 norms)
            for p in params:
                p.grad.mul_(min(1.0, bound / (math.sqrt(float(total)) + EPS)))
            opt.step()
        return snapshot(opt, params)

    ref = build(False, config, as_params(mixed))
    oracle = build(False, config, as_params([v.double() for v in inits]))
    for step in range(2):
        clipped_step(ref, step), clipped_step(oracle, step)
    # torch -> native: the host steps land on the device as fp32
    native = build(True, config, as_params([p.detach() for p in ref.param_groups[0]['params']],
                                           cuda))
    saved = copy.deepcopy(ref.state_dict())
    assert all(not s['step'].is_cuda for s in saved['state'].values())
    native.load_state_dict(saved)
    for p in native.param_groups[0]['params']:
        step = native.state[p]['step']
        assert step.device == p.device and step.dtype == torch.float32 and float(step) == 2
    got, want, exact = (clipped_step(opt, 2) for opt in (native, ref, oracle))
    _worst_ratio(got[:2], want[:2], exact[:2])
    # the fp64 parameter: fp64 arithmetic in another order, under the same fp64 clip
    torch.testing.assert_close(got[2][0], exact[2][0], rtol=1e-12, atol=1e-13)
    # native -> torch: the next step continues in torch.optim.AdamW on the GPU
    back = build(False, config, as_params([p for p, _ in got], cuda))
    back.load_state_dict(copy.deepcopy(native.state_dict()))
    got, want = clipped_step(back, 3), clipped_step(ref, 3)
    for (gp, _), (wp, _), p in zip(got, want, back.param_groups[0]['params']):
        torch.testing.assert_close(gp, wp)  # torch's GPU kernels against its CPU ones
        assert float(back.state[p]['step']) == 4


def test_nan_gradient_and_nan_sumsq_propagate_as_in_torch():
    c = optim.optim_info()[0]
    inits, grads = make_values([5, 2 * c + 5, 300], seed=5)
    grads[1][0][c + 11] = float('nan')
    want, _, _ = run(False, 'adamw_amsgrad', inits, grads, steps=1)
    got, _, _ = run(True, 'adamw_amsgrad', inits, grads, device=cuda, steps=1)
    for i, ((gp, gs), (wp, ws)) in enumerate(zip(got[0], want[0])):
        for a, b in [(gp, wp)] + [(gs[k], ws[k]) for k in ws]:
            assert torch.equal(a.isnan(), b.isnan())
            assert int(a.isnan().sum()) == (i == 1) and (i != 1 or bool(a[c + 11].isnan()))
    # a NaN sum of squares is a NaN coefficient: every element it reaches becomes NaN
    params = as_params(inits, cuda)
    opt = build(True, 'adamw_amsgrad', params)
    set_grads(params, grads, 1)
    before = [p.grad.clone() for p in params]
    opt.step(grad_sumsq=torch.tensor(float('nan'), dtype=torch.float64, device=cuda),
             max_norm=1.0)
    assert all(bool(p.isnan().all()) for p in params)
    assert all(torch.equal(p.grad, b) for p, b in zip(params, before))
