"""Editing designs on the GPU: the bounded DDIM step (dgdm_ddim_guided_step_bounded) against today's step and against the float32
restatement (tests/edit_oracle.py), the bounded chain runner against today's runner and against its step-by-step composition, the end
points an edit promises, and the command line.  Every comparison is exact.

Sizes: T = 15, S = 5; 2-D B = 3, L = 14, G = 4, P = 2; 3-D B = 2, L = 42, G = 4, P = 2, sub_bs = 9 (the 3-D grid of
test_native_loop_equals_step_by_step, tests/test_gpu_parity.py); 2-3 chains."""
import ctypes as C
import json
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine, sampler, synth
from dgdm_amd.edit import Edit
from dgdm_amd.scheduler import DDIMScheduler
from tests import edit_oracle, util

pytestmark = pytest.mark.gpu
T, S = 15, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def _sched():
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(S)
    return s


_RIGS = {}


def _rig(dev, mode, gc=0):
    """(net, guidance handle over 4 objects, scheduler, noise (B, L, 1), designs (B, L)), built once per module."""
    key = (mode, gc)
    if key not in _RIGS:
        net = engine.Unet1d(synth.synth_state_dict(synth.unet_spec(global_cond_dim=gc), 11) if gc else util.unet_sd(11))
        if mode == 'point':
            nv, B, G, P, L, sub = 100, 3, 4, 2, 14, 0
            dyn = engine.Dynamics(2, util.dyn2d_sd(22, nv), L, 2 * nv)
            objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(4)])
        else:
            nv, B, G, P, L, sub = 512, 2, 4, 2, 42, 9
            dyn = engine.Dynamics(3, util.dyn3d_sd(33), L)
            objs = torch.stack([synth.synth_object_3d(i) for i in (1, 8, 2, 31)])
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 8, T, nv, sub, max_objects=4)
        gd.set_objects(objs.to(dev))
        gd._objs = objs                                              # (for the sharded functions, which build handles of their own)
        designs = np.random.RandomState(77).uniform(-0.95, 0.95, (B, L)).astype(np.float32)
        designs[0, 1], designs[1, 2] = 1.0, -0.99                    # a band that is cut by the sampler's range
        _RIGS[key] = (net, gd, _sched(), synth.synth_noise(0, B, L).to(dev), designs)
    return _RIGS[key]


def _step_inputs(seed, shape, n_grad):
    rs = np.random.RandomState(seed)
    x = (rs.randn(*shape) * 5.0).astype(np.float32)
    x.reshape(-1)[::7] = np.where(np.arange(x.size)[::7] % 2 == 0, 15.0, -15.0).astype(np.float32)           # up to +-15: the clamp is active
    eps = rs.randn(*shape).astype(np.float32)
    grad = rs.randn(n_grad, *shape).astype(np.float32) if n_grad else None
    return x, eps, grad


def _mixed_bounds(seed, B, L):
    """Bounds (B, L) that mix pins, bands cut and uncut by [-1, 1], and free entries."""
    rs = np.random.RandomState(seed)
    d = rs.uniform(-1.0, 1.0, (B, L)).astype(np.float32)
    kind = rs.randint(0, 3, (B, L))
    u = np.float32(0.07)
    lo = np.where(kind == 0, d, np.where(kind == 1, np.maximum(np.float32(-1.0), d - u), np.float32(-1.0))).astype(np.float32)
    hi = np.where(kind == 0, d, np.where(kind == 1, np.minimum(np.float32(1.0), d + u), np.float32(1.0))).astype(np.float32)
    assert (kind == 0).any() and (kind == 1).any() and (kind == 2).any() and np.all(lo <= hi)
    return lo, hi


CASES = [((3, 3, 14), 42), ((9, 3, 14), 42), ((3, 2, 42), 84), ((7, 2, 42), 84)]       # 126, 378 (two blocks), 252, 588 entries; period B * L


# ------------------------------------------------------------------------------------------------ 1. step vs today's step
@pytest.mark.parametrize("n_grad", [0, 1, 3])
def test_step_free_bounds_equal_todays_step(dev, n_grad):
    s = _sched()
    for ci, (shape, period) in enumerate(CASES):
        x, eps, grad = _step_inputs(100 + ci, shape, n_grad)
        xd, ed = torch.from_numpy(x).to(dev), torch.from_numpy(eps).to(dev)
        gd_ = torch.from_numpy(grad).to(dev) if n_grad else None
        for p in (1, period):
            bounds = (torch.full((p,), -1.0, device=dev), torch.full((p,), 1.0, device=dev))
            for t in s.timesteps:
                coef = s.coefficients(int(t))
                for scale in (0.8, 10.0):
                    ref = engine.ddim_guided_step(xd, ed, gd_, n_grad, coef, scale)
                    out = engine.ddim_guided_step_bounded(xd, ed, gd_, n_grad, coef, scale, bounds)
                    assert torch.equal(out, ref), (shape, p, int(t), scale)
        assert float(ref.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. step vs restatement
@pytest.mark.parametrize("n_grad", [0, 1, 3])
def test_step_equals_restatement(dev, n_grad):
    s = _sched()
    for ci, (shape, period) in enumerate(CASES):
        x, eps, grad = _step_inputs(200 + ci, shape, n_grad)
        lo, hi = _mixed_bounds(300 + ci, *shape[1:])
        bounds = (torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))
        xd, ed = torch.from_numpy(x).to(dev), torch.from_numpy(eps).to(dev)
        gd_ = torch.from_numpy(grad).to(dev) if n_grad else None
        for t in s.timesteps:
            coef = s.coefficients(int(t))
            for scale in (0.8, 10.0):
                out = engine.ddim_guided_step_bounded(xd, ed, gd_, n_grad, coef, scale, bounds).cpu().numpy()
                ref = edit_oracle.bounded_step(x, eps, grad, n_grad, coef, scale, lo, hi)
                assert np.array_equal(out, ref), (shape, int(t), scale, float(np.abs(out - ref).max()))
        pinned = np.broadcast_to(lo == hi, shape)
        assert np.array_equal(out[pinned], np.broadcast_to(lo, shape)[pinned])              # the last step (t = 0) returns the pins exactly


# ------------------------------------------------------------------------------------------------ 3. argument checks
def test_einval_before_any_launch(dev):
    n, period = 126, 42
    x, eps = torch.randn(n, device=dev), torch.randn(n, device=dev)
    lo, hi = torch.full((n,), -1.0, device=dev), torch.full((n,), 1.0, device=dev)
    out = torch.full((n,), 7.0, device=dev)
    step = lambda l, h, p: _lib.lib().dgdm_ddim_guided_step_bounded(x.data_ptr(), eps.data_ptr(), None, 0, out.data_ptr(), n, 0.9, 0.4, 0.95, 0.3, 0.0,      # noqa: E731
                                                                   l, h, p, _lib.stream_ptr())
    for l, h, p in ((lo.data_ptr(), hi.data_ptr(), 40), (lo.data_ptr(), hi.data_ptr(), 0), (lo.data_ptr(), hi.data_ptr(), -42),
                    (lo.data_ptr(), hi.data_ptr(), 2 * n), (None, hi.data_ptr(), period), (lo.data_ptr(), None, period), (None, None, period)):
        assert step(l, h, p) == _lib.EINVAL, (l is None, h is None, p)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert step(lo.data_ptr(), hi.data_ptr(), period) == _lib.OK and step(lo.data_ptr(), hi.data_ptr(), n) == _lib.OK
    torch.cuda.synchronize()
    assert bool((out != 7.0).all())
    with pytest.raises(ValueError):
        engine.ddim_guided_step_bounded(x, eps, None, 0, (0.9, 0.4, 0.95, 0.3), 0.0, (lo[:40], hi[:40]))
    with pytest.raises(ValueError):
        engine.ddim_guided_step_bounded(x, eps, None, 0, (0.9, 0.4, 0.95, 0.3), 0.0, (lo[:42], hi[:21]))
    with pytest.raises(ValueError):
        engine.ddim_guided_step_bounded(x, eps, None, 0, (0.9, 0.4, 0.95, 0.3), 0.0, (lo[:42], None))
    # the runner: exactly one bound is DGDM_EINVAL before anything is launched
    net, gd, s, noise, designs = _rig(dev, 'point')
    B, L = designs.shape
    objectives = [engine.make_objective('rotate', 0), engine.make_objective('shift_up', 1)]
    arr = (_lib.Objective * 2)(*objectives)
    tsa = (C.c_int32 * S)(*[int(t) for t in s.timesteps])
    cfa = (C.c_float * (4 * S))(*[float(v) for t in s.timesteps for v in s.coefficients(int(t))])
    sca = (C.c_float * 2)(0.001, 0.001)
    x0, res = noise.reshape(B, L).contiguous(), torch.full((2, B, L), 7.0, device=dev)
    run = lambda l, h: _lib.lib().dgdm_guided_chains_run_bounded(net._h, gd._h, x0.data_ptr(), 2, 1, arr, None, None, tsa, cfa, sca, S, res.data_ptr(),      # noqa: E731
                                                                 None, 0, 1.0, l, h, _lib.stream_ptr())
    assert run(lo.data_ptr(), None) == _lib.EINVAL and run(None, hi.data_ptr()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((res == 7.0).all())
    with pytest.raises(ValueError):
        engine.guided_chains_run(net, gd, x0, 2, 1, objectives, None, None, [int(t) for t in s.timesteps], [s.coefficients(int(t)) for t in s.timesteps],
                                 [0.001, 0.001], bounds=(lo[:14], hi[:14]))


# ------------------------------------------------------------------------------------------------ the step-by-step composition
def _compose(net, gd, s, timesteps, x_start, objectives, rowcoef, scales, n_grad, bounds, starts=None, cond=None, w=1.0):
    """Unet1d.forward (+ the library's classifier-free mix), Guidance.grad and the scheduler step, step by step from Python: the
    bounded step, or today's when bounds is None.  x_start (B, L, 1); gradient chains object-major (gradient j of chain k is j * nc + k)."""
    nc, (B, L) = len(scales), x_start.shape[:2]
    x = x_start.reshape(1, B, L).expand(nc, -1, -1).contiguous()
    crow = None if cond is None else cond.reshape(1, B, -1).expand(nc, -1, -1).reshape(nc * B, -1).contiguous()
    for si, t in enumerate(timesteps):
        t = int(t)
        ts = torch.full((nc * B,), t, dtype=torch.int32, device=x.device)
        if crow is None:
            eps = net.forward(x.reshape(nc * B, L, 1), ts)
        elif w == 1.0:
            eps = net.forward(x.reshape(nc * B, L, 1), ts, crow)
        else:
            eps = engine.cfg_mix(net.forward(x.reshape(nc * B, L, 1), ts, crow), net.forward(x.reshape(nc * B, L, 1), ts, torch.zeros_like(crow)), w)
        eps = eps.reshape(nc, B, L)
        g = gd.grad(x.repeat(n_grad, 1, 1), t, objectives, rowcoef, None if starts is None else np.ascontiguousarray(starts[si]).reshape(-1))
        coef = s.coefficients(t)
        step = (lambda *a: engine.ddim_guided_step(*a)) if bounds is None else (lambda *a: engine.ddim_guided_step_bounded(*a, bounds))     # noqa: E731
        if len(set(scales)) == 1:
            x = step(x, eps, g, n_grad, coef, scales[0])
        else:
            x = torch.stack([step(x[c], eps[c], g[c], 1, coef, scales[c]) for c in range(nc)])
    return x.reshape(nc, B, L, 1)


# ------------------------------------------------------------------------------------------------ 4. runner vs today's runner
@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_runner_without_bounds_is_todays_runner(dev, mode):
    net, gd, s, noise, designs = _rig(dev, mode)
    B, L = designs.shape
    chains = [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left')]
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    scales = [sampler.chain_scale(mode, o) for _, o in chains]
    ts, coefs = [int(t) for t in s.timesteps], [s.coefficients(int(t)) for t in s.timesteps]
    starts = None
    if mode == 'point_3d':
        _, starts = sampler.draw_chain_starts(gd, chains, S, sampler.pair_stream(512, 9, 3, 0))
        starts = np.ascontiguousarray(starts)
    x0 = noise.reshape(B, L).contiguous()
    a = engine.guided_chains_run(net, gd, x0, 3, 1, objectives, None, starts, ts, coefs, scales)                       # bounds=None
    arr = (_lib.Objective * 3)(*objectives)
    tsa, cfa, sca = (C.c_int32 * S)(*ts), (C.c_float * (4 * S))(*[float(v) for c in coefs for v in c]), (C.c_float * 3)(*scales)
    sp = None if starts is None else starts.ctypes.data
    out = {}
    for name in ("plain", "cond", "bounded"):
        out[name] = torch.full((3, B, L), 7.0, device=dev)
    assert _lib.lib().dgdm_guided_chains_run(net._h, gd._h, x0.data_ptr(), 3, 1, arr, None, sp, tsa, cfa, sca, S, out["plain"].data_ptr(), _lib.stream_ptr()) == _lib.OK
    assert _lib.lib().dgdm_guided_chains_run_cond(net._h, gd._h, x0.data_ptr(), 3, 1, arr, None, sp, tsa, cfa, sca, S, out["cond"].data_ptr(), None, 0, 1.0,
                                                  _lib.stream_ptr()) == _lib.OK
    assert _lib.lib().dgdm_guided_chains_run_bounded(net._h, gd._h, x0.data_ptr(), 3, 1, arr, None, sp, tsa, cfa, sca, S, out["bounded"].data_ptr(), None, 0, 1.0,
                                                     None, None, _lib.stream_ptr()) == _lib.OK
    for name, o in out.items():
        assert torch.equal(o, a), (mode, name)
    # today's runner is today's steps, composed (the plain kernel: nothing of this feature in the reference)
    ref = _compose(net, gd, s, s.timesteps, noise, objectives, None, scales, 1, None, starts)
    assert torch.equal(a.reshape(ref.shape), ref), mode
    # and the bounded kernel with the scheduler's own range is the same run
    free = (torch.full((B, L), -1.0, device=dev), torch.full((B, L), 1.0, device=dev))
    b = engine.guided_chains_run(net, gd, x0, 3, 1, objectives, None, starts, ts, coefs, scales, bounds=free)
    assert torch.equal(a, b), mode
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5. runner vs composition
def _edit(designs, mode, steps=None):
    L = designs.shape[1]
    return Edit(designs, pins=(0, 1, 2, 3, 4, 5, 6, 10) if L == 14 else tuple(range(0, 21)) + (30,), band=0.05, steps=steps, mode=mode)


def test_edit_chains_2d_mixed_scales(dev):
    """Per-object chains with mixed classifier scales (one 'convergence' chain, whose centres come from the source designs): the
    per-chain-scale loop of the runner, each chain with the same bounds block."""
    net, gd, s, noise, designs = _rig(dev, 'point')
    e = _edit(designs, 'point')
    chains = [(0, 'rotate'), (1, 'convergence'), (2, 'shift_up')]
    a = sampler.guided_chains(net, gd, s, 'point', noise, chains, edit=e)
    assert torch.equal(a, sampler.guided_chains(net, gd, s, 'point', noise, chains, edit=e, trace=[]))
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    scales = [sampler.chain_scale('point', o) for _, o in chains]
    assert len(set(scales)) == 2
    centers = sampler.convergence_centers(gd, 'point', e.designs_on(dev), [1])
    rc = np.zeros((3, gd.rows), dtype=np.float32)
    rc[1] = gd.rowcoef(centers[0])
    x_start, ts = e.start(s, noise)
    assert len(ts) == S
    ref = _compose(net, gd, s, ts, x_start, objectives, torch.from_numpy(rc).to(dev), scales, 1, e.bounds_on(dev))
    assert torch.equal(a, ref), float((a - ref).abs().max())
    # the unguided sample is not read by an edit: its 'convergence' centres are the designs'
    assert torch.equal(a, sampler.guided_chains(net, gd, s, 'point', noise, chains, edit=e, unguided=torch.zeros_like(noise)))


def test_edit_chains_3d(dev):
    """3-D, one classifier scale for all chains: one bounded launch with period B * L over all chains; K = 3 of S = 5, the FPS starts
    drawn for 3 steps."""
    net, gd, s, noise, designs = _rig(dev, 'point_3d')
    e = _edit(designs, 'point_3d', steps=3)
    chains = [(0, 'rotate'), (1, 'shift_up'), (3, 'clockwise_left')]
    pre = sampler.draw_chain_starts(gd, chains, 3, sampler.pair_stream(512, 9, 5, 0))
    assert pre[1].shape[0] == 3
    a = sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, edit=e, predrawn=pre)
    assert torch.equal(a, sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, edit=e, predrawn=pre, trace=[]))
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    scales = [sampler.chain_scale('point_3d', o) for _, o in chains]
    assert len(set(scales)) == 1
    x_start, ts = e.start(s, noise)
    assert [int(t) for t in ts] == [6, 3, 0]
    ref = _compose(net, gd, s, ts, x_start, objectives, None, scales, 1, e.bounds_on(dev), pre[1])
    assert torch.equal(a, ref), float((a - ref).abs().max())
    # without predrawn starts the sampler draws them itself, for the edit's 3 steps
    torch.manual_seed(9)
    b = sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, edit=e)
    torch.manual_seed(9)
    assert torch.equal(b, sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, edit=e, trace=[]))


def test_edit_multi_object(dev):
    """n_grad > 1: one chain that averages three objects' gradients, and two such chains in one launch."""
    net, gd, s, noise, designs = _rig(dev, 'point')
    e = _edit(designs, 'point')
    a = sampler.guided_multi_object(net, gd, s, 'point', noise, [0, 1, 2], 'shift_left', edit=e)
    assert torch.equal(a, sampler.guided_multi_object(net, gd, s, 'point', noise, [0, 1, 2], 'shift_left', edit=e, on_step=lambda i, x: None))
    x_start, ts = e.start(s, noise)
    objectives = [engine.make_objective('shift_left', oi) for oi in (0, 1, 2)]
    ref = _compose(net, gd, s, ts, x_start, objectives, None, [sampler.chain_scale('point', 'shift_left', multi=True)], 3, e.bounds_on(dev))
    assert torch.equal(a, ref[0]), float((a - ref[0]).abs().max())
    groups, objv = [[0, 1], [2, 3]], ['rotate', 'shift_down']
    ga = sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, edit=e)
    assert torch.equal(ga, sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, edit=e, python_loop=True))
    objectives = [engine.make_objective(objv[k], groups[k][j]) for j in range(2) for k in range(2)]
    ref = _compose(net, gd, s, ts, x_start, objectives, None, [sampler.chain_scale('point', o, multi=True) for o in objv], 2, e.bounds_on(dev))
    assert torch.equal(ga, ref), float((ga - ref).abs().max())
    # the unguided loop and the scheduler's own step take the same bounds
    u = sampler.unguided_sample(net, s, noise, edit=e)
    x = x_start
    for t in ts:
        x = s.step(net.forward(x, torch.full((x.shape[0],), int(t), dtype=torch.int32, device=dev)), t, x, bounds=e.bounds_on(dev)).prev_sample
    assert torch.equal(u, x)


def test_edit_conditional_cfg_partial(dev):
    """A conditional eps-net with cfg_weight = 2.5 (one eps-net call of twice the samples, then the mix) and K = 2 of S = 5 from Edit.start."""
    gc = 6
    net, gd, s, noise, designs = _rig(dev, 'point', gc)
    e = _edit(designs, 'point', steps=2)
    B = designs.shape[0]
    cond = torch.from_numpy(np.random.RandomState(21).uniform(-1, 1, (B, gc)).astype(np.float32)).to(dev)
    chains = [(0, 'rotate'), (1, 'shift_left')]
    a = sampler.guided_chains(net, gd, s, 'point', noise, chains, edit=e, global_cond=cond, cfg_weight=2.5)
    assert torch.equal(a, sampler.guided_chains(net, gd, s, 'point', noise, chains, edit=e, global_cond=cond, cfg_weight=2.5, trace=[]))
    x_start, ts = e.start(s, noise)
    assert [int(t) for t in ts] == [3, 0]
    assert torch.equal(x_start, s.add_noise(e.designs_on(dev), noise, torch.full((B,), 3)))
    objectives = [engine.make_objective(o, oi) for oi, o in chains]
    ref = _compose(net, gd, s, ts, x_start, objectives, None, [sampler.chain_scale('point', o) for _, o in chains], 1, e.bounds_on(dev), cond=cond, w=2.5)
    assert torch.equal(a, ref), float((a - ref).abs().max())
    assert not torch.equal(a, sampler.guided_chains(net, gd, s, 'point', noise, chains, edit=e, global_cond=cond, cfg_weight=1.0))


def test_sharded_functions_forward_the_edit(dev):
    """dist.guided_chains_sharded / guided_multi_object_sharded in one process: the edit goes through, the 3-D draws are made for its K steps."""
    from dgdm_amd import dist as ddist
    for mode, (nv, sub) in (('point', (100, 0)), ('point_3d', (512, 9))):
        net, gd, s, noise, designs = _rig(dev, mode)
        e = _edit(designs, mode, steps=3)
        spec = ddist.GuidanceSpec(gd.dyn, designs.shape[0], 4, 2, (-1.0, 1.0), T, nv, sub)
        chains = [(0, 'rotate'), (2, 'shift_up'), (0, 'clockwise_left')]
        stream = lambda: sampler.pair_stream(512, 9, 8, 0) if mode == 'point_3d' else None      # noqa: E731
        a = ddist.guided_chains_sharded(net, spec, s, mode, noise, gd._objs, chains, starts=stream(), edit=e)
        assert torch.equal(a, sampler.guided_chains(net, gd, s, mode, noise, chains, starts=stream(), edit=e)), mode
        b = ddist.guided_multi_object_sharded(net, spec, s, mode, noise, gd._objs[:3], 'shift_left', starts=stream(), edit=e)
        assert torch.equal(b, sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1, 2], 'shift_left', starts=stream(), edit=e)), mode
        assert np.array_equal(b.cpu().numpy()[:, list(e.pins), 0], designs[:, list(e.pins)])


# ------------------------------------------------------------------------------------------------ 6. end points
@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_end_points(dev, mode):
    net, gd, s, noise, designs = _rig(dev, mode)
    e = _edit(designs, mode)
    pins, u = list(e.pins), np.float32(e.band)
    free = [i for i in range(designs.shape[1]) if i not in pins]
    chains = [(0, 'rotate'), (2, 'shift_up')]
    pre = sampler.draw_chain_starts(gd, chains, S, sampler.pair_stream(512, 9, 6, 0)) if mode == 'point_3d' else None
    run = lambda ed: sampler.guided_chains(net, gd, s, mode, noise, chains, edit=ed, predrawn=pre).cpu().numpy()[..., 0]      # noqa: E731
    out = run(e)
    lo, hi = e.bounds()
    d = np.broadcast_to(designs, out.shape)
    assert np.array_equal(out[:, :, pins], d[:, :, pins])                                  # the pins, exactly
    assert np.all(out >= lo[None]) and np.all(out <= hi[None])                             # every entry inside its bounds
    assert np.all(out[:, :, free] >= (d[:, :, free] - u)) and np.all(out[:, :, free] <= (d[:, :, free] + u))      # |out - d| <= u, in float32
    assert np.all(np.abs(out) <= 1.0)
    assert not np.array_equal(out[:, :, free], d[:, :, free])                              # and the edit did move something
    mx, rms = e.moved_mm(out)
    assert mx.shape == out.shape[:2] and float(mx.max()) <= float(u) * (30.0 if mode == 'point' else 50.0) * (1 + 1e-5) and float(rms.max()) > 0
    # pins alone: the pinned points' states are what the eps-net saw, so the free points end elsewhere than without pins
    pinned, unpinned = run(Edit(designs, pins=pins, mode=mode)), run(Edit(designs, mode=mode))
    assert np.array_equal(pinned[:, :, pins], d[:, :, pins])
    assert not np.array_equal(pinned[:, :, free], unpinned[:, :, free])
    assert not np.array_equal(unpinned[:, :, pins], d[:, :, pins])


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_cli_edit(dev, tmp_path, monkeypatch):
    """generator/train.py --mode=test at the sizes of test_cli_entry_point (tests/test_gpu_api.py) with --edit_from f.npy --pin 0-6
    --edit_band_mm 2 --edit_steps 3 --predicted_sim.  Two things stand beside the flags the test is about: --predicted_rollout=1, because
    --predicted_sim alone refuses that test's even --num_pos=2 (it has no centre cell to score), and the per-step PNG plots are stubbed
    (they are test_cli_entry_point's subject and take most of its time)."""
    from dgdm_amd.generator import artefacts
    from dgdm_amd.generator.train import OBJECT_NAMES_3D, train
    from dynamics.parser import parse
    monkeypatch.setattr(artefacts, "plot_fingers", lambda path, *a, **k: path)
    src = np.random.RandomState(5).uniform(-0.9, 0.9, (5, 42)).astype(np.float32)
    f = str(tmp_path / "f.npy")
    np.save(f, src[..., None])
    common = ("--mode=test --classifier_guidance --fingers_3d --num_fingers=4 --batch_size=2 --grid_size=3 --num_pos=2 --sub_bs=5 "
              "--object_max_num_vertices=512 --ctrlpts_dim=42 --num_train_timesteps=15 --num_inference_steps=5 --predicted_sim --predicted_rollout=1")
    flags = f" --edit_from {f} --pin 0-6 --edit_band_mm 2 --edit_steps 3"
    torch.manual_seed(3)
    _, res = train(parse(shlex.split(common + flags + f" --save_dir={tmp_path / 'edit'}")))
    assert len(res) == 2
    tag = "rotate_orirange=-1.000_1.000"
    u = np.float32(2.0 / 1000.0 / 0.05)
    assert "guided/rotate" not in res[1]                  # validation_step runs the sweep on batch 0 only, i.e. on rows [0, 2)
    for b in range(1):
        d = src[2 * b:2 * b + 2]
        for key in ("guided/rotate", "guided/convergence", "multi/shift_up"):
            out = res[b][key].cpu().numpy()[..., 0]
            assert out.shape[-2:] == (2, 42)
            assert np.array_equal(out[..., :7], np.broadcast_to(d[:, :7], out[..., :7].shape)), (b, key)
            assert np.all(out >= np.maximum(np.float32(-1), d - u)) and np.all(out <= np.minimum(np.float32(1), d + u)), (b, key)
            assert not np.array_equal(out[..., 7:], np.broadcast_to(d[:, 7:], out[..., 7:].shape)), (b, key)
    root = tmp_path / "edit"
    assert not os.path.exists(root / "vis_guided")
    saved = np.load(root / "vis_edit" / tag / "BABY_CAR.npy")
    assert saved.shape == (2, 42, 1) and np.array_equal(saved[:, :7, 0], src[0:2, :7])
    assert np.array_equal(saved, res[0]["guided/rotate"].cpu().numpy()[OBJECT_NAMES_3D.index("BABY_CAR")])
    assert os.path.exists(root / "vis_edit" / tag / "BABY_CAR_geometry.npy") and os.path.exists(root / "vis_edit" / tag / "allobj.npy")
    assert np.array_equal(np.load(root / "vis_edit" / "edit_source" / "edit_source.npy")[..., 0], src[0:2])
    assert os.path.exists(root / "val_vis_noise" / "unguided" / "unguided.npy")                 # the unguided loops are untouched
    tables = sorted(os.listdir(root / "tables"))
    assert len([t for t in tables if t.startswith("val__edit_sample__allobj_")]) == 11
    assert len([t for t in tables if t.startswith("val__edit_sample__") and "allobj" not in t]) == 12
    assert not [t for t in tables if t.startswith("val__guided_sample__")] and len([t for t in tables if t.startswith("val__unguided_sample__")]) == 12
    for t in tables:
        if not t.startswith("val__edit_sample__"):
            continue
        tab = json.load(open(root / "tables" / t))
        cols = tab["columns"]
        assert cols[-3:] == ["edit_moved_mm_max", "edit_moved_mm_rms", "edit_pins"], t
        assert all(len(row) == len(cols) for row in tab["data"]), t
        assert all(row[-1] == 7 and 0.0 <= row[-2] <= row[-3] <= 2.0 * (1 + 1e-5) for row in tab["data"]), t
        source = [row for row in tab["data"] if row[cols.index("gripper")] == "edit_source"]
        assert len(source) == (1 if "allobj" in t else 6), t
        assert all(isinstance(row[cols.index("objective")], dict) and row[cols.index("objective")].get("predicted") for row in source), t
        assert any(row[-3] > 0 for row in tab["data"]), t
    # the same command without the edit flags: the tree of a run without edits, and no vis_edit/
    torch.manual_seed(3)
    _, plain = train(parse(shlex.split(common + f" --save_dir={tmp_path / 'plain'}")))
    root = tmp_path / "plain"
    assert "vis_edit" not in os.listdir(root) and {"tables", "val_vis_noise", "vis_guided"} <= set(os.listdir(root))
    assert len(os.listdir(root / "vis_guided")) == 12 and os.path.exists(root / "vis_guided" / tag / "BABY_CAR.npy")
    tables = sorted(os.listdir(root / "tables"))
    assert not [t for t in tables if "edit" in t] and len([t for t in tables if t.startswith("val__guided_sample__")]) == 23
    tab = json.load(open(root / "tables" / [t for t in tables if t.startswith("val__guided_sample__rotate_")][0]))
    assert tab["columns"] == ["object_idx", "gripper", "objective", "profile", "final", "last_img", "gripper_dir"]
    assert plain[0].keys() == res[0].keys() and torch.equal(plain[0]["unguided"], res[0]["unguided"])
    assert not torch.equal(plain[0]["guided/rotate"], res[0]["guided/rotate"])
    with pytest.raises(ValueError, match="edit_from"):
        train(parse(shlex.split(common + " --pin 0-6")))
