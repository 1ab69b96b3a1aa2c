"""Stochastic DDIM steps (eta > 0) on the GPU: the keyed device normals against numpy's Philox and the float64 Box-Muller recipe
(tests/step_noise_oracle.py), the noisy step against its float32 restatement, the eta = 0 corner against today's step, the chain runner
against the walk of its steps, and what the keys promise - a run split into calls or over ranks draws what the single call draws,
replicas of a pair diverge, an edit keeps its pins.  Every comparison of results is exact.

Sizes: T = 15, S = 5; 2-D B = 2, L = 14, G = 4, P = 1; 3-D B = 2, L = 42, G = 4, P = 2, sub_bs = 9 (the 3-D grid of tests/test_gpu_edit.py)."""
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine, sampler, synth
from dgdm_amd import dist as ddist
from dgdm_amd.edit import Edit
from dgdm_amd.scheduler import DDIMScheduler
from tests import step_noise_oracle as orc
from tests import util

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


def _rig(dev, mode):
    """(net, guidance handle over 4 objects, scheduler, noise (B, L, 1), GuidanceSpec of the handle), built once per module."""
    if mode not in _RIGS:
        net = engine.Unet1d(util.unet_sd(11))
        if mode == 'point':
            nv, B, G, P, L, sub = 100, 2, 4, 1, 14, 0
            dyn = engine.Dynamics(2, util.dyn2d_sd(22, nv), L, 2 * nv)
            objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(4)])
        else:
            nv, B, G, P, L, sub = 512, 2, 4, 2, 42, 9
            dyn = engine.Dynamics(3, util.dyn3d_sd(33), L)
            objs = torch.stack([synth.synth_object_3d(i) for i in (1, 8, 2, 31)])
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 8, T, nv, sub, max_objects=4)
        gd.set_objects(objs.to(dev))
        gd._objs = objs
        spec = ddist.GuidanceSpec(dyn, B, G, P, (-1.0, 1.0), T, nv, sub)
        _RIGS[mode] = (net, gd, _sched(), synth.synth_noise(0, B, L).to(dev), spec)
    return _RIGS[mode]


def _ulp_steps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float32 steps (both finite; the integer images of float32 are monotone on each side of zero)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ------------------------------------------------------------------------------------------------ 1. the noise values
def test_noise_values_match_the_recipe(dev):
    seed, keys = 7, [0, 5, 2 ** 40 + 1]
    seen = {}
    for step in (0, 3):
        for per_chain in (28, 84):
            z = engine.step_noise(seed, keys, step, per_chain).cpu().numpy()
            ref = orc.step_noise(seed, keys, step, per_chain)
            assert z.shape == ref.shape == (3, per_chain) and np.isfinite(z).all()
            d = _ulp_steps(z, ref)
            print(f"step {step}, per_chain {per_chain}: {int((d != 0).sum())} of {d.size} values differ, by at most {int(d.max())} float32 step")
            assert int(d.max()) <= 1, (step, per_chain, int(d.max()))
            seen[(step, per_chain)] = z
    for (step, per_chain), z in seen.items():
        assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[1], z[2]) and not np.array_equal(z[0], z[2])
        assert not np.array_equal(z, seen[(3 - step, per_chain)])
    # a chain's element does not depend on how many elements the chain has, on its place in the launch or on its neighbours
    assert np.array_equal(seen[(0, 28)], seen[(0, 84)][:, :28])
    one = engine.step_noise(seed, [5], 3, 84).cpu().numpy()
    assert np.array_equal(one[0], seen[(3, 84)][1])
    assert not np.array_equal(engine.step_noise(seed + 1, keys, 0, 28).cpu().numpy(), seen[(0, 28)])


# ------------------------------------------------------------------------------------------------ 2. moments
def test_noise_moments(dev):
    """N = 2^20 values of one launch, 4 keys x 2^18 elements; every bound is five standard errors of the exact normal."""
    per_chain, keys = 2 ** 18, [0, 1, 2, 3]
    z = engine.step_noise(11, keys, 2, per_chain).cpu().numpy().astype(np.float64)
    N = z.size
    assert N == 2 ** 20 and np.isfinite(z).all()
    mean, var = float(z.mean()), float(z.var())
    print(f"mean {mean:.3e} (bound {5 / np.sqrt(N):.3e}), variance - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / N):.3e})")
    assert abs(mean) < 5 / np.sqrt(N)
    assert abs(var - 1.0) < 5 * np.sqrt(2.0 / N)
    c = np.corrcoef(z)
    for i in range(4):
        for j in range(i + 1, 4):
            print(f"correlation of keys {i}, {j}: {c[i, j]:.3e} (bound {5 / np.sqrt(N / 4):.3e})")
            assert abs(c[i, j]) < 5 / np.sqrt(N / 4)


# ------------------------------------------------------------------------------------------------ 3. step arithmetic
def _step_inputs(seed, shape, n_grad):
    rs = np.random.RandomState(seed)
    x = (rs.randn(*shape) * 5.0).astype(np.float32)
    x.reshape(-1)[::7] = np.where(np.arange(x.size)[::7] % 2 == 0, 15.0, -15.0).astype(np.float32)           # the clamp is active
    eps = rs.randn(*shape).astype(np.float32)
    grad = rs.randn(n_grad, *shape).astype(np.float32)
    return x, eps, grad, rs.randn(*shape).astype(np.float32)


def _bounds(seed, B, L):
    rs = np.random.RandomState(seed)
    d = rs.uniform(-1.0, 1.0, (B, L)).astype(np.float32)
    kind = rs.randint(0, 3, (B, L))
    u = np.float32(0.07)
    lo = np.where(kind == 0, d, np.where(kind == 1, np.maximum(np.float32(-1.0), d - u), np.float32(-1.0))).astype(np.float32)
    hi = np.where(kind == 0, d, np.where(kind == 1, np.minimum(np.float32(1.0), d + u), np.float32(1.0))).astype(np.float32)
    return lo, hi


CASES = [(3, 2, 14), (10, 2, 14), (3, 2, 42), (4, 2, 42)]       # 84, 280 (two blocks), 252, 336 entries; per chain B * L = 28 / 84


@pytest.mark.parametrize("n_grad", [1, 3])
def test_noisy_step_equals_restatement(dev, n_grad):
    s = _sched()
    for ci, shape in enumerate(CASES):
        x, eps, grad, z = _step_inputs(400 + ci, shape, n_grad)
        lo, hi = _bounds(500 + ci, *shape[1:])
        xd, ed, gd_, zd = (torch.from_numpy(a).to(dev) for a in (x, eps, grad, z))
        keys = [3 * c + 1 for c in range(shape[0])]
        for si, t in enumerate(s.timesteps):
            coef, (sigma, dirc) = s.coefficients(int(t)), s.eta_coefficients(int(t), 0.7)
            for bounds, bd in ((None, None), ((lo, hi), (torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)))):
                kw = {} if bounds is None else dict(lo=bounds[0], hi=bounds[1])
                out = engine.ddim_guided_step(xd, ed, gd_, n_grad, coef, 0.8, bd, eta_coef=(sigma, dirc), variance_noise=zd).cpu().numpy()
                ref = orc.noisy_step(x, eps, grad, n_grad, coef, 0.8, sigma, dirc, z, **kw)
                assert np.array_equal(out, ref), (shape, int(t), bounds is None, float(np.abs(out - ref).max()))
                # the device's own noise: the restatement fed what engine.step_noise says the step drew
                zk = engine.step_noise(9, keys, si, shape[1] * shape[2]).cpu().numpy().reshape(shape)
                out = engine.ddim_guided_step(xd, ed, gd_, n_grad, coef, 0.8, bd, eta_coef=(sigma, dirc), seed=9, chain_keys=keys,
                                              step_index=si).cpu().numpy()
                ref = orc.noisy_step(x, eps, grad, n_grad, coef, 0.8, sigma, dirc, zk, **kw)
                assert np.array_equal(out, ref), (shape, int(t), bounds is None, float(np.abs(out - ref).max()))
    with pytest.raises(ValueError):
        engine.ddim_guided_step(xd, ed, None, 0, coef, 0.0, eta_coef=(0.3, 0.2))
    # the scheduler's own step: one chain, either source
    t = int(s.timesteps[1])
    a = s.step(ed, t, xd, eta=0.7, noise_key=(9, 4, 1)).prev_sample.cpu().numpy()
    z4 = engine.step_noise(9, [4], 1, x.size).cpu().numpy().reshape(x.shape)
    ref = orc.noisy_step(x, eps, None, 0, s.coefficients(t), 0.0, *s.eta_coefficients(t, 0.7), z4)
    assert np.array_equal(a, ref)
    assert np.array_equal(s.step(ed, t, xd, eta=0.7, variance_noise=torch.from_numpy(z4).to(dev)).prev_sample.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ 4. eta = 0 is the old step
@pytest.mark.parametrize("n_grad", [0, 1, 3])
def test_sigma_zero_is_todays_step(dev, n_grad):
    s = _sched()
    for ci, shape in enumerate(CASES):
        x, eps, grad, z = _step_inputs(600 + ci, shape, max(1, n_grad))
        lo, hi = _bounds(700 + ci, *shape[1:])
        bd = (torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))
        xd, ed, zd = (torch.from_numpy(a).to(dev) for a in (x, eps, z))
        gd_ = torch.from_numpy(grad).to(dev) if n_grad else None
        for t in s.timesteps:
            coef = s.coefficients(int(t))
            assert s.eta_coefficients(int(t), 0.0) == (0.0, coef[3])
            for b in (None, bd):
                ref = engine.ddim_guided_step(xd, ed, gd_, n_grad, coef, 10.0, b)
                for kw in ({}, dict(variance_noise=zd), dict(seed=3, chain_keys=[1] * shape[0])):
                    out = engine.ddim_guided_step(xd, ed, gd_, n_grad, coef, 10.0, b, eta_coef=(0.0, coef[3]), **kw)
                    assert torch.equal(out, ref), (shape, int(t), b is None, sorted(kw))


# ------------------------------------------------------------------------------------------------ 5. runner == walk
def _starts(gd, mode, n_rows, seed):
    """[S][n_rows][starts_per_call] for n_rows gradient chains (3-D), None in 2-D."""
    if mode != 'point_3d':
        return None
    _, st = sampler.draw_chain_starts(gd, [(0, 'rotate')] * n_rows, S, sampler.pair_stream(512, 9, seed, 0))
    return np.ascontiguousarray(st)


def _both(dev, mode, pairs, n_chains, n_grad, scales, **kw):
    """run_chains as the one library call and as the walk of its steps, for the gradient chains `pairs` (object-major)."""
    net, gd, s, noise, _ = _rig(dev, mode)
    B, L = noise.shape[:2]
    objectives = [engine.make_objective(o, oi) for oi, o in pairs]
    st = _starts(gd, mode, len(pairs), 12)
    args = (net, gd, s, noise.reshape(B, L), n_chains, n_grad, objectives, None, st, s.timesteps, scales)
    a = sampler.run_chains(*args, **kw)
    b = sampler.run_chains(*args, stepwise=True, **kw)
    assert a.shape == (n_chains, B, L) and bool(torch.isfinite(a).all())
    return a, b


RUNNER_CASES = {
    "2d": ('point', [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left')], 3, 1, [0.001] * 3),
    "2d_per_chain_scales": ('point', [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left')], 3, 1, [0.001, 10.0, 0.5]),
    "2d_multi_object": ('point', [(0, 'rotate'), (1, 'shift_down'), (2, 'rotate'), (3, 'shift_down')], 2, 2, [0.001] * 2),
    "3d": ('point_3d', [(0, 'rotate'), (1, 'shift_up'), (3, 'clockwise_left')], 3, 1, [0.5] * 3),
}


@pytest.mark.parametrize("case", sorted(RUNNER_CASES))
def test_runner_equals_walk(dev, case):
    mode, pairs, nc, n_grad, scales = RUNNER_CASES[case]
    a, b = _both(dev, mode, pairs, nc, n_grad, scales, eta=0.5, noise_seed=5)
    assert torch.equal(a, b), float((a - b).abs().max())
    a0, b0 = _both(dev, mode, pairs, nc, n_grad, scales)
    assert torch.equal(a0, b0) and not torch.equal(a, a0)
    assert float(a.abs().max()) <= 1.0              # the last step has sigma = 0: the result is the clipped prediction
    k, _ = _both(dev, mode, pairs, nc, n_grad, scales, eta=0.5, noise_seed=5, chain_keys=[7, 8, 9][:nc])
    assert not torch.equal(k, a)


# ------------------------------------------------------------------------------------------------ 6. split invariance
CHAINS6 = [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left'), (3, 'rotate'), (0, 'shift_down'), (2, 'shift_left')]


@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_split_into_calls_and_ranks(dev, mode):
    net, gd, s, noise, spec = _rig(dev, mode)
    kw = dict(eta=0.5, noise_seed=5)
    pre = sampler.draw_chain_starts(gd, CHAINS6, S, sampler.pair_stream(512, 9, 4, 0)) if mode == 'point_3d' else None
    cut = lambda lo, hi: None if pre is None else (pre[0][lo:hi], np.ascontiguousarray(pre[1][:, lo:hi]))      # noqa: E731
    one = sampler.guided_chains(net, gd, s, mode, noise, CHAINS6, predrawn=pre, **kw)
    halves = [sampler.guided_chains(net, gd, s, mode, noise, CHAINS6[lo:lo + 3], predrawn=cut(lo, lo + 3), chain_keys=[lo, lo + 1, lo + 2], **kw)
              for lo in (0, 3)]
    assert torch.equal(torch.cat(halves), one)
    # without its keys the second half draws the first half's noise
    assert not torch.equal(sampler.guided_chains(net, gd, s, mode, noise, CHAINS6[3:], predrawn=cut(3, 6), **kw), halves[1])
    # ranks 0 and 1 of world 2, the way dist.guided_chains_sharded runs a rank's block: its objects, its chains, its global indices as keys
    blocks = []
    for rank in (0, 1):
        mine, local_objects, local_chains = ddist.shard_chains(CHAINS6, rank, 2)
        guid = spec.build(gd._objs[local_objects].to(dev), len(local_chains))
        blocks.append(sampler.guided_chains(net, guid, s, mode, noise, local_chains, predrawn=cut(mine.start, mine.stop),
                                            chain_keys=ddist.chain_noise_keys(mine), **kw))
    assert torch.equal(torch.cat(blocks), one)
    # the sharded functions themselves, at world size 1
    stream = lambda: sampler.pair_stream(512, 9, 4, 0) if mode == 'point_3d' else None      # noqa: E731
    assert torch.equal(ddist.guided_chains_sharded(net, spec, s, mode, noise, gd._objs, CHAINS6, starts=stream(), **kw), one)
    m = sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1, 2], 'shift_left', starts=stream(), **kw)
    assert torch.equal(ddist.guided_multi_object_sharded(net, spec, s, mode, noise, gd._objs[:3], 'shift_left', starts=stream(), **kw), m)
    assert not torch.equal(m, sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1, 2], 'shift_left', starts=stream()))


# ------------------------------------------------------------------------------------------------ 7. replicas and shared noise
def test_replicas_and_shared_noise(dev):
    net, gd, s, noise, _ = _rig(dev, 'point')
    twice = [(1, 'shift_up'), (1, 'shift_up')]
    run = lambda **kw: sampler.guided_chains(net, gd, s, 'point', noise, twice, **kw)      # noqa: E731
    plain = run()
    assert torch.equal(plain[0], plain[1])                          # eta = 0: replicas are one design
    a = run(eta=1.0, noise_seed=3)
    assert not torch.equal(a[0], a[1])
    shared = run(eta=1.0, noise_seed=3, shared_step_noise=True)
    assert torch.equal(shared[0], shared[1]) and torch.equal(shared[0], a[0])       # key 0 is the first replica's own key
    assert torch.equal(run(eta=1.0, noise_seed=3), a)
    assert not torch.equal(run(eta=1.0, noise_seed=4), a)
    # the unguided loop and the groups take the same arguments
    u = sampler.unguided_sample(net, s, noise, eta=1.0, noise_seed=3)
    assert torch.equal(u, sampler.unguided_sample(net, s, noise, eta=1.0, noise_seed=3)) and not torch.equal(u, sampler.unguided_sample(net, s, noise))
    groups, objv = [[0, 1], [0, 1]], ['rotate', 'rotate']
    g = sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, eta=1.0, noise_seed=3)
    assert torch.equal(g, sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, eta=1.0, noise_seed=3, python_loop=True))
    assert not torch.equal(g[0], g[1])
    gs = sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, eta=1.0, noise_seed=3, shared_step_noise=True)
    assert torch.equal(gs[0], gs[1])


# ------------------------------------------------------------------------------------------------ 8. edits
@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_edits_keep_their_promises_under_noise(dev, mode):
    net, gd, s, noise, _ = _rig(dev, mode)
    B, L = noise.shape[:2]
    designs = np.random.RandomState(77).uniform(-0.95, 0.95, (B, L)).astype(np.float32)
    designs[0, 8] = 1.0                                             # a band that is cut by the sampler's range
    e = Edit.from_physical(designs, pins=tuple(range(7)), band_mm=2.0, steps=3, mode=mode)
    twice = [(1, 'shift_up'), (1, 'shift_up')]
    pre = sampler.draw_chain_starts(gd, twice, 3, sampler.pair_stream(512, 9, 6, 0)) if mode == 'point_3d' else None
    run = lambda **kw: sampler.guided_chains(net, gd, s, mode, noise, twice, edit=e, predrawn=pre, **kw)      # noqa: E731
    out = run(eta=1.0, noise_seed=3)
    assert torch.equal(out, run(eta=1.0, noise_seed=3, trace=[]))
    o = out.cpu().numpy()[..., 0]
    lo, hi = e.bounds()
    assert np.array_equal(o[:, :, :7], np.broadcast_to(designs[:, :7], o[:, :, :7].shape))         # the pins, exactly
    assert np.all(o >= lo[None]) and np.all(o <= hi[None])                                          # no entry leaves its band
    assert not np.array_equal(o[0], o[1])                                                           # two keys, two edits
    assert not np.array_equal(o[0, :, 7:], designs[:, 7:])
    assert not torch.equal(out, run())


# ------------------------------------------------------------------------------------------------ 9. the entry point
def test_cli_eta(dev, monkeypatch):
    """generator/train.py --mode=test with the flags of test_cli_entry_point (tests/test_gpu_api.py) in 2-D, at its smallest sizes,
    plus --eta 0.5 --noise_seed 3.  The per-step PNG plots are stubbed (they are that test's subject) and nothing is saved."""
    from dgdm_amd.generator import artefacts
    from dgdm_amd.generator.train import train
    from dgdm_amd.dynamics.parser import parse
    monkeypatch.setattr(artefacts, "plot_fingers", lambda path, *a, **k: path)
    common = ("--mode=test --classifier_guidance --num_fingers=2 --batch_size=2 --grid_size=3 --num_pos=2 --object_max_num_vertices=10 "
              "--ctrlpts_dim=14 --num_train_timesteps=15 --num_inference_steps=5")
    _, plain = train(parse(shlex.split(common)))
    _, again = train(parse(shlex.split(common)))
    _, noisy = train(parse(shlex.split(common + " --eta 0.5 --noise_seed 3")))
    assert len(plain) == 1 and plain[0]["eta"] == 0.0 and plain[0]["noise_seed"] == 0
    assert noisy[0]["eta"] == 0.5 and noisy[0]["noise_seed"] == 3
    keys = [k for k in plain[0] if k.startswith(("guided/", "multi/")) or k == "unguided"]
    assert len(keys) == 24 and noisy[0].keys() == plain[0].keys()
    for k in keys:
        assert torch.equal(plain[0][k], again[0][k]), k
        assert not torch.equal(plain[0][k], noisy[0][k]), k
        assert bool(torch.isfinite(noisy[0][k]).all()) and float(noisy[0][k].abs().max()) <= 1.0, k
    assert plain[0]["stats"] == again[0]["stats"] and plain[0]["stats"]["val/denoise loss"] != noisy[0]["stats"]["val/denoise loss"]
