"""sampler.run_chains, the one stepwise denoise loop, seen through its callers: the sharded loops of dgdm_amd/dist.py in a world of one rank
against the single-process samplers, the contract of guided_chains' trace, and the general case (several chains of averaged gradients,
a condition per chain, the classifier-free mix) against the library's loop.  Shapes: the small ones of tests/test_gpu_parity.py."""
import numpy as np
import pytest
import torch

from dgdm_amd import dist as ddist
from dgdm_amd import engine, sampler, synth
from tests import util
from tests.test_gpu_parity import dev, sched      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
T, S = 15, 5
_RIGS = {}


def _rig(dev, mode):      # noqa: F811
    """(net, handle over 4 objects, its spec, the objects, schedule, noise, unguided sample), built once per mode and left unchanged."""
    if mode not in _RIGS:
        net = engine.Unet1d(util.unet_sd(11))
        if mode == 'point':
            nv, B, G, P, L, sub = 100, 3, 7, 3, 14, 0
            dyn = engine.Dynamics(2, util.dyn2d_sd(22, nv), L, 2 * nv)
            objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(4)])
        else:
            nv, B, G, P, L, sub = 512, 2, 4, 2, 42, 9
            dyn = engine.Dynamics(3, util.dyn3d_sd(33), L)
            objs = torch.stack([synth.synth_object_3d(i) for i in (1, 8, 2, 31)])
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 8, T, nv, sub, max_objects=4)
        gd.set_objects(objs.to(dev))
        spec = ddist.GuidanceSpec(dyn, B, G, P, (-1.0, 1.0), T, nv, sub)
        s = sched(T, S)
        noise = synth.synth_noise(0, B, L).to(dev)
        _RIGS[mode] = (net, gd, spec, objs, s, noise, sampler.unguided_sample(net, s, noise))
    return _RIGS[mode]


def _stream(spec, mode, seed):
    return sampler.StartStream(spec.num_object_points, spec.sub_batch_size, seed=seed) if mode == 'point_3d' else None


@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_sharded_equals_single_process(dev, mode):      # noqa: F811
    """No process group is a world of one rank: the sharded loops then hold every object and every chain, and give the single-process
    samplers' bits from the same start stream - a named objective, a Goal (whose field leaves the handle as it found it), and per-object
    chains that mix 'convergence' with other objectives."""
    net, gd, spec, objs, s, noise, ug = _rig(dev, mode)
    assert ddist.world_rank() == (1, 0)
    want = sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1, 2, 3], 'shift_left', starts=_stream(spec, mode, 8))
    got = ddist.guided_multi_object_sharded(net, spec, s, mode, noise, objs, 'shift_left', starts=_stream(spec, mode, 8))
    assert got.shape == want.shape and torch.equal(got, want) and not torch.equal(got, ug)
    goal = sampler.Goal.from_physical(200.0, 0.01, -0.005, weight=(1.0, 0.5, 0.5), profile='linear')
    own = torch.zeros((1, gd.rows, 3), dtype=torch.float32, device=dev)
    gd.set_row_field(own)                                   # a field the caller set: the Goal's replaces it for the loop only
    try:
        want = sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1, 2, 3], goal, starts=_stream(spec, mode, 9))
        assert gd._row_field is own
        got = ddist.guided_multi_object_sharded(net, spec, s, mode, noise, objs, goal, starts=_stream(spec, mode, 9), build=lambda o, k: gd)
        assert gd._row_field is own
    finally:
        gd.set_row_field(None)
    assert torch.equal(got, want) and not torch.equal(got, ug)
    chains = [(0, 'rotate'), (1, 'convergence'), (2, 'shift_up'), (3, 'clockwise_left'), (0, 'convergence')]
    want = sampler.guided_chains(net, gd, s, mode, noise, chains, unguided=ug, starts=_stream(spec, mode, 10))
    got = ddist.guided_chains_sharded(net, spec, s, mode, noise, objs, chains, unguided=ug, starts=_stream(spec, mode, 10))
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("mode", ['point', 'point_3d'])
def test_trace_contract(dev, mode):      # noqa: F811
    """guided_chains(trace=tr): one (eps, grad, x) per step, each (n_chains, B, L), x the step's INPUT - so the first x is the start
    sample in every chain, and the DDIM step on an entry, chain by chain with the chain's own scale, is the next entry's x (the returned
    sample after the last).  Three chains whose scales differ, 'convergence' among them."""
    net, gd, spec, objs, s, noise, ug = _rig(dev, mode)
    B, L = noise.shape[:2]
    chains = [(0, 'rotate'), (1, 'convergence'), (2, 'shift_up')]
    scales = [sampler.chain_scale(mode, o) for _, o in chains]
    assert len(set(scales)) == 2
    tr = []
    out = sampler.guided_chains(net, gd, s, mode, noise, chains, unguided=ug, starts=_stream(spec, mode, 11), trace=tr)
    assert len(tr) == S == len(s.timesteps)
    for entry in tr:
        assert len(entry) == 3 and all(isinstance(v, torch.Tensor) and tuple(v.shape) == (3, B, L) for v in entry)
    assert torch.equal(tr[0][2], noise.reshape(1, B, L).expand(3, -1, -1))
    for si, t in enumerate(s.timesteps):
        eps, g, x = tr[si]
        nxt = tr[si + 1][2] if si + 1 < S else out.reshape(3, B, L)
        for c in range(3):
            assert torch.equal(engine.ddim_guided_step(x[c], eps[c], g[c], 1, s.coefficients(int(t)), scales[c]), nxt[c]), (mode, si, c)
    assert float(tr[0][1].abs().max()) > 0


def test_groups_stepwise_equals_library_with_chain_conditions(dev):      # noqa: F811
    """The runner's general case - K = 3 chains, each averaging 2 gradients, a condition block per chain and the classifier-free mix
    (cfg_weight 2.5) - walked in Python against the library's loop, 2-D."""
    _, gd, _, _, s, noise, _ = _rig(dev, 'point')
    gc, B = 6, noise.shape[0]
    net = engine.Unet1d(synth.synth_state_dict(synth.unet_spec(global_cond_dim=gc), 11))
    cond = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, (3, B, gc)).astype(np.float32)).to(dev)
    groups, objv = [[0, 1], [2, 3], [1, 3]], ['rotate', 'shift_down', 'counterclockwise_up']
    a = sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, global_cond=cond, cfg_weight=2.5)
    b = sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, global_cond=cond, cfg_weight=2.5, python_loop=True)
    assert a.shape == (3, B, noise.shape[1], 1) and torch.equal(a, b)
    assert not torch.equal(a, sampler.guided_multi_object_groups(net, gd, s, 'point', noise, groups, objv, global_cond=torch.roll(cond, 1, 0), cfg_weight=2.5))
