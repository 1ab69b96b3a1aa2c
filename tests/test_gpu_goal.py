"""Goal-pose objectives on the GPU: the per-row seed of the trunk's backward pass (use_rowcoef == 2, dgdm_guidance_set_row_field) in the
three trunks, the goal field builder (dgdm_guidance_goal_field), Goal chains through the sampler, and the predicted goal scores."""
import ctypes as C
import json
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine, sampler, synth
from dgdm_amd._lib import DgdmError
from oracle import dgdm_oracle as orc
from tests import goal_oracle, util
from tests.test_gpu_parity import REL, _guid2d, dev, finger_l2, sched      # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
DTYPES = ("f32", "f32_mfma", "bf16")


def _field_objective(oi, lin=(0.0, 0.0, 0.0), quad=(0.0, 0.0, 0.0)):
    return engine.make_objective(None, oi, row_field=True, lin=lin, quad=quad)


def _case(kind, dev, dtype):
    """A small handle of either kind with a ragged last tile, two chains' inputs and (3-D) their start draws."""
    if kind == 2:
        nv, B, G, P, L, T = 100, 5, 7, 3, 14, 15
        dyn = engine.Dynamics(2, util.dyn2d_sd(77, nv), L, 2 * nv)
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 4, T, nv, 0, max_objects=2, contraction_dtype=dtype)
        gd.set_objects(torch.stack([synth.synth_object_2d(i, nv) for i in range(2)]).to(dev))
        starts = None
    else:
        B, G, P, L, T, sub = 3, 5, 3, 42, 15, 11
        dyn = engine.Dynamics(3, util.dyn3d_sd(44), L)
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 4, T, 512, sub, max_objects=2, contraction_dtype=dtype)
        gd.set_objects(torch.stack([synth.synth_object_3d(31), synth.synth_object_3d(8)]).to(dev))
        torch.manual_seed(3)
        st = sampler.StartStream(512, sub)
        starts = np.concatenate([st.call(gd.rows), st.call(gd.rows)])
    x = torch.stack([synth.synth_noise(60 + i, B, L) for i in range(2)]).clamp(-1, 1).reshape(2, B, L).to(dev)
    return gd, x, starts


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_field_equals_named_objective_and_rowcoef_bitwise(dev, kind, dtype):
    """With lin = quad = 0 the seed is the field value itself: a constant field (-1, 0, 0) gives rotate_clockwise's bits, (1, 0, -1)
    counterclockwise_left's, and a field whose column 0 is the 'convergence' row coefficients gives that objective's - in every trunk,
    2-D and 3-D, both chains of one launch reading their own field rows."""
    gd, x, starts = _case(kind, dev, dtype)
    R = gd.rows
    named = [engine.make_objective('rotate_clockwise', 0), engine.make_objective('counterclockwise_left', 1)]
    want = gd.grad(x, 6, named, None, starts)
    field = torch.empty((2, R, 3), dtype=torch.float32, device=dev)
    field[0] = torch.tensor([-1.0, 0.0, 0.0], device=dev)
    field[1] = torch.tensor([1.0, 0.0, -1.0], device=dev)
    gd.set_row_field(field)
    got = gd.grad(x, 6, [_field_objective(0), _field_objective(1)], None, starts)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)
    # 'convergence': use_rowcoef == 1 reads rowcoef for delta_0 and nothing for the others
    centers = torch.arange(gd.cfg.batch) % gd.cfg.grid_size
    rc = torch.zeros((2, R), dtype=torch.float32)
    rc[1] = torch.from_numpy(gd.rowcoef(centers))
    conv = [engine.make_objective('shift_up', 0), engine.make_objective('convergence', 1)]
    want = gd.grad(x, 6, conv, rc.to(dev), starts)
    field = torch.zeros((2, R, 3), dtype=torch.float32)
    field[1, :, 0] = rc[1]
    gd.set_row_field(field.to(dev))
    got = gd.grad(x, 6, [conv[0], _field_objective(1)], None, starts)
    assert float(want[1].abs().max()) > 0 and torch.equal(got, want)
    gd.set_row_field(None)
    assert torch.equal(gd.grad(x, 6, conv, rc.to(dev), starts), want)


@pytest.mark.parametrize("dtype", ["f32", "f32_mfma"])
def test_mixed_launch_2d_against_autograd(dev, dtype):
    """A named objective, 'convergence' (rowcoef), a random field and a random field + lin + quad in one launch, on the shapes, seeds,
    objects, x and t of test_dyn2d_cond_fn_oracle_multichain (63 cells: a ragged last tile, which the LAST chain's field rows end in - the
    field tensor is exactly [4][R][3]) against torch.autograd over the oracle's forward.  Same tolerance and tie allowance as that test:
    the ReLU pattern depends on (x, object, t), which are its chains 0, 4, 1 and 2."""
    nv, B, G, P, L, T = 100, 5, 7, 3, 14, 15
    sd = util.dyn2d_sd(77, nv)
    dyn = engine.Dynamics(2, sd, L, 2 * nv)
    objs = [synth.synth_object_2d(i, nv) for i in range(3)]
    gd = _guid2d(dyn, B, G, P, (-1.0, 1.0), T, nv, objs, dev, max_chains=6)
    gd.set_contraction_dtype(dtype)
    s = util.setup('point', None, sd, T, 5, L, G, P)
    R = gd.rows
    centers = torch.tensor([2, 0, 6, 3, 1])
    lin, quad = (0.25, -0.5, 0.125), (0.5, 0.0, -0.25)
    chains = [(0, 50, 'rotate'), (0, 54, 'convergence'), (1, 51, 'field'), (2, 52, 'field+')]
    xs = torch.stack([synth.synth_noise(seed, B, L).clamp(-1, 1) for _, seed, _ in chains])
    field = torch.randn((4, R, 3), generator=torch.Generator().manual_seed(9))
    rc = np.zeros((4, R), np.float32)
    rc[1] = gd.rowcoef(centers)
    objectives = [engine.make_objective('rotate', 0), engine.make_objective('convergence', 0), _field_objective(1), _field_objective(2, lin, quad)]
    gd.set_row_field(field.to(dev))
    gr = gd.grad(xs.reshape(4, B, L).to(dev), 6, objectives, torch.from_numpy(rc).to(dev)).cpu()
    t = torch.full((B,), 6, dtype=torch.int64)
    ties = 0
    for c, (oi, _, o) in enumerate(chains):
        if o.startswith('field'):
            ref = goal_oracle.cond_fn_field(s, xs[c], t, objs[oi], field[c], *((lin, quad) if o == 'field+' else ()))
        else:
            ref = orc.cond_fn(s, xs[c], t, o, objs[oi], (-1.0, 1.0), centers if o == 'convergence' else None)
        err = util.finger_err(gr[c].reshape(B, L, 1), ref).sort().values
        norm = float(ref.double().norm())
        print(f"{dtype} chain {c} ({o}): rel err {float(err.norm()) / norm:.3e}")
        if float(err.norm()) / norm < REL:
            continue
        ties += 1
        assert float(err[:-1].norm()) / norm < REL and float(err[-1]) / norm < 1e-3, (c, o, err / norm)
    assert ties <= 1, ties


def test_mixed_launch_3d_against_autograd(dev):
    """The same four kinds of chain in 3-D on the set-up of test_dyn3d_cond_fn_oracle_fps_paths (seed 44, objects 31 and 32 with exact
    duplicate points, sub = 11, N = 512) at B = 3, G = 5, P = 3: 45 cells = two tiles per finger, R = 135 rows, not a multiple of sub.  The
    reference is torch.autograd over the oracle's forward on the logged FPS starts (goal_oracle.mixed3d_reference through orc.StartLog);
    its 540 PointNet++ evaluations take the CPU half a minute, so they are read from tests/golden/goal_mixed3d.npz, which carries the
    inputs it was made from - checked here against the ones the test draws."""
    c = goal_oracle.mixed3d_case()
    B, L, R = c["B"], c["L"], c["R"]
    gold = np.load(goal_oracle.GOLDEN_3D)
    assert np.array_equal(gold["starts"], c["starts"]) and np.array_equal(gold["x"], c["x"].numpy()) and np.array_equal(gold["field"], c["field"].numpy())
    dyn = engine.Dynamics(3, c["sd"], L)
    gd = engine.Guidance(dyn, B, c["G"], c["P"], (-1.0, 1.0), 4, c["T"], 512, c["sub"], max_objects=2)
    gd.set_objects(c["objs"].to(dev))
    rc = np.zeros((4, R), np.float32)
    rc[1] = gd.rowcoef(c["centers"])
    objectives = [engine.make_objective('rotate', 0), engine.make_objective('convergence', 1), _field_objective(1), _field_objective(0, c["lin"], c["quad"])]
    gd.set_row_field(c["field"].to(dev))                       # exactly [4][R][3]: the last chain's last tile is ragged
    gr = gd.grad(c["x"].reshape(4, B, L).to(dev), c["t"], objectives, torch.from_numpy(rc).to(dev), c["starts"]).cpu()
    for k, (oi, o) in enumerate(c["chains"]):
        e = util.rel_l2(gr[k].reshape(B, L, 1), gold["grads"][k])
        print(f"3-D chain {k} ({o}): rel err {e:.3e}")
        assert e < REL, (k, o, e)


def test_loop_equals_steps_with_field_chains(dev):
    """dgdm_guided_chains_run with n_grad = 2 gradients for each of n_chains = 2 chains over three steps, every gradient chain a field
    chain with its own field rows (gradient j of chain k reads field[j * n_chains + k]; one of them with lin / quad besides), against
    the same loop driven step by step: bit-identical (the template is test_native_loop_equals_step_by_step)."""
    nv, B, G, P, L, T = 100, 3, 7, 3, 14, 15
    net = engine.Unet1d(util.unet_sd(11))
    dyn = engine.Dynamics(2, util.dyn2d_sd(22, nv), L, 2 * nv)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 8, T, nv, 0, max_objects=4)
    gd.set_objects(torch.stack([synth.synth_object_2d(i, nv) for i in range(4)]).to(dev))
    s = sched(T, 3)
    K, n_grad = 2, 2
    field = torch.randn((n_grad * K, gd.rows, 3), generator=torch.Generator().manual_seed(12)).to(dev)
    gd.set_row_field(field)
    objectives = [_field_objective(0), _field_objective(1, (0.5, 0.0, -0.5), (0.0, 0.25, 0.0)), _field_objective(2), _field_objective(3)]
    noise = synth.synth_noise(0, B, L).to(dev)
    ts = [int(t) for t in s.timesteps]
    scale = 0.05
    a = engine.guided_chains_run(net, gd, noise.reshape(B, L), K, n_grad, objectives, None, None, ts, [s.coefficients(t) for t in ts], [scale] * K)
    x = noise.reshape(1, B, L).expand(K, -1, -1).contiguous()
    for t in ts:
        eps = net.forward(x.reshape(K * B, L, 1), torch.full((K * B,), t, dtype=torch.int32, device=dev)).reshape(K, B, L)
        g = gd.grad(x.repeat(n_grad, 1, 1), t, objectives, None)
        x = engine.ddim_guided_step(x, eps, g, n_grad, s.coefficients(t), scale)
    assert torch.equal(a, x)
    # the gradient chains do read different rows: with the field's chain blocks swapped the result moves
    gd.set_row_field(field.flip(0).contiguous())
    b = engine.guided_chains_run(net, gd, noise.reshape(B, L), K, n_grad, objectives, None, None, ts, [s.coefficients(t) for t in ts], [scale] * K)
    assert not torch.equal(a, b)


@pytest.mark.parametrize("ori_range", [(-1.0, 1.0), (-0.5, 0.25)])
def test_goal_field_against_numpy_exact(dev, ori_range):
    """dgdm_guidance_goal_field against its numpy restatement on the oracle's own pose rows, bit for bit: both profiles, per-finger
    goals - one on a grid value (pull exactly zero there under 'sign'), one that needs the wrap (u0 beyond +-1), one off the grid -, a
    weight of 0, windows that cut the grid, the full and a partial ori_range."""
    nv, B, G, P, L, T = 100, 3, 8, 3, 14, 15
    dyn = engine.Dynamics(2, util.dyn2d_sd(77, nv), L, 2 * nv)
    gd = engine.Guidance(dyn, B, G, P, ori_range, 4, T, nv, 0, max_objects=1)
    s = util.setup('point', None, None, T, 5, L, G, P)
    grid = goal_oracle.linspace_f32(ori_range[0], ori_range[1], G)      # the handle's grid values (a last bit from torch.linspace's at some entries)
    goals = torch.tensor([[[float(grid[2]), 0.0, -1.0], [0.9, 0.3, -0.7], [-0.95, -1.5, 0.2]],
                          [[0.9, 0.3, -0.7], [float(grid[5]), 1.0, 0.0], [0.123, 0.0, 0.0]],
                          [[-1.0, 0.5, 0.5], [1.0, -0.5, 0.25], [0.0, 0.0, 2.5]]], dtype=torch.float32)
    specs = [((1.0, 0.5, -2.0), 0.5, 1.0, 0), ((0.75, 0.0, 1.5), 0.3, 0.6, 1), ((0.0, 1.0, 1.0), 1.0, 2.5, 0)]
    got = gd.goal_field(goals, [_lib.GoalSpec((C.c_float * 3)(*w), ow, pw, pr) for w, ow, pw, pr in specs]).cpu().numpy()
    want = goal_oracle.goal_field(s, B, ori_range, goals.numpy(), specs)
    assert got.shape == (3, gd.rows, 3) and np.array_equal(got, want)
    assert np.any(want[0] != 0) and np.any(want[1] != 0) and np.all(want[2][:, 0] == 0)
    if ori_range == (-1.0, 1.0):
        # the wrap: finger 1 of chain 0 has its goal at ori 0.9; the rows at ori = -1 are 0.1 away the short way round (pull backwards)
        rows = want[0].reshape(G, P, P, B, 3)
        assert rows[0, 0, 0, 1, 0] == -1.0 and rows[G - 1, 0, 0, 1, 0] == -1.0 and rows[G - 2, 0, 0, 1, 0] == 1.0
        assert rows[2, 0, 0, 0, 0] == 0.0 and rows[1, 0, 0, 0, 0] == 1.0 and rows[3, 0, 0, 0, 0] == -1.0      # on the grid value: no pull under 'sign'
    # the same through sampler.Goal (what guided_chains hands the library) and its host restatement
    goal = sampler.Goal.per_finger(goals[1], weight=specs[1][0], ori_window=specs[1][1], pos_window=specs[1][2], profile='linear')
    _, field = sampler.chain_objectives(gd, [(0, 'rotate'), (0, goal)])
    assert field.shape == (2, gd.rows, 3) and not field[0].any() and np.array_equal(field[1].cpu().numpy(), want[1])
    assert np.array_equal(goal.field(B, G, P, ori_range).numpy(), want[1])


def test_goal_chains_through_the_sampler(dev):
    """A Goal chain with zero weights equals the unguided sample bit for bit (the guided step with a zero gradient is the unguided step);
    the library loop equals the traced loop for Goal chains, alone and beside named and 'convergence' chains, 2-D and 3-D; the default
    scale is 'convergence''s and Goal.scale overrides it."""
    net = engine.Unet1d(util.unet_sd(11))
    for mode in ('point', 'point_3d'):
        if mode == 'point':
            nv, B, G, P, L, T, sub = 100, 3, 7, 3, 14, 15, 0
            dyn = engine.Dynamics(2, util.dyn2d_sd(22, nv), L, 2 * nv)
            objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(2)])
        else:
            nv, B, G, P, L, T, sub = 512, 2, 4, 2, 42, 15, 9
            dyn = engine.Dynamics(3, util.dyn3d_sd(33), L)
            objs = torch.stack([synth.synth_object_3d(i) for i in (1, 8)])
        gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 4, T, nv, sub, max_objects=2)
        gd.set_objects(objs.to(dev))
        s = sched(T, 5)
        noise = synth.synth_noise(0, B, L).to(dev)
        ug = sampler.unguided_sample(net, s, noise)
        torch.manual_seed(4)
        zero = sampler.guided_chains(net, gd, s, mode, noise, [(1, sampler.Goal(ori=0.25, weight=(0.0, 0.0, 0.0)))])
        d = finger_l2(zero[0].cpu(), ug.cpu())
        print(f"{mode}: zero-weight Goal chain vs unguided sample: finger L2 {d:.3e}, bitwise {torch.equal(zero[0], ug)}")
        assert torch.equal(zero[0], ug), (mode, d)
        goal = sampler.Goal.from_physical(200.0, 0.01, -0.005, weight=(1.0, 0.5, 0.5), profile='linear')
        chains = [(0, goal), (1, 'convergence'), (1, sampler.Goal(ori=-0.5, scale=0.01)), (0, 'shift_up')]
        torch.manual_seed(4)
        a = sampler.guided_chains(net, gd, s, mode, noise, chains, unguided=ug)
        torch.manual_seed(4)
        tr = []
        b = sampler.guided_chains(net, gd, s, mode, noise, chains, unguided=ug, trace=tr)
        assert torch.equal(a, b), mode
        assert float(tr[0][1][0].abs().max()) > 0 and float(tr[0][1][2].abs().max()) > 0 and not torch.equal(a[0], ug)
        assert sampler.chain_scale(mode, goal) == sampler.classifier_scale(mode, 'convergence') and sampler.chain_scale(mode, chains[2][1]) == 0.01
        torch.manual_seed(5)
        a = sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1], goal)
        torch.manual_seed(5)
        b = sampler.guided_multi_object(net, gd, s, mode, noise, [0, 1], goal, on_step=lambda i, x: None)
        assert torch.equal(a, b) and not torch.equal(a, ug), mode
        assert gd._row_field is None                               # a launch's field does not outlive it on the handle
        with pytest.raises(ValueError, match="scales differ"):     # one scale per launch of averaged gradients: Goals must agree on it
            sampler.guided_multi_object_groups(net, gd, s, mode, noise, [[0, 1], [1, 0]], [goal, chains[2][1]])


def test_row_field_and_goal_errors(dev):
    """What the library refuses, each with DGDM_EINVAL and a message before anything is launched: a field chain with no field set, a field
    set for fewer chains than the chain's index, a use_rowcoef outside 0 .. 2, windows out of range, an unknown profile, a non-finite goal
    or weight.  The handle works afterwards."""
    gd, x, _ = _case(2, dev, "f32")
    R = gd.rows
    two = [engine.make_objective('rotate', 0), _field_objective(1)]
    with pytest.raises(DgdmError, match=r"error -1: .*chain 1 uses the row field but none is set"):
        gd.grad(x, 6, two, None)
    gd.set_row_field(torch.zeros((1, R, 3), dtype=torch.float32, device=dev))
    with pytest.raises(DgdmError, match=r"error -1: .*chain 1 uses the row field, which was set for 1 chains"):
        gd.grad(x, 6, two, None)
    net = engine.Unet1d(util.unet_sd(11))
    s = sched(15, 2)
    with pytest.raises(DgdmError, match=r"error -1: .*set for 1 chains"):
        engine.guided_chains_run(net, gd, x[0], 1, 2, [_field_objective(0), _field_objective(1)], None, None, [int(t) for t in s.timesteps],
                                 [s.coefficients(int(t)) for t in s.timesteps], [0.1])
    gd.set_row_field(None)
    with pytest.raises(DgdmError, match=r"error -1: .*none is set"):
        gd.grad(x, 6, two, None)
    bad = engine.make_objective('rotate', 0)
    bad.use_rowcoef = 3
    with pytest.raises(DgdmError, match=r"error -1: .*use_rowcoef 3"):
        gd.grad(x[:1], 6, [bad], None)
    with pytest.raises(ValueError, match="set_row_field"):
        gd.set_row_field(torch.zeros((1, R + 1, 3), dtype=torch.float32, device=dev))
    with pytest.raises(DgdmError, match=r"error -1: .*n_chains 5 outside"):
        gd.set_row_field(torch.zeros((5, R, 3), dtype=torch.float32, device=dev))
    goals = torch.zeros((1, gd.cfg.batch, 3))
    spec = lambda w=(1.0, 0.0, 0.0), ow=0.5, pw=1.0, pr=0: [_lib.GoalSpec((C.c_float * 3)(*w), ow, pw, pr)]      # noqa: E731
    for kw, msg in ((dict(ow=0.0), "ori_window"), (dict(ow=1.5), "ori_window"), (dict(ow=float("nan")), "ori_window"), (dict(pw=0.0), "pos_window"),
                    (dict(pw=-1.0), "pos_window"), (dict(pw=float("inf")), "pos_window"), (dict(pr=2), "profile"), (dict(w=(1.0, float("nan"), 0.0)), "weight")):
        with pytest.raises(ValueError, match=msg):
            gd.goal_field(goals, spec(**kw))
    nan = goals.clone()
    nan[0, 1, 2] = float("nan")
    with pytest.raises(ValueError, match=r"goal 0, finger 1: coordinate 2 is not finite"):
        gd.goal_field(nan, spec())
    assert gd.goal_field(goals, spec(ow=1.0)).shape == (1, R, 3)
    want = gd.grad(x, 6, [engine.make_objective('rotate', 0), engine.make_objective('shift_up', 1)], None)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0


def test_predicted_goal_scores(dev, tmp_path):
    """PredictedSimulator(rollout_interactions=3) + goal_objective: keys, dtypes and ranges; and Diffusion.guided_sample /
    guided_sample_multi_object with a Goal return the same bits with the predicted tables on and off, and fill the tables' rows."""
    from dgdm_amd.dynamics import metrics, predicted
    from tests.test_gpu_api import _diffusion
    B, G, P, L, nv = 3, 6, 3, 14, 100
    objs = torch.stack([synth.synth_object_2d(i, nv) for i in range(2)])
    d, s = _diffusion('point', dev, B, G, P, L, objs)
    goal = sampler.Goal.from_physical(30.0, 0.0, 0.0)
    # Diffusion.cond_fn / deltas_to_objective with a Goal: the oracle's autograd over the goal's own field
    pull = sampler.Goal.from_physical(200.0, 0.01, -0.005, weight=(1.0, 0.5, -0.5), profile='linear')
    x, t = synth.synth_noise(9, B, L).clamp(-1, 1), torch.full((B,), 6, dtype=torch.int64)
    got = d.cond_fn(x.to(dev), t.to(dev), opt_obj=pull, object_vertices=objs[1], ori_range=[-1.0, 1.0])
    own = torch.zeros((1, B * G * P * P, 3), dtype=torch.float32, device=dev)
    handle = d._guidance_for(B, [-1.0, 1.0], objs[1].reshape(1, *objs[1].shape[-2:]), 1)
    handle.set_row_field(own)                                   # a field the caller set survives a Goal call on the same handle
    got = d.cond_fn(x.to(dev), t.to(dev), opt_obj=pull, object_vertices=objs[1], ori_range=[-1.0, 1.0])
    assert got.shape == x.shape and util.rel_l2(got.cpu(), goal_oracle.cond_fn_field(s, x, t, objs[1], pull.field(B, G, P))) < REL
    assert d._guidance_for(B, [-1.0, 1.0], objs[1].reshape(1, *objs[1].shape[-2:]), 1) is handle and handle._row_field is own
    handle.set_row_field(None)
    deltas = torch.randn((B * G * P * P, 3), generator=torch.Generator().manual_seed(1))
    assert torch.equal(d.deltas_to_objective(deltas, pull), (deltas * pull.field(B, G, P)).sum(dim=-1))
    sim = predicted.PredictedSimulator(d, rollout_interactions=3)
    samples = synth.synth_noise(2, B, L).clamp(-1, 1).numpy()
    num_rot = 24
    out = sim(samples, [0, 1], None, num_rot=num_rot, ori_range=(-1.0, 1.0))
    assert len(out[1]) == 2 * B
    for m in out[1]:
        o = predicted.goal_objective(m, goal)
        assert set(o) == {'goal_basin_3deg', 'goal_basin_5deg', 'goal_basin_10deg', 'goal_error_deg', 'goal_pos_error_cm', 'predicted'}
        assert o['predicted'] is True and all(o[f'goal_basin_{k}deg'].dtype == np.int16 for k in (3, 5, 10))
        assert 0 <= o['goal_basin_3deg'] <= o['goal_basin_5deg'] <= o['goal_basin_10deg'] <= num_rot
        assert isinstance(o['goal_error_deg'], float) and 0.0 <= o['goal_error_deg'] <= 180.0 and o['goal_pos_error_cm'] >= 0.0
        assert metrics.metric2objective(m, goal) == o
    one = predicted.PredictedSimulator(d)(samples, [0], None, num_rot=num_rot, ori_range=(-1.0, 1.0))[1][0]
    with pytest.raises(ValueError, match="no settled pose"):
        predicted.goal_objective(one, goal)
    noise = synth.synth_noise(0, B, L).to(dev)
    runs = {}
    for tag in ("off", "on"):
        d.simulator = sim if tag == "on" else None
        save = str(tmp_path / tag)
        runs[tag] = (d.guided_sample(0, B, noise, save, opt_obj=goal).cpu(), d.guided_sample_multi_object(0, B, noise, save, opt_obj=goal).cpu())
    assert torch.equal(runs["on"][0], runs["off"][0]) and torch.equal(runs["on"][1], runs["off"][1])
    assert runs["on"][0].shape == (2, B, L, 1) and runs["on"][1].shape == (B, L, 1)
    tables = sorted(os.listdir(tmp_path / "on" / "tables"))
    assert len(tables) == 2 and all("goal_30.0deg" in t for t in tables), tables
    for t in tables:
        tab = json.load(open(tmp_path / "on" / "tables" / t))
        oc = tab["columns"].index("objective")
        scores = [row[oc] for row in tab["data"] if isinstance(row[oc], dict) and row[oc].get("predicted")]
        assert scores and all("goal_basin_5deg" in sc for sc in scores), t


def test_goal_pose_flag_end_to_end(dev, tmp_path):
    """--goal_pose adds multi/goal_... and guided/goal_... behind the sweep's entries and leaves every other output as it is."""
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    common = ("--mode=test --classifier_guidance --object_max_num_vertices=100 --ctrlpts_dim=14 --num_fingers=2 --batch_size=2 --grid_size=3 "
              "--num_pos=3 --num_train_timesteps=15 --num_inference_steps=2")
    torch.manual_seed(7)
    _, plain = train(parse(shlex.split(common)))
    torch.manual_seed(7)
    _, goal = train(parse(shlex.split(common + " --goal_pose=30,0.5,-0.5 --goal_weight=1,0.5,0.5 --goal_profile=linear")))
    keys, gkeys = list(plain[0].keys()), list(goal[0].keys())
    assert gkeys[:len(keys)] == keys and gkeys[len(keys):] == ["multi/goal_30.0deg_0.50_-0.50cm", "guided/goal_30.0deg_0.50_-0.50cm"]
    for k in keys:
        if isinstance(plain[0][k], torch.Tensor):
            assert torch.equal(plain[0][k], goal[0][k]), k
    assert bool(torch.isfinite(goal[0][gkeys[-1]]).all()) and not torch.equal(goal[0][gkeys[-1]][0], goal[0]["unguided"])
