"""Layer 1's object part from a table (the tabled front of the f16x3 gradient trunk, csrc/trunk_f16l.hip) changes no bit.

A chain whose object has no crowded centre and no tie-flagged start reads its embedding as M0[q]; set_objects builds, per such object,
what layer 1's object contraction returns for each of the N rows M0[q], and the trunk takes those chains through a front that looks
the result up.  The reference in every case is the same call with the general front: a handle created under DGDM_L1TAB=0 (no tables)
and debug_fps_path modes 3 and 1 (materialised rows, which never take the table).  N = 512, L = 42; objects from dgdm_amd.synth:
1 and 7 uncrowded, 2 and 8 crowded."""
import os

import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd.scheduler import DDIMScheduler
from tests import util

pytestmark = pytest.mark.gpu
L, T, N = 42, 15, 512
NAMED = ('rotate', 'shift_up', 'clockwise_left', 'shift_down')


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dyn(dev):
    return engine.Dynamics(3, util.dyn3d_sd(44), L)


@pytest.fixture(scope="module")
def crowded_counts(dev, dyn):
    """Crowded centres of the synthetic objects used here (the index decisions of the library's own PointNet++ pipeline)."""
    return {i: int(engine.debug_pointnet_indices(dyn, synth.synth_object_3d(i).to(dev))["crowded"].sum()) for i in (1, 2, 7, 8)}


def _guidance(dyn, B, G, P, nc, sub, max_objects, **env):
    """A handle created with `env` set (the switches are read at creation)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, N, sub, max_objects=max_objects)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _x(nc, B, dev, seed=70):
    return torch.stack([synth.synth_noise(seed + i, B, L) for i in range(nc)]).clamp(-1, 1).reshape(nc, B, L).to(dev)


def _starts(gd, nc, seed=5):
    torch.manual_seed(seed)
    st = sampler.StartStream(N, gd.cfg.sub_batch_size)
    return np.concatenate([st.call(gd.rows) for _ in range(nc)])


def _objectives(gd, nc, dev, order=None):
    """Named objectives, a row-field objective on every third chain (its field set on the handle), object = the chain's number or order[i]."""
    field = torch.from_numpy(np.random.RandomState(9).standard_normal((nc, gd.rows, 3)).astype(np.float32)).to(dev)
    gd.set_row_field(field)
    out = []
    for i in range(nc):
        o = i if order is None else order[i]
        out.append(engine.make_objective(None, o, row_field=True, lin=(0.25, -0.5, 1.0), quad=(0.5, 0.0, -0.25)) if i % 3 == 2
                   else engine.make_objective(NAMED[i % len(NAMED)], o))
    return out


def _same_everywhere(gd, ref, x, timesteps, starts, dev, order=None):
    """gd.grad on the default path against the handle without tables and against gd's own materialised rows, bit for bit."""
    nc = x.shape[0]
    for t in timesteps:
        got = gd.grad(x, t, _objectives(gd, nc, dev, order), None, starts).cpu()
        assert float(got.abs().max()) > 0
        assert torch.equal(got, ref.grad(x, t, _objectives(ref, nc, dev, order), None, starts).cpu()), ("DGDM_L1TAB=0", t)
        for mode in (3, 1):
            gd.debug_fps_path(mode)
            try:
                assert torch.equal(got, gd.grad(x, t, _objectives(gd, nc, dev, order), None, starts).cpu()), (mode, t)
            finally:
                gd.debug_fps_path(0)


def _pair(dyn, B, G, P, nc, sub, objs, max_objects=None):
    mo = max_objects or objs.shape[0]
    gd, ref = _guidance(dyn, B, G, P, nc, sub, mo), _guidance(dyn, B, G, P, nc, sub, mo, DGDM_L1TAB=0)
    gd.set_objects(objs)
    ref.set_objects(objs)
    return gd, ref


def test_all_tabled_workgroups(dev, dyn, crowded_counts):
    """64 cells: 2 tiles per finger, 4 per chain - every workgroup of the tabled launch is full; three kinds of objective, two timesteps.
    (Object 1 has no tie-flagged start; object 7, as uncrowded, may have some and then keeps the gather: not asserted.)"""
    assert crowded_counts[1] == 0 and crowded_counts[7] == 0
    B, G, P, sub = 2, 16, 2, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 7)]).to(dev)
    gd, ref = _pair(dyn, B, G, P, 3, sub, objs)
    assert gd.debug_fps_path(0)[0]
    x = _x(3, B, dev)
    _same_everywhere(gd, ref, x, (3, 11), _starts(gd, 3), dev, order=(0, 1, 0))


@pytest.mark.parametrize("reverse", [False, True])
def test_straddling_workgroups_and_padding_rows(dev, dyn, crowded_counts, reverse):
    """45 cells: the finger's second tile holds 13 valid rows; 6 tiles per chain, tabled and gathered chains alternate, and the 30 tiles
    are no multiple of 4 (a last workgroup has waves without a tile); the chain order once reversed."""
    assert crowded_counts[2] > 0 and crowded_counts[8] > 0
    B, G, P, sub = 3, 5, 3, 64
    ids = (1, 2, 7, 8, 1)[::-1] if reverse else (1, 2, 7, 8, 1)
    objs = torch.stack([synth.synth_object_3d(i) for i in ids]).to(dev)
    gd, ref = _pair(dyn, B, G, P, 5, sub, objs)
    assert (gd.cfg.grid_size * gd.cfg.num_pos ** 2) % 32 == 13 and (5 * B * 2) % 4 != 0
    _same_everywhere(gd, ref, _x(5, B, dev), (6,), _starts(gd, 5), dev)


def test_tabled_launch_with_idle_waves(dev, dyn):
    """One tabled chain of 6 tiles between two gathered ones: the last workgroup of the tabled chains' launch has two waves without a tile."""
    B, G, P, sub = 3, 5, 3, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (2, 1, 8)]).to(dev)
    gd, ref = _pair(dyn, B, G, P, 3, sub, objs)
    assert gd.debug_fps_path(0)[1] and (B * 2) % 4 != 0
    _same_everywhere(gd, ref, _x(3, B, dev), (9,), _starts(gd, 3), dev)


def _dup(i):
    """Rows 9 and 10 overwritten by row 400: bit-identical points are interchangeable in FPS, not a tie - the object stays eligible."""
    o = synth.synth_object_3d(i).clone()
    o[9] = o[400]
    o[10] = o[400]
    return o


def _mirrored(i):
    """Point-symmetric about the origin: different points at exactly equal distances, so most starts carry a tie flag.  Uncrowded, and
    still gathered: not eligible."""
    o = synth.synth_object_3d(i).clone()
    o[256:] = -o[:256]
    return o


def test_eligibility_edges(dev, dyn):
    B, G, P, sub = 2, 12, 3, 64
    clouds = [_dup(1), _mirrored(1), synth.synth_object_3d(1)]
    for c in clouds:
        assert int(engine.debug_pointnet_indices(dyn, c.to(dev))["crowded"].sum()) == 0
    objs = torch.stack(clouds).to(dev)
    gd, ref = _pair(dyn, B, G, P, 3, sub, objs)
    assert gd.debug_fps_path(0) == [True, False, True]
    _same_everywhere(gd, ref, _x(3, B, dev), (4,), _starts(gd, 3), dev)


def test_stale_tables(dev, dyn):
    """Crowded, uncrowded, crowded objects in the same slots of one handle; then a handle with more slots than objects."""
    B, G, P, sub = 2, 12, 3, 64
    sets = [(2, 8), (1, 7), (8, 1), (2, 8)]
    first = torch.stack([synth.synth_object_3d(i) for i in sets[0]]).to(dev)
    gd, ref = _pair(dyn, B, G, P, 2, sub, first)
    x, starts = _x(2, B, dev), _starts(gd, 2)
    for ids in sets:
        objs = torch.stack([synth.synth_object_3d(i) for i in ids]).to(dev)
        gd.set_objects(objs)
        ref.set_objects(objs)
        _same_everywhere(gd, ref, x, (7,), starts, dev)
    objs = torch.stack([synth.synth_object_3d(i) for i in (7, 2)]).to(dev)
    gd, ref = _pair(dyn, B, G, P, 2, sub, objs, max_objects=5)
    _same_everywhere(gd, ref, x, (7,), starts, dev)


def test_denoise_loop(dev, dyn):
    """Five denoise steps on the mixed set: the default handle, one without tables, one on the serial step schedule."""
    B, G, P, sub = 2, 12, 3, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 2, 7, 8)]).to(dev)
    net = engine.Unet1d(util.unet_sd(11))
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(5)
    noise = synth.synth_noise(0, B, L).to(dev)
    ug = sampler.unguided_sample(net, s, noise)
    chains = [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left'), (3, 'rotate')]
    ends = []
    for env in ({}, {"DGDM_L1TAB": 0}, {"DGDM_SERIAL_STEP": 1}):
        gd = _guidance(dyn, B, G, P, 4, sub, 4, **env)
        gd.set_objects(objs)
        torch.manual_seed(4)
        ends.append(sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, unguided=ug).cpu())
    assert float((ends[0] - ug.cpu()).abs().max()) > 0
    assert torch.equal(ends[0], ends[1])
    assert torch.equal(ends[0], ends[2])


def test_same_bits_every_run(dev, dyn):
    """The same call twice on the tabled path (a missed hazard behind inline assembly shows as run-to-run differences)."""
    B, G, P, sub = 2, 16, 2, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 7)]).to(dev)
    gd = _guidance(dyn, B, G, P, 2, sub, 2)
    gd.set_objects(objs)
    x, starts = _x(2, B, dev), _starts(gd, 2)
    a = gd.grad(x, 5, _objectives(gd, 2, dev), None, starts).cpu()
    for _ in range(3):
        assert torch.equal(a, gd.grad(x, 5, _objectives(gd, 2, dev), None, starts).cpu())


def test_wide_channel_range(dev):
    """A checkpoint whose first trunk layer has rows 2^20 above and 2^-18 below the rest: the stored row scale and scaled accumulators
    survive the equilibration and large row scales."""
    sd = util.dyn3d_sd(45)
    w, b = sd["linears.0.weight"], sd["linears.0.bias"]
    for row, k in ((5, 20), (77, -18), (300, 12), (511, -9)):
        w[row] *= 2.0 ** k
        b[row] *= 2.0 ** k
    w[:, :256] *= 8.0                                     # and the object-embedding columns as a whole
    wide = engine.Dynamics(3, sd, L)
    B, G, P, sub = 2, 12, 3, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 2, 7)]).to(dev)
    gd, ref = _pair(wide, B, G, P, 3, sub, objs)
    _same_everywhere(gd, ref, _x(3, B, dev), (2,), _starts(gd, 3), dev)


@pytest.mark.parametrize("dtype", ["bf16", "f32_mfma"])
def test_other_trunks_take_no_table(dev, dyn, dtype):
    B, G, P, sub = 2, 12, 3, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 2, 7)]).to(dev)
    res = []
    for env in ({}, {"DGDM_L1TAB": 0}):
        gd = _guidance(dyn, B, G, P, 3, sub, 3, **env)
        gd.set_contraction_dtype(dtype)
        gd.set_objects(objs)
        res.append(gd.grad(_x(3, B, dev), 3, _objectives(gd, 3, dev), None, _starts(gd, 3)).cpu())
    assert float(res[0].abs().max()) > 0
    assert torch.equal(res[0], res[1])


def test_score_is_unchanged(dev, dyn):
    """The forward-only kernels keep the general front: the logits of a tabled object's chains with and without the tables."""
    B, G, P, sub = 2, 12, 3, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 7)]).to(dev)
    gd, ref = _pair(dyn, B, G, P, 2, sub, objs)
    x, starts = _x(2, B, dev), _starts(gd, 2)
    a = gd.score(x, (0, 1), (0.1, 0.1, 0.1), 3, starts, want_logits=True)
    b = ref.score(x, (0, 1), (0.1, 0.1, 0.1), 3, starts, want_logits=True)
    assert float(a[2].abs().max()) > 0
    for u, v in zip(a, b):
        assert torch.equal(u.cpu(), v.cpu())
