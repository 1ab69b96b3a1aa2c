"""The 3-D object path computes nothing twice and changes no bit (N = 512, objects from dgdm_amd.synth):

* the sa2/sa3 tables of a default set_objects against the dense build (mode 4: l2_kernel's per-(variant, centre) gathers, every Z row
  from its own L2 row), through gd.grad, and the embedding tables X[s1][q] built from them (mode 5).  Objects 2, 12, 24, 30, 1: 22 % of
  the (variant, centre) selections shared, 98.6 % shared in classes of hundreds, almost none shared, one crowded centre with two
  selections, no crowded centre.  Every variant s1 is drawn (s1 = row mod 512, 16 rows each).
* chains whose object has no crowded centre and no tie-flagged start get no gathered rows: the trunk reads M0[q] through the row index.
  Launches of such chains only, mixed launches, an uncrowded object with exact duplicate points, one WITH tie-flagged starts (which
  keeps the gather), and a 5-step run whose calls share one launch - all bit-equal to the modes that materialise every row (3: group
  gather, 2: per-row table, 1: per-row FPS)."""
import os

import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd.scheduler import DDIMScheduler
from tests import util

pytestmark = pytest.mark.gpu
L, T, N = 42, 15, 512
OBJECTIVES = ('rotate', 'shift_up', 'clockwise_left', 'rotate', 'shift_down')


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dyn(dev):
    return engine.Dynamics(3, util.dyn3d_sd(44), L)


def _inputs(nc, B, dev):
    x = torch.stack([synth.synth_noise(70 + i, B, L) for i in range(nc)]).clamp(-1, 1).reshape(nc, B, L).to(dev)
    return x, [engine.make_objective(OBJECTIVES[i % len(OBJECTIVES)], i) for i in range(nc)]


def _every_variant_starts(nc, rows, sub, seed):
    """The library's draw layout, by hand: per chain and sub-batch the s1 draws, then the s2 draws; s1 = row mod 512."""
    rs = np.random.RandomState(seed)
    out = np.empty((nc, 2 * rows), dtype=np.int64)
    for c in range(nc):
        for r0 in range(0, rows, sub):
            n = min(sub, rows - r0)
            out[c, 2 * r0:2 * r0 + n] = np.arange(r0, r0 + n) % N
            out[c, 2 * r0 + n:2 * r0 + 2 * n] = rs.randint(0, 512, n)
    return out.reshape(-1)


def test_tables_equal_dense_build(dev, dyn):
    B, G, P, sub = 4, 128, 4, 512
    objs = torch.stack([synth.synth_object_3d(i) for i in (2, 12, 24, 30, 1)]).to(dev)
    nc = objs.shape[0]
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, N, sub, max_objects=nc)
    assert gd.rows == 8192
    x, objectives = _inputs(nc, B, dev)
    starts = _every_variant_starts(nc, gd.rows, sub, 3)
    gd.set_objects(objs)
    default = gd.grad(x, 3, objectives, None, starts).cpu()
    gd.debug_fps_path(4)                      # dense rebuild: the reference
    gd.set_objects(objs)
    dense = gd.grad(x, 3, objectives, None, starts).cpu()
    gd.debug_fps_path(5)                      # default tables again, and X[s1][q] built from them right away
    gd.set_objects(objs)
    xtab = gd.grad(x, 3, objectives, None, starts).cpu()
    gd.debug_fps_path(0)
    assert float(dense.abs().max()) > 0
    assert torch.equal(default, dense)
    assert torch.equal(xtab, dense)


def _dup(i):
    """Rows 9 and 10 overwritten by row 400.  Bit-identical points are interchangeable in FPS, not a tie: no start is flagged."""
    o = synth.synth_object_3d(i).clone()
    o[9] = o[400]
    o[10] = o[400]
    return o


def _mirrored(i):
    """Point-symmetric about the origin: DIFFERENT points at exactly equal distances, so most starts carry a tie flag; still uncrowded."""
    o = synth.synth_object_3d(i).clone()
    o[256:] = -o[:256]
    return o


@pytest.mark.parametrize("case", ["uncrowded", "mixed", "uncrowded_dup", "uncrowded_ties"])
def test_uncrowded_chains_skip_the_gather(dev, dyn, case):
    B, G, P, sub = 2, 12, 3, 64
    objs = {"uncrowded": [synth.synth_object_3d(1), synth.synth_object_3d(7)],
            "mixed": [synth.synth_object_3d(i) for i in (1, 2, 7, 8)],
            "uncrowded_dup": [_dup(1), synth.synth_object_3d(1)],
            "uncrowded_ties": [_mirrored(1), synth.synth_object_3d(1)]}[case]
    objs = torch.stack(objs).to(dev)
    nc = objs.shape[0]
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, N, sub, max_objects=nc)
    gd.set_objects(objs)
    ok = gd.debug_fps_path(0)
    # object 1 has no tie-flagged start, with or without the duplicates; the mirrored one has (so may any other object: not asserted)
    known = {"uncrowded": (True, None), "mixed": (True, None, None, None), "uncrowded_dup": (True, True), "uncrowded_ties": (False, True)}[case]
    assert all(k is None or k == o for k, o in zip(known, ok)), ok
    x, objectives = _inputs(nc, B, dev)
    torch.manual_seed(5)
    st = sampler.StartStream(N, sub)
    starts = np.concatenate([st.call(gd.rows) for _ in range(nc)])
    res = {}
    for mode in (0, 3, 2, 1):
        gd.debug_fps_path(mode)
        res[mode] = gd.grad(x, 3, objectives, None, starts).cpu()
    gd.debug_fps_path(0)
    assert float(res[1].abs().max()) > 0
    for mode in (3, 2, 1):
        assert torch.equal(res[0], res[mode]), (case, mode)


def test_mixed_run_shares_one_launch(dev, dyn):
    """Five denoise steps on the mixed set: the calls' rows in one launch (native loop), call by call (trace), in groups of two calls,
    and with every row materialised (mode 3)."""
    B, G, P, sub = 2, 12, 3, 64
    objs = torch.stack([synth.synth_object_3d(i) for i in (1, 2, 7, 8)]).to(dev)
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), 4, T, N, sub, max_objects=4)
    gd.set_objects(objs)
    net = engine.Unet1d(util.unet_sd(11))
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(5)
    noise = synth.synth_noise(0, B, L).to(dev)
    ug = sampler.unguided_sample(net, s, noise)
    chains = [(0, 'rotate'), (1, 'shift_up'), (2, 'clockwise_left'), (3, 'rotate')]

    def run(**kw):
        gd.set_objects(objs)                  # every run starts below the embedding-table policy's call count
        torch.manual_seed(4)
        return sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, unguided=ug, **kw).cpu()
    a = run()
    assert torch.equal(a, run(trace=[]))
    os.environ["DGDM_EMBED_CALLS"] = "2"
    try:
        assert torch.equal(a, run())
    finally:
        os.environ.pop("DGDM_EMBED_CALLS", None)
    gd.debug_fps_path(3)
    try:
        assert torch.equal(a, run())
    finally:
        gd.debug_fps_path(0)
