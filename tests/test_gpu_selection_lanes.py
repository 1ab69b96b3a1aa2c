"""The float32 table build's selection stage with the variants on its lanes, and the rows its classes share (N = 512).

Three clouds made for the edges of that code, beside synth objects 12 (classes of hundreds) and 1 (no crowded centre): a tight cluster
of n points (radius 0.12, centred at x = 0.85: every member lies in every member's r = 0.4 ball, so n centres have K = n) plus points
of a 0.25-spaced lattice in x <= 0.3, jittered by +-0.01 (K <= 19, and no lattice point within 0.4 of the cluster):

* n = 300: the K > 255 path - every variant is its own representative, no row is shared;
* n = 66: selections that differ in only two members - many classes of many variants; from a lattice start the cluster comes last
  in the FPS order, so the scans run to the final positions;
* n = 200: the ball sizes of the heavy bench objects.

The ball sizes are asserted on the CPU with the reference's float32 formula.  Default build against the dense build (mode 4) and the
embedding tables (mode 5) with every variant drawn, and against the modes that materialise every row (3, 2, 1), bit for bit."""
import numpy as np
import pytest
import torch

from dgdm_amd import engine, sampler, synth
from dgdm_amd.scheduler import DDIMScheduler
from tests import util

pytestmark = pytest.mark.gpu
L, T, N = 42, 15, 512
OBJECTIVES = ('rotate', 'shift_up', 'clockwise_left', 'rotate', 'shift_down')
CLUSTERS = (300, 66, 200)


def _cloud(n, seed):
    """n cluster points first, then 512 - n lattice points."""
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cluster = np.array([0.85, 0.0, 0.0]) + d * (0.12 * rs.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0))
    xs = 0.3 - 0.25 * np.arange(6)
    yz = -1.0 + 0.25 * np.arange(9)
    lattice = np.stack(np.meshgrid(xs, yz, yz, indexing="ij"), -1).reshape(-1, 3)
    lattice = np.clip(lattice[rs.permutation(len(lattice))[:N - n]] + rs.uniform(-0.01, 0.01, (N - n, 3)), -1.0, 1.0)
    return torch.from_numpy(np.concatenate([cluster, lattice]).astype(np.float32))


def _ball_sizes(o):
    """Points in every centre's r = 0.4 ball as the reference counts them: float32, -2ab + a^2 + b^2, `> radius ** 2` excluded."""
    d = -2.0 * (o @ o.T)
    d = d + (o * o).sum(-1)[:, None]
    d = d + (o * o).sum(-1)[None, :]
    return (d <= torch.tensor(np.float32(0.4 ** 2))).sum(1)


_cache = {}


def _objects():
    if "o" not in _cache:
        clouds = [_cloud(n, 100 + n) for n in CLUSTERS]
        for n, o in zip(CLUSTERS, clouds):
            k = _ball_sizes(o)
            assert bool((k[:n] == n).all()), (n, k[:n].min(), k[:n].max())
            assert int(k[n:].max()) <= 19, (n, int(k[n:].max()))
        _cache["o"] = torch.stack(clouds + [synth.synth_object_3d(12), synth.synth_object_3d(1)])
    return _cache["o"]


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


def test_ball_sizes_on_the_cpu():
    """The clouds are what the other tests take them for (no GPU work: the assertions sit in _objects)."""
    assert _objects().shape == (5, N, 3)


def test_every_variant_equals_dense_build(dev, dyn):
    B, G, P, sub = 4, 128, 4, 512
    objs = _objects().to(dev)
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


def test_small_grid_equals_materialised_rows(dev, dyn):
    B, G, P, sub = 2, 12, 3, 64
    objs = _objects().to(dev)
    nc = objs.shape[0]
    gd = engine.Guidance(dyn, B, G, P, (-1.0, 1.0), nc, T, N, sub, max_objects=nc)
    gd.set_objects(objs)
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
        assert torch.equal(res[0], res[mode]), mode

    net = engine.Unet1d(util.unet_sd(11))
    s = DDIMScheduler(num_train_timesteps=T)
    s.set_timesteps(5)
    noise = synth.synth_noise(0, B, L).to(dev)
    ug = sampler.unguided_sample(net, s, noise)
    chains = [(i, OBJECTIVES[i]) for i in range(nc)]

    def run():
        gd.set_objects(objs)                  # every run starts below the embedding-table policy's call count
        torch.manual_seed(4)
        return sampler.guided_chains(net, gd, s, 'point_3d', noise, chains, unguided=ug).cpu()
    a = run()
    gd.debug_fps_path(3)
    try:
        b = run()
    finally:
        gd.debug_fps_path(0)
    assert torch.equal(a, b)
