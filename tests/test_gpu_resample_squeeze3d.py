"""Resampling 3-D fingers by the sliced squeeze's objective on the GPU (csrc/squeeze.hip: dgdm_squeeze_values_3d, values3d_pair_kernel and
table3d_fingers_kernel over groups; DESIGN.md 4.3e "potential: squeeze_3d").

The entry's contract is the composition of two entries that exist - dgdm_squeeze_map_3d on the groups' pairs, then
dgdm_squeeze_objective_values on its cells / y - and every operation of both is a basic IEEE float64 or an int32 one in a fixed order.
So everything here is compared bit for bit, as int64 views, with no tolerance and no cell excluded: the values with
engine.squeeze_tables_3d + engine.squeeze_objective_values and with tests/squeeze3d_oracle.squeeze_map_3d +
tests/resample_squeeze_oracle.objective_values; the tables with table3d_kernel's and the oracle's; a chain's run with a replay written
here from those engine calls.

Shapes: tests/test_gpu_squeeze3d.py's 5 non-uniform abscissae, 3 levels, 12 orientations, 9 x cells and four meshes.  Three groups of
`batch` consecutive fingers from fingers 0, 19 and 38 on objects [1, 3, 0], and a fourth that reuses group 0's fingers on object 1;
batch 1, 3, 8, 11, 19 = a tail alone, a smaller tail, one full block of 8, a block and a tail, two blocks and a tail."""
import ctypes as C
import functools
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine, sampler
from dgdm_amd import dist as ddist
from dgdm_amd.dynamics.dataloader import SCORE_STD
from dgdm_amd.resample import Resample, SqueezePotential3D
from dgdm_amd.sim import squeeze
from tests import resample_squeeze_oracle as rso
from tests import squeeze3d_oracle as so3
from tests import squeeze_oracle as so
from tests import test_gpu_resample as tgr
from tests.test_gpu_squeeze3d import GX, GZ, THETA, meshes, ngon, prism, rect, surfaces

pytestmark = pytest.mark.gpu

STD = tuple(float(v) for v in SCORE_STD[0])
ORI = (-1.0, 1.0)
BLOCK, N_FINGERS = 19, 57
GROUP_FIRST, GROUP_OBJECT = [0, 19, 38, 0], [1, 3, 0, 1]
BATCHES = [1, 3, 8, 11, 19]
# (window, closing_steps): three steps in a window of 2, and a run that settles
CONFIGS = {"k3": (2, 3), "settles": (1, 1 << 20)}
# n_starts: (G, P) of the pose grid - 1 start leaves 63 lanes idle, 54 some, 81 are more than one stride of the wave
GRIDS = {1: (1, 1), 54: (6, 3), 81: (9, 3)}
# the groups' objectives: linear ones, 'rotate' (quadratic) among them, 'convergence' (rowcoef) among them
OBJECTIVES = {"linear": ['clockwise_up', 'shift_left', 'counterclockwise_down', 'shift_up'],
              "rotate": ['rotate', 'clockwise_up', 'rotate', 'shift_right'],
              "convergence": ['convergence', 'rotate', 'convergence', 'clockwise_left']}
SENTINEL = -77.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def config(name):
    R, k = CONFIGS[name]
    return dict(theta_cells=THETA, x_cells=9, x_half=0.06, window=R, closing_steps=k, travel_max=0.15)


@functools.lru_cache(maxsize=None)
def fingers():
    return np.stack([surfaces(s) for s in range(1, N_FINGERS + 1)])


def starts_of(n):
    return rso.start_grid(*GRIDS[n], ORI)


ALL_STARTS = {81: slice(0, 81), 54: slice(81, 135), 1: slice(135, 136)}


@functools.lru_cache(maxsize=None)
def oracle_map(name):
    """tests/squeeze3d_oracle.squeeze_map_3d of the three blocks of 19 fingers on their objects, over all three start grids at once (a
    start's outputs do not depend on the other starts): made once per config, never changed.  Row g * 19 + b = (finger 19 g + b,
    GROUP_OBJECT[g])."""
    cfg = config(name)
    seg, off = so3.slice_meshes(meshes(), GZ)
    pairs = [(GROUP_FIRST[g] + b, GROUP_OBJECT[g]) for g in range(3) for b in range(BLOCK)]
    st = np.concatenate([starts_of(81), starts_of(54), starts_of(1)])
    return so3.squeeze_map_3d(fingers(), GX, seg, off, pairs, so.rotation_table(THETA), st, x_cells=cfg["x_cells"], x_half=cfg["x_half"],
                              window=cfg["window"], closing_steps=cfg["closing_steps"], travel_max=cfg["travel_max"])


def rows_of(batch):
    """The oracle map's rows of the four groups' pairs, group-major (group 3 is group 0's fingers on group 0's object)."""
    return np.concatenate([np.arange(batch) + BLOCK * g for g in (0, 1, 2, 0)])


def pairs_of(batch):
    return [(GROUP_FIRST[g] + b, GROUP_OBJECT[g]) for g in range(4) for b in range(batch)]


def objectives_of(kind):
    return [engine.make_objective(n, GROUP_OBJECT[g]) for g, n in enumerate(OBJECTIVES[kind])]


def rowcoef_of(n_starts, batch):
    return np.random.RandomState(n_starts + batch).choice([-1.0, 0.0, 1.0, 0.5, -2.0], size=(4, n_starts * batch)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def slices():
    return engine.squeeze_slice(meshes(), GZ)


def workspace(name, chunk_groups, batch):
    return int(_lib.lib().dgdm_squeeze_values_3d_workspace_bytes(C.byref(engine.squeeze_config(**config(name))), chunk_groups, batch, len(GX), len(GZ), 4))


def values(dev, name, batch, n_starts, kind, tables=False, **kw):
    sl = slices()
    rc = torch.from_numpy(rowcoef_of(n_starts, batch)).to(dev) if kind == "convergence" else None
    return engine.squeeze_values_3d(fingers(), GX, sl["segments"], sl["offsets"], GROUP_FIRST, batch, objectives_of(kind), starts_of(n_starts), rc, STD,
                                    rot=so.rotation_table(THETA), tables=tables, **config(name), **kw)


# ------------------------------------------------------------------------------------------------ 1. values against the composition
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("n_starts", list(GRIDS))
@pytest.mark.parametrize("batch", BATCHES)
def test_values_equal_the_composition(dev, batch, n_starts, name):
    cfg, sl = config(name), slices()
    st = starts_of(n_starts)
    assert st.shape == (n_starts, 3)
    std = torch.from_numpy(st).to(dev)
    route = engine.squeeze_tables_3d(fingers(), GX, sl["segments"], sl["offsets"], pairs_of(batch), std, rot=so.rotation_table(THETA), **cfg)
    ref_map, idx = oracle_map(name), rows_of(batch)
    cells, y = ref_map["cells"][idx][:, ALL_STARTS[n_starts]], ref_map["y"][idx][:, ALL_STARTS[n_starts]]
    assert np.array_equal(route["cells"].cpu().numpy(), cells) and np.array_equal(bits(route["y"]), bits(y))      # the two yardsticks agree
    for kind in OBJECTIVES:
        objectives = objectives_of(kind)
        rowcoef = rowcoef_of(n_starts, batch) if kind == "convergence" else None
        if kind == "rotate":
            assert any(v != 0 for v in objectives[0].quad) and objectives[0].use_rowcoef == 0
        if kind == "convergence":
            assert objectives[0].use_rowcoef == 1 and objectives[2].use_rowcoef == 1
        rcd = None if rowcoef is None else torch.from_numpy(rowcoef).to(dev)
        want = engine.squeeze_objective_values(route["cells"], route["y"], std, batch, objectives, rcd, STD, **cfg)
        ref = rso.objective_values(cells, y, st, batch, objectives, rowcoef, STD, THETA, cfg["x_cells"], cfg["x_half"])
        got = values(dev, name, batch, n_starts, kind)
        assert got.shape == (4, batch) and got.dtype == torch.float64
        assert np.array_equal(bits(got), bits(want)), (kind, got.cpu().numpy(), want.cpu().numpy())
        assert np.array_equal(bits(got).reshape(-1), bits(ref)), (kind, got.cpu().numpy().reshape(-1), ref)
        assert np.isfinite(ref).all()
        if n_starts > 1 and batch > 1:
            assert len(np.unique(ref)) > batch                      # the case tells fingers and groups apart


def test_the_cases_move(dev):
    """A condition on the inputs: in both configs closed cells differ from the start cells, in theta and in x."""
    for name in CONFIGS:
        c = oracle_map(name)["cells"][:, ALL_STARTS[81]]
        a0, b0, a1, b1 = c[..., 0] // 9, c[..., 0] % 9, c[..., 1] // 9, c[..., 1] % 9
        assert np.count_nonzero(a0 != a1) > 100 and np.count_nonzero(b0 != b1) > 100, name


# ------------------------------------------------------------------------------------------------ 2. tables
@pytest.mark.parametrize("batch", [11, 19])
def test_tables_equal_table3d_kernel_and_the_oracle(dev, batch):
    got, tab = values(dev, "k3", batch, 54, "linear", tables=True)
    sl = slices()
    per_pair = engine.squeeze_tables_3d(fingers(), GX, sl["segments"], sl["offsets"], pairs_of(batch), None, rot=so.rotation_table(THETA), tables=True,
                                        **config("k3"))
    ref, idx = oracle_map("k3"), rows_of(batch)
    for k in ("S", "touch_l", "touch_r"):
        assert tab[k].shape == (4 * batch, THETA, 9)
        assert np.array_equal(bits(tab[k]), bits(per_pair[k])), k
        assert np.array_equal(bits(tab[k]), bits(ref[k][idx])), k
    assert np.isfinite(tab["S"].cpu().numpy()).all() and len(np.unique(tab["S"].cpu().numpy())) > 3 * batch * THETA
    assert np.array_equal(bits(got), bits(values(dev, "k3", batch, 54, "linear")))      # asking for the tables changes no value


def test_a_level_of_more_than_one_segment_tile(dev):
    """tests/test_gpu_squeeze_label3d.py's 300-gon prism: 600 segments on each level, two LDS tiles of the finger-shared kernel, the second
    partly filled; one group of 9 fingers (a full block and a single-finger block)."""
    mesh = [prism(ngon(300, 0.05, 0.2), -0.01, 0.06)]
    seg, off = so3.slice_meshes(mesh, GZ)
    assert (np.diff(off, axis=1) == 600).all()
    cfg = dict(theta_cells=4, x_cells=7, x_half=0.06, window=1, closing_steps=2, travel_max=0.15)
    st = rso.start_grid(4, 2, ORI)
    pairs = [(f, 0) for f in range(9)]
    sf = fingers()[:9]
    ref = so3.squeeze_map_3d(sf, GX, seg, off, pairs, so.rotation_table(4), st, x_cells=7, x_half=0.06, window=1, closing_steps=2, travel_max=0.15)
    sl = engine.squeeze_slice(mesh, GZ)
    objectives = [engine.make_objective('clockwise_up', 0)]
    got, tab = engine.squeeze_values_3d(sf, GX, sl["segments"], sl["offsets"], [0], 9, objectives, st, None, STD, tables=True, **cfg)
    std = torch.from_numpy(st).to(dev)
    route = engine.squeeze_tables_3d(sf, GX, sl["segments"], sl["offsets"], pairs, std, tables=True, **cfg)
    want = engine.squeeze_objective_values(route["cells"], route["y"], std, 9, objectives, None, STD, **cfg)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got).reshape(-1), bits(rso.objective_values(ref["cells"], ref["y"], st, 9, objectives, None, STD, 4, 7, 0.06)))
    for k in ("S", "touch_l", "touch_r"):
        assert np.array_equal(bits(tab[k]), bits(ref[k])), k
        assert np.array_equal(bits(tab[k]), bits(route[k])), k
    assert len(np.unique(got.cpu().numpy())) > 1


# ------------------------------------------------------------------------------------------------ 3. chunking
def test_chunking_changes_no_bit(dev):
    """Workspaces of 1 group, 2 groups, all 4 groups and a size the sizer never returned; the same call twice."""
    batch = 11
    sizes = [workspace("k3", n, batch) for n in (1, 2, 4)]
    assert 0 < sizes[0] < sizes[1] < sizes[2]
    whole, whole_tab = values(dev, "k3", batch, 81, "convergence", tables=True)
    assert len(np.unique(whole.cpu().numpy())) > batch
    for ws in (sizes[0], sizes[1], sizes[2], sizes[1] + 12345, sizes[0] + 1, None, None):
        got, tab = values(dev, "k3", batch, 81, "convergence", tables=True, workspace_bytes=ws)
        assert np.array_equal(bits(got), bits(whole)), ws
        for k in ("S", "touch_l", "touch_r"):
            assert np.array_equal(bits(tab[k]), bits(whole_tab[k])), (ws, k)


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_every_bad_argument_is_refused_before_a_launch(dev):
    lib = _lib.lib()
    mu, mv, N, B = 5, 3, 7, 2
    sf = torch.zeros(5, 2, mv, mu, dtype=torch.float64, device=dev)
    seg = torch.zeros(6, 4, dtype=torch.float64, device=dev)
    rot = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    st = torch.zeros(N, 3, dtype=torch.float64, device=dev)
    rowcoef = torch.zeros(2, N * B, dtype=torch.float32, device=dev)
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device=dev)
    tab = torch.full((4, 8, 5), SENTINEL, dtype=torch.float64, device=dev)
    good = dict(theta_cells=8, x_cells=5, window=1, closing_steps=2, x_half=0.06, travel_max=0.1, finger_half_len=0.12)
    size = lambda: int(lib.dgdm_squeeze_values_3d_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1, B, mu, mv, 3))      # noqa: E731
    ws = torch.empty(2 * size(), dtype=torch.uint8, device=dev)
    nan, inf = float("nan"), float("inf")
    offsets = np.array([[0, 1, 2, 2], [2, 2, 3, 4], [4, 5, 6, 6]], dtype=np.int32)
    plain = [engine.make_objective('rotate', 2), engine.make_objective('shift_up', 0)]
    conv = [engine.make_objective('convergence', 2), engine.make_objective('rotate', 0)]
    field = [engine.make_objective(None, 2, row_field=True), engine.make_objective('rotate', 0)]

    def call(cfg=None, gx=tuple(GX), mu_=mu, mv_=mv, n_seg=6, off=offsets, nf=5, nb=3, surf=sf, segs=seg, n_starts=N, n_groups=2, batch=B,
             first=(3, 0), objectives=plain, rc=None, std=STD, values_=out, ws_b=None, starts=st, rot_=rot, gx_null=False, off_null=False,
             first_null=False, obj_null=False, std_null=False, no_cfg=False):
        c = engine.squeeze_config(**dict(good, **(cfg or {})))
        g = np.array(gx, dtype=np.float64)
        of = np.ascontiguousarray(off, dtype=np.int32)
        gf = np.array(first, dtype=np.int32)
        arr = (_lib.Objective * len(objectives))(*objectives)
        return lib.dgdm_squeeze_values_3d(None if no_cfg else C.byref(c), _lib.dptr(surf), nf, None if gx_null else g.ctypes.data, mu_, mv_,
                                          _lib.dptr(segs), n_seg, None if off_null else of.ctypes.data, nb, _lib.dptr(rot_), _lib.dptr(starts), n_starts,
                                          n_groups, batch, None if first_null else gf.ctypes.data, None if obj_null else arr, _lib.dptr(rc),
                                          None if std_null else (C.c_double * 3)(*std), _lib.dptr(values_), _lib.dptr(tab), None, None, _lib.dptr(ws),
                                          size() if ws_b is None else ws_b, None)

    down = offsets.copy()
    down[1, 1] = 1
    late = offsets.copy()
    late[0, 0] = 1
    out_of_bank = [engine.make_objective('rotate', 3), engine.make_objective('shift_up', 0)]
    negative = [engine.make_objective('rotate', 0), engine.make_objective('shift_up', -1)]
    odd = [engine.make_objective('rotate', 0), engine.make_objective('shift_up', 0)]
    odd[1].use_rowcoef = 3
    bad = [dict(cfg=dict(theta_cells=0)), dict(cfg=dict(x_cells=1)), dict(cfg=dict(theta_cells=1 << 20, x_cells=1 << 11)), dict(cfg=dict(window=0)),
           dict(cfg=dict(closing_steps=-1)), dict(cfg=dict(x_half=0.0)), dict(cfg=dict(x_half=nan)), dict(cfg=dict(travel_max=inf)),
           dict(cfg=dict(finger_half_len=-0.1)), dict(no_cfg=True),
           # what dgdm_squeeze_map_3d refuses
           dict(mu_=1), dict(mu_=129), dict(mv_=0), dict(mv_=513), dict(mu_=128, mv_=9), dict(nb=0), dict(nb=(1 << 20) + 1), dict(nf=0), dict(surf=None),
           dict(gx_null=True), dict(off_null=True), dict(rot_=None), dict(gx=(-0.12, -0.07, -0.07, 0.03, 0.12)), dict(gx=(-0.12, -0.07, nan, 0.03, 0.12)),
           dict(gx=(0.12, 0.03, 0.0, -0.07, -0.12)), dict(n_seg=-1), dict(n_seg=5), dict(segs=None), dict(off=down), dict(off=late),
           # what dgdm_squeeze_objective_values refuses
           dict(objectives=field), dict(objectives=field, rc=rowcoef), dict(objectives=conv), dict(objectives=odd), dict(std=(0.05, 0.0, 0.004)),
           dict(std=(-0.05, 0.002, 0.004)), dict(std=(0.05, 0.002, nan)), dict(std=(inf, 0.002, 0.004)), dict(n_starts=0), dict(n_starts=-1),
           dict(starts=None), dict(values_=None), dict(obj_null=True), dict(std_null=True),
           # the groups
           dict(batch=0), dict(batch=-1), dict(n_groups=0), dict(n_groups=-1), dict(batch=65536), dict(first_null=True), dict(first=(4, 0)),
           dict(first=(0, -1)), dict(first=(3, 0), nf=4), dict(objectives=out_of_bank), dict(objectives=negative),
           dict(ws_b=size() - 1), dict(ws_b=0)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((tab == SENTINEL).all())      # nothing was launched
    assert call() == _lib.OK and call(objectives=conv, rc=rowcoef) == _lib.OK and call(ws_b=2 * size()) == _lib.OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool((tab != SENTINEL).all())
    cfg = C.byref(engine.squeeze_config(**good))
    assert lib.dgdm_squeeze_values_3d_workspace_bytes(C.byref(engine.squeeze_config(**dict(good, window=0))), 1, B, mu, mv, 3) == _lib.EINVAL
    for groups_, batch_, mu_, mv_, nb in ((0, 2, 5, 3, 3), (1, 0, 5, 3, 3), (1, 65536, 5, 3, 3), (32768, 2, 5, 3, 3), (1, 2, 1, 3, 3), (1, 2, 129, 3, 3),
                                          (1, 2, 5, 0, 3), (1, 2, 5, 513, 3), (1, 2, 128, 9, 3), (1, 2, 5, 3, 0)):
        assert lib.dgdm_squeeze_values_3d_workspace_bytes(cfg, groups_, batch_, mu_, mv_, nb) == _lib.EINVAL, (groups_, batch_, mu_, mv_, nb)
    assert lib.dgdm_squeeze_values_3d_workspace_bytes(cfg, 2, B, mu, mv, 3) > lib.dgdm_squeeze_values_3d_workspace_bytes(cfg, 1, B, mu, mv, 3) > 0
    with pytest.raises(ValueError, match="window"):
        engine.squeeze_values_3d(sf, GX, seg, offsets, [0], 2, plain[1:], st, window=0)
    with pytest.raises(ValueError, match="objectives"):
        engine.squeeze_values_3d(sf, GX, seg, offsets, [0, 2], 2, plain[1:], st)
    with pytest.raises(ValueError, match="rowcoef"):
        engine.squeeze_values_3d(sf, GX, seg, offsets, [0, 2], 2, conv, st, rowcoef[:1])
    with pytest.raises(ValueError, match="surfaces"):
        engine.squeeze_values_3d(sf[:, :, :2], GX, seg, offsets, [0], 2, plain[1:], st)


# ------------------------------------------------------------------------------------------------ 5. chain level
# tests/test_gpu_resample.py's 3-D rig: B = 4, G = 4, P = 2, L = 42, sub = 9, 4 objects, its chains and its FPS pre-draws
CFG5 = dict(theta_cells=24, x_cells=9, closing_steps=3, travel_max=0.15)
SAMPLE5 = 5
CHAINS5 = tgr.CHAINS['point_3d']


def meshes5():
    """Four prisms through every level of a 5 x 5 finger grid (z = 0 .. 0.12), wide enough for the decoded faces (L in -0.23 .. -0.13,
    U in 0.13 .. 0.23 at travel 0) to reach them within travel_max = 0.15."""
    return [prism(rect(0.09, 0.05), -0.01, 0.13), prism(rect(0.07, 0.04, (0.01, 0.0)), -0.01, 0.13), prism(ngon(3, 0.09, 0.2), -0.01, 0.13),
            prism(ngon(5, 0.08, 0.3), -0.01, 0.13)]


def potential():
    return SqueezePotential3D(meshes5(), sample_size=SAMPLE5, **CFG5)


def replay(dev, rs, seed, pre):
    """run_chains' walk with the sliced squeeze's potential, from engine calls that existed before dgdm_squeeze_values_3d: the per-pair
    map, then the values of its cells / y."""
    net, gd, s, noise, _ = tgr._rig(dev, 'point_3d')
    B, L = noise.shape[:2]
    nc, G, P = len(CHAINS5), gd.cfg.grid_size, gd.cfg.num_pos
    objectives = [engine.make_objective(o, oi) for oi, o in CHAINS5]
    scale = sampler.chain_scale('point_3d', CHAINS5[0][1])
    assert all(sampler.chain_scale('point_3d', o) == scale for _, o in CHAINS5)
    starts = torch.from_numpy(rso.start_grid(G, P, ORI)).to(dev)
    pairs = [(k * B + b, oi) for k, (oi, _) in enumerate(CHAINS5) for b in range(B)]
    x = noise.reshape(1, B, L).expand(nc, -1, -1).contiguous()
    logw, vprev = (torch.zeros((nc, B), dtype=torch.float64, device=dev) for _ in range(2))
    log, sl = [], None
    for si, t in enumerate(s.timesteps):
        t = int(t)
        n = 1 if si == 0 else nc
        eps = net.forward_cfg(x[:n].reshape(n * B, L, 1), torch.full((n * B,), t, dtype=torch.int32, device=dev), None, 1.0)
        eps = eps.reshape(n, B, L).expand(nc, -1, -1).contiguous()
        g = gd.grad(x, t, objectives, None, pre[1][si].reshape(-1))
        x = engine.ddim_guided_step(x, eps, g, 1, s.coefficients(t), scale, None, eta_coef=s.eta_coefficients(t, 0.5), seed=seed,
                                    chain_keys=list(range(nc)), step_index=si)
        if rs.evaluates(si, tgr.S):
            tn = int(s.timesteps[si + 1])
            eps_n = net.forward_cfg(x.reshape(nc * B, L, 1), torch.full((nc * B,), tn, dtype=torch.int32, device=dev), None, 1.0)
            clean = engine.ddim_pred_x0(x, eps_n.reshape(nc, B, L).contiguous(), s.coefficients(tn)[:2])
            gx, gz, sf = squeeze.finger_surfaces_3d(clean.reshape(nc * B, L), SAMPLE5)
            sl = sl or engine.squeeze_slice(meshes5(), gz)
            m = engine.squeeze_tables_3d(sf, gx, sl["segments"], sl["offsets"], pairs, starts, **CFG5)
            v = engine.squeeze_objective_values(m["cells"], m["y"], starts, B, objectives, None, STD, **CFG5)
            x, anc, ess, did = engine.chain_resample(x, v, 1, rs.beta / (G * P * P), rs.ess_frac, seed, list(range(nc)), si, logw, vprev)
            log.append((si, ess, did, anc, v))
    return x, log


def test_chains_equal_the_replay(dev):
    net, gd, s, noise, spec = tgr._rig(dev, 'point_3d')
    B, L = noise.shape[:2]
    nc, seed = len(CHAINS5), 5
    kw = dict(eta=0.5, noise_seed=seed)
    pre = tgr._predrawn(gd, 'point_3d', CHAINS5, 0)
    assert len(pre) == 2                                             # no evaluation draws: the guidance draws alone
    pot = potential()
    rs = Resample(1, 1.0, 2.0, 'squeeze_3d', pot)
    plain = sampler.guided_chains(net, gd, s, 'point_3d', noise, CHAINS5, predrawn=pre, **kw)
    log = []
    out = sampler.guided_chains(net, gd, s, 'point_3d', noise, CHAINS5, predrawn=pre, resample=rs, resample_log=log, **kw)
    ref, ref_log = replay(dev, rs, seed, pre)
    assert [e[0] for e in log] == [e[0] for e in ref_log] == [0, 1, 2, 3]
    for (_, ess, did, anc), (_, ress, rdid, ranc, v) in zip(log, ref_log):
        assert torch.equal(anc, ranc) and torch.equal(did, rdid) and torch.equal(ess, ress)
        assert int(did.sum()) == nc                                  # ess_frac = 2: every chain resamples at every evaluation
        print("values:", v.cpu().numpy().tolist())
        assert len(set(v.cpu().numpy().reshape(-1).tolist())) > 1   # a condition on the inputs: the per-pair route told the fingers apart
    print("ancestors:", [a.cpu().numpy().tolist() for _, _, _, a in log])
    assert np.array_equal(tgr._bits(out.reshape(nc, B, L)), tgr._bits(ref))
    assert not torch.equal(out, plain)
    # the same bits when run twice (the potential keeps its slices)
    assert torch.equal(sampler.guided_chains(net, gd, s, 'point_3d', noise, CHAINS5, predrawn=pre, resample=rs, **kw), out)
    # beta = 0 weighs all fingers alike: the run without `resample`, bit for bit
    log0 = []
    zero = sampler.guided_chains(net, gd, s, 'point_3d', noise, CHAINS5, predrawn=pre, resample=Resample(1, 0.0, potential='squeeze_3d', squeeze=pot),
                                 resample_log=log0, **kw)
    assert torch.equal(zero, plain) and len(log0) == 4 and all(int(d.sum()) == 0 for _, _, d, _ in log0)
    # the sharded sampler at world size 1, from the same start stream: its local bank is the chains' objects in first-use order
    sh = ddist.guided_chains_sharded(net, spec, s, 'point_3d', noise, gd._objs, CHAINS5, starts=tgr._stream(), resample=rs, **kw)
    assert torch.equal(sh, out)


def test_bf16_handle_and_refusals(dev):
    """The squeeze potential needs no forward-only trunk: a bf16 3-D handle resamples.  What check_resample refuses is refused before
    anything runs (the eps-net handed over is None)."""
    net, gd, s, noise, _ = tgr._rig(dev, 'point_3d')
    B = noise.shape[0]
    bf = engine.Guidance(gd.dyn, B, gd.cfg.grid_size, gd.cfg.num_pos, ORI, 20, tgr.T, 512, 9, max_objects=4, contraction_dtype="bf16")
    bf.set_objects(gd._objs.to(dev))
    pre = tgr._predrawn(gd, 'point_3d', CHAINS5, 0)
    pot = potential()
    log = []
    out = sampler.guided_chains(net, bf, s, 'point_3d', noise, CHAINS5, predrawn=pre, eta=0.5, noise_seed=5, resample_log=log,
                                resample=Resample(1, 1.0, 2.0, 'squeeze_3d', pot))
    assert out.shape == (len(CHAINS5), B, 42, 1) and bool(torch.isfinite(out).all()) and len(log) == 4
    assert all(int(d.sum()) == len(CHAINS5) for _, _, d, _ in log)
    with pytest.raises(ValueError, match="bf16"):
        sampler.guided_chains(None, bf, s, 'point_3d', noise, CHAINS5, predrawn=pre, eta=0.5, resample=Resample(1, 1.0, 2.0))
    with pytest.raises(ValueError, match="meshes"):                  # a bank of another size than the handle's objects
        sampler.guided_chains(None, gd, s, 'point_3d', noise, CHAINS5, predrawn=pre, eta=0.5,
                              resample=Resample(1, 1.0, potential='squeeze_3d', squeeze=SqueezePotential3D(meshes5()[:3])))
    _, gd2, s2, noise2, _ = tgr._rig(dev, 'point')
    with pytest.raises(ValueError, match="3-D fingers"):             # a 2-D handle
        sampler.guided_chains(None, gd2, s2, 'point', noise2, tgr.CHAINS['point'], eta=0.5, resample=Resample(1, 1.0, potential='squeeze_3d', squeeze=pot))


# ------------------------------------------------------------------------------------------------ 6. the entry point
def test_cli_resample_potential_squeeze_3d(dev, tmp_path, monkeypatch):
    """generator/train.py --mode=test on 3-D flags with mesh objects and --resample_potential squeeze_3d on a small table: the run's
    resample summary names the potential, every chain was evaluated twice, the unguided samples are those of the run without the flags."""
    from dgdm_amd.dynamics.parser import parse
    from dgdm_amd.generator import artefacts
    from dgdm_amd.generator.train import OBJECT_NAMES_3D, train
    monkeypatch.setattr(artefacts, "plot_fingers", lambda path, *a, **k: path)
    for k, name in enumerate(OBJECT_NAMES_3D):                      # mesh objects the decoded faces reach
        v, f = prism(rect(0.09 - 0.005 * k, 0.05 + 0.004 * k, (0.002 * k, 0.0)), 0.0, 0.1 + 0.004 * k)
        os.makedirs(tmp_path / "objects" / name)
        engine.write_obj(str(tmp_path / "objects" / name / "model.obj"), v, f)
    common = (f"--mode=test --classifier_guidance --fingers_3d --object_max_num_vertices=512 --ctrlpts_dim=42 --sub_bs=40 --num_fingers=2 --batch_size=2 "
              f"--grid_size=3 --num_pos=3 --num_train_timesteps=15 --num_inference_steps=5 --eta 0.5 --noise_seed 3 --object_dir={tmp_path / 'objects'}")
    flags = (" --resample_every 2 --resample_beta 2.0 --resample_ess 2.0 --resample_potential squeeze_3d --resample_squeeze_cells 24,9 "
             "--squeeze_closing_steps 3")
    torch.manual_seed(7)
    _, plain = train(parse(shlex.split(common)))
    torch.manual_seed(7)
    _, res = train(parse(shlex.split(common + flags)))
    rep = dict(res[0]["resample"])
    assert rep.pop("potential") == 'squeeze_3d' and "resample" not in plain[0]
    keys = [k for k in res[0] if k.startswith(("guided/", "multi/")) and "goal" not in k]
    assert keys and sorted(rep) == sorted(keys)
    for k in keys:
        for c in rep[k]:
            assert c["evaluations"] == 2 and c["resamples"] == 2, (k, c)      # --resample_ess 2: whenever evaluated
        assert bool(torch.isfinite(res[0][k]).all()) and float(res[0][k].abs().max()) <= 1.0, k
    assert any(not torch.equal(res[0][k], plain[0][k]) for k in keys)
    assert torch.equal(res[0]["unguided"], plain[0]["unguided"])
    with pytest.raises(ValueError, match="model.obj"):               # the run's objects are not mesh files
        train(parse(shlex.split(common.split(" --object_dir")[0] + flags)))
    with pytest.raises(ValueError, match="2-D only"):
        train(parse(shlex.split(common + flags.replace("squeeze_3d", "squeeze"))))
