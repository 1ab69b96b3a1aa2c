"""The squeeze simulator with Coulomb friction on the device (csrc/squeeze.hip, dgdm_squeeze_map_friction) against its float64 CPU
restatement tests/squeeze_friction_oracle.py, through the C ABI and through the layers above it.

Every operation of the contract (include/dgdm_hip.h "squeeze simulator with Coulomb friction") is a basic IEEE float64 one or an int32
one, so nothing here has a tolerance: the three tables and y are compared bit for bit; the successors, the three cells per start, the
flags, the jam table and the contact codes as integers, with no row excluded.  Shapes: 24 orientations x 7 x cells; 2, 9 and 17 surface
samples; 3 and 12 vertices; three fingers x two polygons, all six pairs; windows 1 and 2; closings of 0 and 3 steps; mu 0.1, 0.5 and 1;
40 starts, some beyond the x range and non-finite ones.  One case runs with a workspace of a single pair (the chunk loop) and one with
300 x cells (the lanes' stride over the x cells).  Every parameter set holds jammed and free cells, which is asserted."""
import ctypes as C
import functools
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import _lib, engine
from tests import resample_squeeze_oracle as rso
from tests import squeeze_friction_oracle as fo
from tests import squeeze_oracle as so
from tests import test_squeeze_friction_host as host

pytestmark = pytest.mark.gpu

HL, XH, TM = 0.12, 0.06, 0.1
PAIRS = [(f, o) for o in range(2) for f in range(3)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.device_init(0)
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def fingers(m, seed=11):
    """Three random jaw pairs about L = -0.05 and U = 0.05: a tilt, a bow and a sample-wise jitter each."""
    rs = np.random.RandomState(seed + m)
    u = np.linspace(-1.0, 1.0, m)
    out = []
    for _ in range(3):
        rows = [off + rs.uniform(-0.01, 0.01) * u + rs.uniform(-0.01, 0.01) * np.cos(2.0 * u + rs.uniform(0, 6)) + rs.uniform(-0.002, 0.002, m)
                for off in (-0.05, 0.05)]
        out.append(np.stack(rows))
    return np.stack(out)


def polygons(nv, seed=23):
    """Two random star-shaped polygons: a slender one about its origin (orientations at which two contacts cannot hold it even at mu = 1)
    and a clockwise one 9 cm off its origin, which passes the finger ends at some cells (no contact there, S = +inf)."""
    rs = np.random.RandomState(seed + nv)
    out = []
    for k, (stretch, centre) in enumerate((((0.045, 0.012), (0.0, 0.0)), ((0.03, 0.03), (0.09, 0.0)))):
        ang = np.sort(rs.uniform(0, 2 * np.pi / nv, nv) + 2 * np.pi * np.arange(nv) / nv)
        p = np.stack([np.cos(ang), np.sin(ang)], axis=1) * rs.uniform(0.7, 1.0, (nv, 1)) * np.array(stretch) + np.array(centre)
        out.append(p[::-1].copy() if k else p)
    return np.stack(out)


def starts(T, x_half, n=40, seed=5):
    rs = np.random.RandomState(seed)
    st = np.stack([rs.uniform(-7.0, 14.0, n), rs.uniform(-1.3 * x_half, 1.3 * x_half, n), rs.uniform(-0.05, 0.05, n)], axis=1)
    dth = so.TWO_PI / T
    st[0] = (0.5 * dth, 0.0, 0.0)                      # halves round up
    st[1] = (-0.5 * dth, -2.0 * x_half, 0.2)           # beyond the x range
    st[2] = (so.TWO_PI - 0.25 * dth, 3.0 * x_half, -0.2)
    st[3] = (np.nan, np.nan, 0.0)                      # non-finite starts land on cell 0, no index leaves the table
    st[4] = (np.inf, -np.inf, 0.01)
    st[5] = (1e300, 1e300, np.nan)
    return st


@functools.lru_cache(maxsize=None)
def contact_reference(m, nv, T=24, X=7):
    """The oracle's tables per pair: they do not depend on mu, the window or the number of steps."""
    sf, ob, rot = fingers(m), polygons(nv), so.rotation_table(T)
    return [fo.contact_tables(sf[f][0], sf[f][1], ob[o], rot, X, XH, HL) for f, o in PAIRS]


def reference(m, nv, window, k, mu, T=24, X=7):
    sf, ob, rot, st = fingers(m), polygons(nv), so.rotation_table(T), starts(T, XH)
    outs = [fo.squeeze_pair(sf[f][0], sf[f][1], ob[o], rot, st, X, XH, window, k, TM, HL, mu, tables=tab)
            for (f, o), tab in zip(PAIRS, contact_reference(m, nv, T, X))]
    return {key: np.stack([o[key] for o in outs]) for key in outs[0]}


def run(m, nv, window, k, mu, T=24, X=7, chunk_pairs=6, entry="friction", slack=0):
    """slack: bytes on top of the size the library gives for chunk_pairs, which must still hold no further pair."""
    cfg = dict(theta_cells=T, x_cells=X, x_half=XH, window=window, closing_steps=k, travel_max=TM, finger_half_len=HL)
    size = _lib.lib().dgdm_squeeze_friction_workspace_bytes if entry == "friction" else _lib.lib().dgdm_squeeze_workspace_bytes
    ws = int(size(C.byref(engine.squeeze_config(**cfg)), chunk_pairs)) + slack
    assert slack == 0 or ws < int(size(C.byref(engine.squeeze_config(**cfg)), chunk_pairs + 1))
    kw = dict(friction=mu, jam=True, contact=True) if entry == "friction" else {}
    out = engine.squeeze_tables(fingers(m), polygons(nv), PAIRS, starts(T, XH), rot=so.rotation_table(T), tables=True, workspace_bytes=ws, **cfg, **kw)
    return {key: v.cpu().numpy() for key, v in out.items()}


def compare(got, ref):
    for key in ("touch_l", "touch_r", "S"):
        bad = np.argwhere(bits(got[key]) != bits(ref[key]))
        assert len(bad) == 0, f"{key}: {len(bad)} cells differ, first (pair, a, b) = {bad[0]}: {got[key][tuple(bad[0])]!r} vs {ref[key][tuple(bad[0])]!r}"
    bad = np.argwhere(got["contact"] != ref["contact"])
    assert len(bad) == 0, f"contact: {len(bad)} differ, first (pair, a, b, side) = {bad[0]}: {got['contact'][tuple(bad[0])]} vs {ref['contact'][tuple(bad[0])]}"
    bad = np.argwhere(got["jam"] != ref["jam"])
    assert len(bad) == 0, f"jam: {len(bad)} cells differ, first (pair, a, b) = {bad[0]}, contacts {ref['contact'][tuple(bad[0])]}"
    assert np.array_equal(got["succ"], ref["succ"])
    assert np.array_equal(got["cells"], ref["cells"])
    assert np.array_equal(bits(got["y"]), bits(ref["y"]))
    assert np.array_equal(got["flags"], ref["flags"])


@pytest.mark.parametrize("mu", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("nv", [3, 12])
@pytest.mark.parametrize("m", [2, 9, 17])
def test_tables_and_maps_equal_the_oracle(dev, m, nv, mu):
    for window in (1, 2):
        for k in (0, 3):
            ref = reference(m, nv, window, k, mu)
            assert (ref["jam"] == 1).any() and (ref["jam"] == 0).any() and (ref["contact"] >= nv).any() and ((ref["contact"] >= 0) & (ref["contact"] < nv)).any()
            compare(run(m, nv, window, k, mu), ref)
    assert (ref["flags"] & 8).any() and (ref["flags"] & 16).any() and (ref["cells"][..., 2] != ref["cells"][..., 0]).any()


def test_a_workspace_of_one_pair_runs_the_chunk_loop(dev):
    ref = reference(9, 12, 2, 3, 0.5)
    one, six = run(9, 12, 2, 3, 0.5, chunk_pairs=1), run(9, 12, 2, 3, 0.5)
    compare(one, ref)
    for key in one:
        assert np.array_equal(one[key].view(np.uint8), six[key].view(np.uint8)), key
    # 6 pairs in chunks of 4 and 2: a shorter last chunk behind the jam table; then 1000 bytes more, still 4 pairs and no size the
    # library returns
    assert {"jam", "contact"} <= set(six)
    for got in (run(9, 12, 2, 3, 0.5, chunk_pairs=4), run(9, 12, 2, 3, 0.5, chunk_pairs=4, slack=1000)):
        assert set(got) == set(six)
        for key in six:
            assert np.array_equal(six[key].view(np.uint8), got[key].view(np.uint8)), key


def test_more_x_cells_than_lanes(dev):
    """300 x cells on 256 lanes, 2 orientations: the second pass of the lanes over the x cells."""
    ref = reference(17, 12, 2, 3, 0.5, T=2, X=300)
    assert (ref["jam"][:, :, 256:] == 1).any() and (ref["jam"][:, :, 256:] == 0).any() and (ref["jam"][:, :, :256] == 1).any()
    compare(run(17, 12, 2, 3, 0.5, T=2, X=300), ref)


def test_mu_zero_is_the_frictionless_entry_bit_for_bit(dev):
    new, old = run(9, 12, 2, 3, 0.0), run(9, 12, 2, 3, 0.0, entry="plain")
    assert set(new) - set(old) == {"jam", "contact"}
    for key in old:
        assert np.array_equal(new[key].view(np.uint8), old[key].view(np.uint8)), key
    assert not new["jam"].any()
    assert np.array_equal(new["contact"], reference(9, 12, 2, 3, 0.0)["contact"]) and (new["contact"] >= 0).any()
    assert not (new["flags"] & 24).any()


@pytest.mark.parametrize("mu", [0.25, 1.0])
def test_rectangle_between_flat_jaws_jams_in_bands_about_the_unstable_poses(dev, mu):
    """tests/test_squeeze_friction_host.py's closed form, on the device."""
    lower, upper, rot, T, X, xh = host.rectangle_case()
    st = host.grid_starts(T, X, xh)
    cfg = dict(theta_cells=T, x_cells=X, x_half=xh, window=1, closing_steps=6, travel_max=0.1, finger_half_len=HL)
    sf = np.stack([lower, upper])[None]
    r = {k: v.cpu().numpy()[0] for k, v in engine.squeeze_tables(sf, host.RECT[None], [(0, 0)], st, rot=rot, tables=True, friction=mu, **cfg).items()}
    free = {k: v.cpu().numpy()[0] for k, v in engine.squeeze_tables(sf, host.RECT[None], [(0, 0)], st, rot=rot, **cfg).items()}
    inside, outside = host.band_masks(T, mu)
    assert (r["jam"][inside] == 1).all() and (r["jam"][outside] == 0).all()
    c0, ck, cf = r["cells"].T
    jammed = r["jam"].reshape(-1)[c0] != 0
    assert np.array_equal(c0, np.arange(T * X)) and jammed[np.repeat(inside, X)].all() and not jammed[np.repeat(outside, X)].any()
    assert np.array_equal(cf[jammed], c0[jammed]) and np.array_equal(ck[jammed], c0[jammed]) and (r["flags"][jammed] & 24 == 24).all()
    assert np.array_equal(cf[~jammed], free["cells"][~jammed, 2]) and np.array_equal(ck[~jammed], free["cells"][~jammed, 1])
    assert (r["flags"][~jammed] & 8 == 0).all() and np.array_equal(cf % X, c0 % X) and np.array_equal(ck % X, c0 % X)


@pytest.mark.parametrize("mu, jams", [(0.10, False), (0.15, False), (0.20, True), (0.25, True)])
def test_disc_in_a_wedge_jams_when_mu_exceeds_tan_of_half_the_angle(dev, mu, jams):
    lower, upper, disc, rot, T, X, xh = host.disc_case()
    st = host.grid_starts(T, X, xh)
    cfg = dict(theta_cells=T, x_cells=X, x_half=xh, window=2, closing_steps=1 << 20, travel_max=0.1, finger_half_len=HL)
    sf = np.stack([lower, upper])[None]
    r = {k: v.cpu().numpy()[0] for k, v in engine.squeeze_tables(sf, disc[None], [(0, 0)], st, rot=rot, tables=True, friction=mu, **cfg).items()}
    if jams:
        assert (r["jam"] == 1).all() and np.array_equal(r["cells"][:, 2], r["cells"][:, 0]) and (r["flags"] & 24 == 24).all()
    else:
        free = engine.squeeze_tables(sf, disc[None], [(0, 0)], st, rot=rot, **cfg)["cells"].cpu().numpy()[0]
        assert (r["jam"] == 0).all() and np.array_equal(r["cells"], free) and (r["flags"] & 24 == 0).all()
        assert (r["cells"][:, 2] % X == 0).all() and (r["flags"] & 4 == 4).all()


def test_every_bad_argument_is_refused_before_a_launch(dev):
    lib = _lib.lib()
    sf = torch.zeros(2, 2, 8, dtype=torch.float64, device=dev)
    ob = torch.zeros(3, 4, 2, dtype=torch.float64, device=dev)
    rot = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    st = torch.zeros(2, 3, dtype=torch.float64, device=dev)
    cells = torch.full((1, 2, 3), -7, dtype=torch.int32, device=dev)
    jam = torch.full((1, 8, 5), -7, dtype=torch.int32, device=dev)
    y = torch.zeros(1, 2, 2, dtype=torch.float64, device=dev)
    flags = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    good = dict(theta_cells=8, x_cells=5, window=1, closing_steps=2, x_half=0.06, travel_max=0.1, finger_half_len=0.12)
    ws_bytes = int(lib.dgdm_squeeze_friction_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1))
    assert ws_bytes > int(lib.dgdm_squeeze_workspace_bytes(C.byref(engine.squeeze_config(**good)), 1))     # the jam table lives there
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call(cfg=None, m=8, nv=4, pair=(1, 2), n_pairs=1, nf=2, no=3, surf=sf, ws_b=ws_bytes, cells_out=cells, mu=0.5):
        c = engine.squeeze_config(**dict(good, **(cfg or {})))
        pr = np.array([pair], dtype=np.int32)
        return lib.dgdm_squeeze_map_friction(C.byref(c), _lib.dptr(surf), nf, m, _lib.dptr(ob), no, nv, pr.ctypes.data, n_pairs, _lib.dptr(rot),
                                             _lib.dptr(st), 2, _lib.dptr(cells_out), _lib.dptr(y), _lib.dptr(flags), None, None, None, None,
                                             _lib.dptr(ws), ws_b, None, mu, _lib.dptr(jam), None)

    bad = [dict(mu=-0.1), dict(mu=float("nan")), dict(mu=float("inf")), dict(mu=-float("inf")),
           dict(cfg=dict(theta_cells=0)), dict(cfg=dict(x_cells=1)), dict(cfg=dict(theta_cells=1 << 20, x_cells=1 << 11)), dict(cfg=dict(window=0)),
           dict(cfg=dict(closing_steps=-1)), dict(cfg=dict(x_half=0.0)), dict(cfg=dict(x_half=float("nan"))), dict(cfg=dict(x_half=float("inf"))),
           dict(cfg=dict(travel_max=float("inf"))), dict(cfg=dict(finger_half_len=-0.1)), dict(m=1), dict(m=4096), dict(nv=2), dict(nv=4096),
           dict(pair=(2, 0)), dict(pair=(0, 3)), dict(pair=(-1, 0)), dict(n_pairs=0), dict(nf=0), dict(no=0), dict(surf=None),
           dict(ws_b=ws_bytes - 1), dict(cells_out=None)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert lib.dgdm_last_error()
    torch.cuda.synchronize()
    assert (cells.cpu() == -7).all() and (jam.cpu() == -7).all()                 # nothing was launched
    assert call() == _lib.OK and (cells.cpu() >= 0).all() and ((jam.cpu() == 0) | (jam.cpu() == 1)).all()
    assert call(mu=0.0) == _lib.OK and (jam.cpu() == 0).all()
    assert lib.dgdm_squeeze_friction_workspace_bytes(C.byref(engine.squeeze_config(**dict(good, window=0))), 1) == _lib.EINVAL
    assert lib.dgdm_squeeze_friction_workspace_bytes(C.byref(engine.squeeze_config(**good)), 0) == _lib.EINVAL
    with pytest.raises(ValueError, match="finite non-negative"):
        engine.squeeze_tables(sf, ob, [(0, 0)], st, friction=-1.0)


def test_squeeze_simulator_with_friction(dev):
    """SqueezeSimulator(friction=0.25): the metric keys and marks, and the maps behind them are the friction oracle's."""
    from dgdm_amd import synth
    from dgdm_amd.sim.squeeze import OBJECT_HALF_BOX_2D, SqueezeSimulator, finger_surfaces

    class Holder:
        mode = 'point'
        object_vertices = torch.stack([synth.synth_object_2d(i, 100) for i in range(2)])

        def _object_ids(self):
            return [11, 12]

    cfg = dict(closing_steps=3, theta_cells=90, x_cells=33)
    samples = np.random.RandomState(0).uniform(-1, 1, (3, 14, 1)).astype(np.float32)
    plain = SqueezeSimulator(Holder(), **cfg)(samples, [12, 11], None, num_rot=45, ori_range=(-0.5, 1.0))[1]
    out = SqueezeSimulator(Holder(), friction=0.25, **cfg)(samples, [12, 11], None, num_rot=45, ori_range=(-0.5, 1.0))
    assert len(out) == 8 and len(out[1]) == 6
    theta0 = (np.linspace(-0.5, 1.0, 45) + 1.0) * np.pi
    st = np.stack([theta0, np.zeros(45), np.zeros(45)], axis=1)
    sf = finger_surfaces(torch.from_numpy(samples).reshape(3, -1)).cpu().numpy()
    bank = Holder.object_vertices.double().numpy()[[1, 0]] * OBJECT_HALF_BOX_2D
    jammed = 0
    for p, (met, base) in enumerate(zip(out[1], plain)):
        assert set(met) - set(base) == {'squeeze_friction', 'squeeze_jammed'} and set(base) <= set(met)
        assert 'predicted' not in met and met['simulated'] == 'squeeze' and met['squeeze_friction'] == 0.25
        assert 'squeeze_friction' not in base and 'squeeze_jammed' not in base
        o, f = divmod(p, 3)                              # object-major, gripper-minor
        ref = fo.squeeze_pair(sf[f][0], sf[f][1], bank[o], so.rotation_table(90), st, 33, 0.06, 2, 3, 0.1, 0.12, mu=0.25)
        assert met['squeeze_jammed'] == int(np.count_nonzero(ref["flags"] & 16))
        # the settled orientation as a cell: degrees are multiples of 360 / 90 = 4 up to the last bit of the conversion
        assert np.array_equal(np.rint(met['final_theta'] / 4.0).astype(np.int64) % 90, ref["cells"][:, 2] // 33)
        assert np.array_equal(np.rint((met['final_theta'] - met['final_delta_theta']) / 4.0).astype(np.int64) % 90, ref["cells"][:, 0] // 33)
        jammed += met['squeeze_jammed']
    assert jammed > 0


def test_cli_squeeze_friction_leaves_the_samples_alone(dev, tmp_path):
    """--squeeze_sim --squeeze_friction through the command-line entry point: the sampled designs are bit-identical with the flags on and
    off, every score is marked 'simulated': 'squeeze' and carries no 'predicted'."""
    import json
    import os
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    common = ("--mode=test --classifier_guidance --object_max_num_vertices=100 --ctrlpts_dim=14 --num_fingers=2 --batch_size=2 --grid_size=3 "
              "--num_pos=3 --num_train_timesteps=15 --num_inference_steps=2")
    runs = {}
    for tag, extra in (("off", ""), ("on", " --squeeze_sim --squeeze_closing_steps 4 --squeeze_window 1 --squeeze_friction 0.25")):
        torch.manual_seed(7)
        _, runs[tag] = train(parse(shlex.split(common + extra + f" --save_dir={tmp_path / tag}")))
    assert runs["on"][0].keys() == runs["off"][0].keys()
    for k, v in runs["off"][0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, runs["on"][0][k]), k
    tables = sorted(os.listdir(tmp_path / "on" / "tables"))
    assert "SKIPPED.txt" not in tables and tables
    for t in tables:
        tab = json.load(open(tmp_path / "on" / "tables" / t))
        oc = tab["columns"].index("objective")
        scores = [row[oc] for row in tab["data"] if isinstance(row[oc], dict) and row[0] != -1]
        assert scores and all(s.get("simulated") == "squeeze" and "predicted" not in s for s in scores), t


@pytest.mark.parametrize("nc,B", [(1, 3), (3, 1)])
def test_resample_values_with_friction_equal_the_oracles(dev, nc, B):
    """SqueezePotential(friction=0.5).values == resample_squeeze_oracle's values of the friction oracle's map of the same surfaces; the
    Resample that carries it says so, and friction changed the map."""
    from dgdm_amd import synth
    from dgdm_amd.dynamics.dataloader import SCORE_STD
    from dgdm_amd.resample import Resample, SqueezePotential
    from dgdm_amd.sim import squeeze
    std = tuple(float(v) for v in SCORE_STD[1])
    G, P, ori, L, n_grad, mu = 8, 3, (-0.5, 0.25), 14, 2, 0.5
    cfg = dict(theta_cells=24, x_cells=9, window=2, closing_steps=3)
    bank = np.stack([synth.synth_object_2d(i, 100).double().numpy().reshape(100, 2) * squeeze.OBJECT_HALF_BOX_2D for i in range(2)])
    x0 = torch.from_numpy(np.random.RandomState(4).uniform(-1, 1, (3, L)).astype(np.float32)).to(dev).reshape(nc, B, L)
    names = ['rotate', 'clockwise_up', 'convergence', 'shift_left', 'rotate_clockwise', 'convergence']
    objectives = [engine.make_objective(names[(j * nc + k) % len(names)], (j + k) % 2) for j in range(n_grad) for k in range(nc)]
    N = G * P * P
    rowcoef = np.random.RandomState(6).choice([-1.0, 0.0, 1.0], size=(n_grad * nc, N * B)).astype(np.float32)
    pot = SqueezePotential(bank, friction=mu, **cfg)
    rs = Resample(1, 1.0, 2.0, potential='squeeze', squeeze=pot)
    assert rs.squeeze.friction == mu and "friction=0.5" in repr(pot)
    got = rs.squeeze.values(x0, objectives, torch.from_numpy(rowcoef).to(dev), n_grad, G, P, ori)
    starts_ = rso.start_grid(G, P, ori)
    sf = squeeze.finger_surfaces(x0.reshape(nc * B, L)).cpu().numpy()
    pairs = [(k * B + b, int(objectives[j * nc + k].object)) for j in range(n_grad) for k in range(nc) for b in range(B)]
    kw = dict(x_cells=9, x_half=0.06, window=2, closing_steps=3, travel_max=0.1, half_len=0.12)
    ref_map = fo.squeeze_map(sf, bank, pairs, so.rotation_table(24), starts_, mu=mu, **kw)
    free_map = so.squeeze_map(sf, bank, pairs, so.rotation_table(24), starts_, **kw)
    assert (ref_map["flags"] & 8).any() and not np.array_equal(ref_map["cells"], free_map["cells"])
    ref = rso.objective_values(ref_map["cells"], ref_map["y"], starts_, B, objectives, rowcoef, std, 24, 9, 0.06)
    assert got.shape == (n_grad * nc, B) and np.array_equal(bits(got.cpu().numpy()).reshape(-1), bits(ref)), (got.cpu().numpy().reshape(-1), ref)
    plain = SqueezePotential(bank, **cfg).values(x0, objectives, torch.from_numpy(rowcoef).to(dev), n_grad, G, P, ori)
    assert not torch.equal(plain, got)
