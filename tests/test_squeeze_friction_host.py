"""Host side of the squeeze simulator's friction rule: tests/squeeze_friction_oracle.py against the frictionless oracle and against two
closed forms of two-contact jamming (a rectangle between flat jaws: bands of atan(mu) about the four unstable poses; a disc in a 20 degree
wedge: jammed exactly when mu >= tan 10 degrees), and the refusals of the layers above.  No tolerance anywhere: bit or integer equality,
and closed forms asserted away from their thresholds.  No GPU."""
import json

import numpy as np
import pytest

from tests import squeeze_friction_oracle as fo
from tests import squeeze_oracle as so

HL = 0.12
RECT = np.array([[-0.03, -0.015], [0.03, -0.015], [0.03, 0.015], [-0.03, 0.015]])       # 0.06 x 0.03 m


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def grid_starts(T, X, x_half):
    return np.array([[2.0 * np.pi * a / T, -x_half + b * (2.0 * x_half / (X - 1)), 0.0] for a in range(T) for b in range(X)])


@pytest.mark.parametrize("m, nv, seed", [(2, 3, 0), (9, 12, 1), (17, 5, 2), (50, 40, 3)])
def test_oracle_keeps_the_frictionless_tables_and_mu_zero_jams_nothing(m, nv, seed):
    rs = np.random.RandomState(seed)
    T, X, xh = 24, 7, 0.08
    u = np.linspace(-1.0, 1.0, m)
    lower = -0.06 + 0.02 * np.cos(3.0 * u + rs.uniform(0, 6)) + rs.uniform(-0.004, 0.004, m)
    upper = 0.07 + 0.02 * np.cos(2.0 * u + rs.uniform(0, 6)) + rs.uniform(-0.004, 0.004, m)
    ang = np.sort(rs.uniform(0, 2 * np.pi, nv))
    verts = np.stack([np.cos(ang), np.sin(ang)], axis=1) * rs.uniform(0.01, 0.09, (nv, 1))       # reaches past the finger ends at some cells
    rot = so.rotation_table(T)
    tab = fo.contact_tables(lower, upper, verts, rot, X, xh, HL)
    tl, tr, S = so.touch_tables(lower, upper, verts, rot, X, xh, HL)
    for got, ref in ((tab["touch_l"], tl), (tab["touch_r"], tr), (tab["S"], S)):
        assert np.array_equal(bits(got), bits(ref))
    none = tab["contact"] < 0
    assert np.array_equal(none[..., 0], np.isinf(tl)) and np.array_equal(none[..., 1], np.isinf(tr))
    assert tab["contact"].max() < nv + nv * m
    st = np.concatenate([grid_starts(T, X, xh), [[np.nan, np.inf, 0.01], [40.0, -1.0, -0.02]]])
    kw = dict(x_cells=X, x_half=xh, window=2, closing_steps=3, travel_max=0.1, half_len=HL)
    ref = so.squeeze_pair(lower, upper, verts, rot, st, **kw)
    got = fo.squeeze_pair(lower, upper, verts, rot, st, mu=0.0, **kw)
    assert not got["jam"].any()
    for k, v in ref.items():
        assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), k
    # and friction only ever stops cells: every successor is the frictionless one or the cell itself
    fr = fo.squeeze_pair(lower, upper, verts, rot, st, mu=0.5, **kw)
    own = np.arange(T * X)
    assert np.array_equal(fr["succ"], np.where(fr["jam"].reshape(-1) != 0, own, ref["succ"]))
    assert np.array_equal((fr["flags"] & 8) != 0, fr["jam"].reshape(-1)[fr["cells"][:, 0]] != 0)
    assert np.array_equal((fr["flags"] & 16) != 0, fr["jam"].reshape(-1)[fr["cells"][:, 2]] != 0)


def rectangle_case():
    """The issue's set-up: 0.06 x 0.03 m rectangle, 41 samples, flat jaws at -0.05 and 0.05, 360 x 5 cells, x_half 0.01."""
    m, T, X, xh = 41, 360, 5, 0.01
    return np.full(m, -0.05), np.full(m, 0.05), so.rotation_table(T), T, X, xh


def band_masks(T, mu):
    """(inside, outside) over the theta cells: more than one cell inside a band theta* +- atan(mu) about the unstable poses atan 2 and its
    mirrors, more than one cell outside every band; 0 / 90 / 180 / 270 are in neither (their contacts tie)."""
    deg = np.arange(T) * (360.0 / T)
    star = np.degrees(np.arctan(2.0))
    half = np.degrees(np.arctan(mu))
    dist = np.min([np.abs(deg - c) for c in (star, 180.0 - star, 180.0 + star, 360.0 - star)], axis=0)
    axis = np.isin(deg, (0.0, 90.0, 180.0, 270.0))
    one = 360.0 / T
    return (dist < half - one) & ~axis, (dist > half + one) & ~axis


@pytest.fixture(scope="module")
def rect_tables():
    lower, upper, rot, T, X, xh = rectangle_case()
    return fo.contact_tables(lower, upper, RECT, rot, X, xh, HL)


@pytest.mark.parametrize("mu", [0.25, 1.0])
def test_rectangle_between_flat_jaws_jams_in_bands_about_the_unstable_poses(rect_tables, mu):
    lower, upper, rot, T, X, xh = rectangle_case()
    st = grid_starts(T, X, xh)
    kw = dict(x_cells=X, x_half=xh, window=1, closing_steps=6, travel_max=0.1, half_len=HL)
    r = fo.squeeze_pair(lower, upper, RECT, rot, st, mu=mu, tables=rect_tables, **kw)
    free = so.squeeze_pair(lower, upper, RECT, rot, st, **kw)
    inside, outside = band_masks(T, mu)
    assert inside.sum() >= 4 * 20 and outside.sum() >= 20
    assert (r["jam"][inside] == 1).all() and (r["jam"][outside] == 0).all()
    c0, ck, cf = r["cells"].T
    assert np.array_equal(c0, np.arange(T * X)) and not (r["flags"] & 3).any()
    jammed = r["jam"].reshape(-1)[c0] != 0
    assert np.array_equal(cf[jammed], c0[jammed]) and np.array_equal(ck[jammed], c0[jammed]) and (r["flags"][jammed] & 24 == 24).all()
    assert np.array_equal(cf[~jammed], free["cells"][~jammed, 2]) and np.array_equal(ck[~jammed], free["cells"][~jammed, 1])
    assert (r["flags"][~jammed] & 8 == 0).all()                    # 16 may be up: flat on the jaws (0 / 90 / ..) is itself a grip that holds
    assert np.array_equal(r["flags"] & 16 != 0, r["jam"].reshape(-1)[cf] != 0)
    assert np.array_equal(cf % X, c0 % X) and np.array_equal(ck % X, c0 % X)
    start_inside = np.repeat(inside, X)
    assert jammed[start_inside].all() and not jammed[np.repeat(outside, X)].any()


def disc_case():
    """A 360-gon of radius 0.02 m over a lower jaw rising at 20 degrees, the upper jaw flat at 0.05; 4 x 9 cells, x_half 0.04."""
    m, T, X, xh = 41, 4, 9, 0.04
    u = -HL + np.arange(m) * (2.0 * HL / (m - 1))
    ang = 2.0 * np.pi * (np.arange(360) + 0.5) / 360
    disc = 0.02 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return np.tan(np.radians(20.0)) * u - 0.05, np.full(m, 0.05), disc, so.rotation_table(T), T, X, xh


@pytest.fixture(scope="module")
def disc_tables():
    lower, upper, disc, rot, T, X, xh = disc_case()
    return fo.contact_tables(lower, upper, disc, rot, X, xh, HL)


@pytest.mark.parametrize("mu, jams", [(0.10, False), (0.15, False), (0.20, True), (0.25, True)])
def test_disc_in_a_wedge_jams_when_mu_exceeds_tan_of_half_the_angle(disc_tables, mu, jams):
    """The chord between the two contacts makes 10 degrees with both normals: tan 10 = 0.176 lies between 0.15 and 0.20 with room for the
    half degree of the 360-gon.  Free, the disc moves toward the wedge's opening (-x) as without friction, to the table's edge."""
    lower, upper, disc, rot, T, X, xh = disc_case()
    st = grid_starts(T, X, xh)
    kw = dict(x_cells=X, x_half=xh, window=2, closing_steps=1 << 20, travel_max=0.1, half_len=HL)
    r = fo.squeeze_pair(lower, upper, disc, rot, st, mu=mu, tables=disc_tables, **kw)
    assert (r["S"] < 0.1).all()
    if jams:
        assert (r["jam"] == 1).all() and np.array_equal(r["cells"][:, 2], r["cells"][:, 0]) and (r["flags"] & 24 == 24).all()
    else:
        free = so.squeeze_pair(lower, upper, disc, rot, st, **kw)
        assert (r["jam"] == 0).all() and np.array_equal(r["cells"], free["cells"]) and (r["flags"] & 24 == 0).all()
        assert (r["cells"][:, 2] % X == 0).all() and (r["flags"] & 4 == 4).all()


def test_flag_and_argument_refusals(tmp_path):
    from dgdm_amd import engine
    from dgdm_amd.generator.train import squeeze_3d_from_args, squeeze_from_args, train
    from dgdm_amd.resample import SqueezePotential, squeeze_potential_from_args
    from dgdm_amd.sim import sim_2d, sim_3d
    from dgdm_amd.sim.squeeze import SqueezeSimulator, SqueezeSimulator3D, squeeze_map_3d, squeeze_metric
    from dynamics.parser import parse
    base = "--mode=test --classifier_guidance --ctrlpts_dim=14 --object_max_num_vertices=100 --num_fingers=2 --batch_size=2"
    assert parse(base.split()).squeeze_friction is None
    assert squeeze_from_args(parse((base + " --squeeze_sim").split())) == {}
    assert squeeze_from_args(parse((base + " --squeeze_sim --squeeze_friction 0.5 --squeeze_window 3").split())) == {"window": 3, "friction": 0.5}
    res = base + " --eta 1.0 --resample_every 2 --resample_beta 1.0 --resample_potential squeeze"
    assert squeeze_potential_from_args(parse((res + " --squeeze_friction 0.25 --squeeze_closing_steps 4").split())) == \
        {"friction": 0.25, "closing_steps": 4}
    assert squeeze_from_args(parse((res + " --squeeze_friction 0.25").split())) is None      # a squeeze user: not refused
    for extra, why in ((" --squeeze_friction 0.5", "needs --squeeze_sim or --resample_potential squeeze"),
                       (" --squeeze_sim --squeeze_friction -0.1", "finite non-negative"), (" --squeeze_sim --squeeze_friction nan", "finite non-negative"),
                       (" --squeeze_sim --squeeze_friction inf", "finite non-negative"),
                       (" --fingers_3d --squeeze_sim_3d --squeeze_friction 0.5", "friction is 2-D only")):
        with pytest.raises(ValueError, match=why):
            train(parse((base + extra).split()))                  # refused before anything is built: no device is touched
    with pytest.raises(ValueError, match="friction is 2-D only"):
        squeeze_3d_from_args(parse((base + " --fingers_3d --squeeze_sim_3d --squeeze_friction 0.5").split()))
    with pytest.raises(ValueError, match="finite non-negative"):
        squeeze_potential_from_args(parse((res + " --squeeze_friction -1").split()))

    class Holder:
        mode = 'point'
    assert SqueezeSimulator(Holder(), friction=0.25).friction == 0.25 and SqueezeSimulator(Holder()).friction == 0.0
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite non-negative"):
            SqueezeSimulator(Holder(), friction=bad)
        with pytest.raises(ValueError, match="finite non-negative"):
            SqueezePotential(np.zeros((1, 4, 2)), friction=bad)
        with pytest.raises(ValueError, match="finite non-negative"):
            engine.squeeze_tables(None, None, [(0, 0)], friction=bad)                # before the library or a device is touched
        with pytest.raises(ValueError, match="finite non-negative"):
            sim_2d.generate(str(tmp_path / "no"), [0], np.zeros((1, 4, 2)), [0], friction=bad)
    assert SqueezePotential(np.zeros((1, 4, 2)), friction=0.5).friction == 0.5
    Holder.mode = 'point_3d'
    with pytest.raises(ValueError, match="friction is 2-D only"):
        SqueezeSimulator3D(Holder(), object_mesh_dir=str(tmp_path), friction=0.5)
    with pytest.raises(ValueError, match="friction is 2-D only"):
        squeeze_map_3d(None, [], None, friction=0.0)
    with pytest.raises(ValueError, match="friction is 2-D only"):
        sim_3d.generate(str(tmp_path / "no"), [0], [], [], [], friction=0.5)
    with pytest.raises(ValueError, match="friction is 2-D only"):
        sim_3d.main(["root", "0", "0", "1", "1", str(tmp_path / "no"), "1", "--friction", "0.5"])
    with pytest.raises(ValueError, match="finite non-negative"):
        sim_2d.main(["root", "0", "0", "1", "1", str(tmp_path / "no"), "1", "--object_dir", "none.npy", "--friction", "-1"])

    # the metric gains its two keys with friction on, and only then
    n = 12
    st = np.stack([np.linspace(0, 2 * np.pi, n, endpoint=False), np.zeros(n)], axis=1)
    cl = np.concatenate([st, np.zeros((n, 1))], axis=1)
    flags = np.array([0, 16, 24, 8, 4, 20, 1, 3, 0, 16, 0, 0])
    plain, fric = squeeze_metric(st, cl, cl, flags), squeeze_metric(st, cl, cl, flags, friction=0.25)
    assert set(fric) - set(plain) == {"squeeze_friction", "squeeze_jammed"} and set(plain) <= set(fric)
    assert fric["squeeze_friction"] == 0.25 and fric["squeeze_jammed"] == 4 and fric["simulated"] == "squeeze"
    assert plain.keys() == squeeze_metric(st, cl, cl, flags, friction=0.0).keys()


def test_stats_json_records_the_friction(tmp_path):
    from dgdm_amd import engine
    from dgdm_amd.dynamics.dataloader import load_score_stats
    from dgdm_amd.sim import sim_2d
    n = 20
    starts = np.zeros((n, 3))
    start = np.zeros((n, 2))
    closed = np.stack([np.linspace(0, 0.3, n), np.linspace(0, 0.01, n), np.linspace(0, 0.02, n)], axis=1)
    rec = sim_2d.pair_record(np.zeros((14, 2)), np.zeros((400, 2)), RECT, starts, start, closed)
    cfg = engine.squeeze_config(theta_cells=360, x_cells=41)
    sim_2d.write_dataset(str(tmp_path / "a"), [(7, 3, rec)], cfg, 0, 0.25)
    stats = json.load(open(tmp_path / "a" / "stats.json"))
    assert stats["friction"] == 0.25 and stats["simulated"] == "squeeze"
    assert len(load_score_stats(str(tmp_path / "a" / "stats.json"))["score_std"]) == 3
    sim_2d.write_dataset(str(tmp_path / "b"), [(7, 3, rec)], cfg, 0)                # other writers (sim_3d) keep their keys
    assert "friction" not in json.load(open(tmp_path / "b" / "stats.json"))
