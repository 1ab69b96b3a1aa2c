"""The mesh rasteriser on the GPU (csrc/render.hip, engine.render_meshes, dgdm_amd/sim/render_mesh.py) against the CPU oracles of
tests/render_oracle.py: (a) the contract of include/dgdm_hip.h "mesh rendering" / DESIGN.md §4.5e, bit for bit in the snapped vertices,
ids and depth; (b) the independent float64 rasteriser, for the colours (within one level: one float32-against-float64 rounding of the
shade can move a rintf by one step and no more) and as a sanity check of the whole.  Then the reference-shaped functions and the
predicted simulator's --predicted_render."""
import functools
import os
import shlex

import numpy as np
import pytest
import torch

from dgdm_amd import engine
from dgdm_amd.sim import render_mesh as rm
from tests import render_oracle as ro
from tests import render_scenes as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def host(out):
    return [None if t is None else t.cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def contract():
    scene = sc.contract_scene()
    return scene, sc.oracle_a(ro, scene), sc.oracle_b(ro, scene)


def test_contract_scene_bit_for_bit(dev):
    """3 views of 40 x 24 (not square, no multiple of the tile), 3 meshes, 4 instances out of view order, 300 triangles in one mesh."""
    scene, a, b = contract()
    ids, depth, rgb, rejected, snapped = host(engine.render_meshes(**sc.engine_args(scene), snapped=True))
    assert np.array_equal(snapped, a[4])
    assert np.array_equal(ids, a[0]) and not rejected.any()
    assert np.array_equal(depth.view(np.int32), a[1].view(np.int32))
    assert np.array_equal(ids, b[0])
    d = np.abs(rgb.astype(int) - b[2].astype(int))
    print("contract scene: max colour difference to the float64 oracle", int(d.max()), "levels; to the contract", int(np.abs(rgb.astype(int) - a[2].astype(int)).max()))
    assert d.max() <= 1
    assert (rgb[ids < 0] == 255).all() and np.isinf(depth[ids < 0]).all()
    no_rgb = host(engine.render_meshes(**{**sc.engine_args(scene), "inst_rgb": None, "eyes": None}))
    assert no_rgb[2] is None and np.array_equal(no_rgb[0], ids) and np.array_equal(no_rgb[1].view(np.int32), depth.view(np.int32))


def test_float64_sanity_scene(dev):
    """A perspective scene whose surfaces are >= 4e-3 apart in depth where they overlap: only a pixel centre on a snapped edge could
    differ from the float64 rasteriser, and for these vertices the contract oracle has none (asserted first, on the CPU)."""
    scene = sc.sanity_scene(rm.free_camera)
    a, b = sc.oracle_a(ro, scene), sc.oracle_b(ro, scene)
    assert np.array_equal(a[0], b[0])
    ids, depth, rgb, rejected = host(engine.render_meshes(**sc.engine_args(scene)))
    assert np.array_equal(ids, b[0]) and not rejected.any()
    assert set(np.unique(ids)) == {-1, 1, 2, 3, 4, 5, 6}
    assert np.array_equal(depth.view(np.int32), a[1].view(np.int32))
    assert np.abs(depth[ids >= 0].astype(np.float64) - b[1][ids >= 0]).max() < 1e-6
    assert np.abs(rgb.astype(int) - b[2].astype(int)).max() <= 1


def one_per_view(tris_px, W, H, z=0.5):
    """Every triangle (pixel-centre coordinates) alone in its own view under the identity matrix -> coverage masks (n, H, W)."""
    v, t = sc.pixel_tris(tris_px, z)
    n = len(t)
    meshes = [(v[3 * k:3 * k + 3], np.array([[0, 1, 2]], dtype=np.int32)) for k in range(n)]
    verts, tris, offsets = sc.concat(meshes)
    ids = engine.render_meshes(verts, tris, offsets, np.arange(n), np.arange(n), np.tile(np.eye(4), (n, 1, 1)), np.arange(n), n, W, H)[0]
    return (ids.cpu().numpy() >= 0)


def test_coverage_partitions(dev):
    m = one_per_view(sc.RECTANGLE, 8, 6)
    want = np.zeros((6, 8), dtype=int)
    want[0:3, 0:4] = 1
    assert np.array_equal(m.sum(axis=0), want)
    for flip in (False, True):
        fan = [[t[0], t[2], t[1]] if flip else t for t in sc.FAN]
        m = one_per_view(fan, 12, 12)
        want = np.zeros((12, 12), dtype=int)
        want[1:9, 1:9] = 1
        assert np.array_equal(m.sum(axis=0), want)
        for k, t in enumerate(fan):
            assert np.array_equal(m[k], ro.cover_mask(sc.snapped_px(t), 12, 12)), k


def test_coverage_across_tiles_and_outside_the_image(dev):
    """One triangle over the corner where four 16 x 16 tiles meet; one reaching out of the image on three sides; slivers and a
    triangle without area."""
    tris = [[(9.25, 11.5), (27.75, 13.0), (14.5, 22.25)], [(-7.5, -3.25), (51.0, 9.5), (18.25, 40.0)], [(2.0, 2.0), (37.0, 2.25), (20.0, 2.0)],
            [(3.0, 3.0), (9.0, 9.0), (15.0, 15.0)], [(31.5, 15.5), (32.5, 15.5), (31.5, 16.5)]]
    m = one_per_view(tris, 40, 24)
    for k, t in enumerate(tris):
        want = ro.cover_mask(sc.snapped_px(t), 40, 24)
        assert np.array_equal(m[k], want), k
    assert m[0].sum() > 50 and m[1].sum() > 300 and not m[3].any()


def test_equal_depth_goes_to_the_earlier_instance_then_the_lower_triangle(dev):
    v, t = sc.pixel_tris([[(2, 1), (30, 4), (11, 20)]] * 2)
    verts, tris, offsets = sc.concat([(v, t)])
    eye4 = np.tile(np.eye(4), (2, 1, 1))
    for id_first, id_second in ((4, 8), (8, 4)):
        ids = engine.render_meshes(verts, tris, offsets, [0, 0], [0, 0], eye4, [id_first, id_second], 1, 40, 24)[0].cpu().numpy()
        assert (ids >= 0).sum() > 100 and set(np.unique(ids)) == {-1, id_first}
    # within one instance: two overlapping triangles in the plane z = 0.5, shaded differently (their centroids see the eye from other
    # directions) - where both cover a pixel the one with the lower index is seen, whichever of the two that is
    pair = [[(2, 1), (30, 4), (11, 20)], [(5, 2), (35, 10), (8, 22)]]
    kw = dict(inst_rgb=[[1.0, 0.5, 0.25]], eyes=[[40.0, 30.0, -20.0]])
    alone = []
    for tri in pair:
        v1, t1 = sc.pixel_tris([tri])
        out = host(engine.render_meshes(v1, t1, (np.array([0, 3]), np.array([0, 1])), [0], [0], np.eye(4)[None], [0], 1, 40, 24, **kw))
        alone.append((out[0][0] >= 0, out[2][0]))
    both = alone[0][0] & alone[1][0]
    assert both.sum() > 100 and not np.array_equal(alone[0][1][both], alone[1][1][both])
    for first in (0, 1):
        v2, t2 = sc.pixel_tris([pair[first], pair[1 - first]])
        rgb = host(engine.render_meshes(v2, t2, (np.array([0, 6]), np.array([0, 2])), [0], [0], np.eye(4)[None], [0], 1, 40, 24, **kw))[2][0]
        assert np.array_equal(rgb[both], alone[first][1][both])
        only = alone[1 - first][0] & ~both
        assert np.array_equal(rgb[only], alone[1 - first][1][only])


def test_rejection(dev):
    """w = z: the vertex at z = -1 is behind the eye.  Its triangle is dropped and counted, the other two are drawn as the oracle says."""
    v = np.array([[2.0, 2.0, 1.0], [30.0, 3.0, 1.0], [12.0, 20.0, 2.0], [5.0, 5.0, -1.0], [33.0, 18.0, 1.0], [20.0, 22.0, 2.0], [38.0, 6.0, 1.0]])
    t = np.array([[0, 1, 2], [3, 1, 2], [4, 5, 6]], dtype=np.int32)
    m = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0.5, 0], [0, 0, 1.0, 0]])
    offsets = (np.array([0, 7]), np.array([0, 3]))
    ids, depth, _, rejected = host(engine.render_meshes(v, t, offsets, [0], [0], m[None], [6], 2, 40, 24))
    a = ro.render_contract(v, t, offsets, [0], [0], m[None], [6], 2, 40, 24)
    assert rejected.tolist() == [1, 0] and a[3].tolist() == [1, 0]
    assert np.array_equal(ids, a[0]) and np.array_equal(depth.view(np.int32), a[1].view(np.int32)) and (ids[0] == 6).sum() > 20 and (ids[1] == -1).all()
    far_v, far_t = sc.box((-0.05, -0.05, 0.0), (0.05, 0.05, 0.1))
    far_v[7] = 2.0 * rm.free_camera(width=32, height=32, **rm.OBJECT_CAMERA)[1]                   # one corner behind the camera
    with pytest.raises(ValueError, match="view 1"):
        _two_view_reject(far_v, far_t)


def _two_view_reject(far_v, far_t):
    """View 0 is fine, view 1 draws a mesh with a corner behind the camera: the module-level call names view 1."""
    good_v, good_t = sc.box((-0.05, -0.05, 0.0), (0.05, 0.05, 0.1))
    verts, tris, offsets = sc.concat([(good_v, good_t), (far_v, far_t)])
    cam, eye = rm.free_camera(width=32, height=32, **rm.OBJECT_CAMERA)
    out = engine.render_meshes(verts, tris, offsets, [0, 1], [0, 1], np.stack([cam, cam]), [0, 0], 2, 32, 32)
    assert out[3].cpu().numpy()[0] == 0 and out[3].cpu().numpy()[1] > 0
    rm._raise_rejected(out[3], "object_silhouettes")


def test_module_call_raises_for_a_vertex_behind_the_camera(dev):
    eye = rm.free_camera(width=128, height=128, **rm.OBJECT_CAMERA)[1]
    v, t = sc.box((-0.05, -0.05, 0.0), (0.05, 0.05, 0.1))
    v[7] = 2.0 * eye
    with pytest.raises(ValueError, match="view 0"):
        rm.object_silhouettes(v, t, [0.0, 0.5])


def test_a_view_does_not_depend_on_the_batch(dev):
    scene, a, _ = contract()
    full = host(engine.render_meshes(**sc.engine_args(scene)))
    for k in range(scene["n_views"]):
        pick = np.flatnonzero(scene["inst_view"] == k)
        alone = host(engine.render_meshes(scene["verts"], scene["tris"], scene["offsets"], np.zeros(len(pick), dtype=np.int32), scene["inst_mesh"][pick],
                                          scene["inst_matrix"][pick], scene["inst_id"][pick], 1, scene["width"], scene["height"],
                                          inst_rgb=scene["inst_rgb"][pick], eyes=scene["eyes"][k:k + 1]))
        assert np.array_equal(alone[0][0], full[0][k]) and np.array_equal(alone[1][0].view(np.int32), full[1][k].view(np.int32))
        assert np.array_equal(alone[2][0], full[2][k]) and alone[3][0] == full[3][k]


def test_bad_arguments_are_value_errors(dev):
    scene, _, _ = contract()
    s = {**sc.engine_args(scene), "inst_rgb": None, "eyes": None}
    with pytest.raises(ValueError, match="view index 3"):
        engine.render_meshes(**{**s, "inst_view": np.array([2, 0, 3, 0])})
    with pytest.raises(ValueError, match="mesh index"):
        engine.render_meshes(**{**s, "inst_mesh": np.array([2, 0, 1, 3])})
    with pytest.raises(ValueError, match="2049"):
        engine.render_meshes(**{**s, "width": 2049})
    with pytest.raises(ValueError, match="offsets"):
        engine.render_meshes(**{**s, "offsets": (np.array([0, 900, 800, 910]), scene["offsets"][1])})
    bad = scene["tris"].copy()
    bad[-1, 2] = 6                                                  # mesh 2 has vertices 0 .. 5
    with pytest.raises(ValueError, match="outside its mesh"):
        engine.render_meshes(**{**s, "tris": bad})


# ------------------------------------------------------------------------------------------------------------------ reference-shaped
def test_render_object_mesh_matches_the_contract_oracle(dev, tmp_path):
    from dgdm_amd.assets.icon_process import extract_contours
    v, t = sc.box((-0.0625, -0.03125, 0.0), (0.046875, 0.0390625, 0.09375))
    os.makedirs(tmp_path / "box")
    engine.write_obj(str(tmp_path / "box" / "model.obj"), v, t)
    z_rots = np.linspace(-1.0, 1.0, 4) * np.pi + np.pi
    got = rm.render_object_mesh(str(tmp_path / "box"), z_rots)
    assert len(got) == 4 and all(c.shape == (100, 2) and c.dtype == np.int32 for c in got)
    cam, _ = rm.free_camera(width=128, height=128, **rm.OBJECT_CAMERA)
    mats = np.stack([cam @ rm.rigid(z_rot=z) for z in z_rots]).astype(np.float32)
    ids = ro.render_contract(v, t, (np.array([0, 8]), np.array([0, 12])), np.arange(4), np.zeros(4, dtype=int), mats, np.zeros(4, dtype=int), 4, 128, 128)[0]
    assert all(300 < (ids[k] == 0).sum() < 3000 for k in range(4))
    for k in range(4):
        img = np.where((ids[k] >= 0)[..., None], 0, 255).astype(np.uint8).repeat(3, axis=2)
        assert np.array_equal(got[k], extract_contours(img, num_points=100, rescale=False)), k
    assert not np.array_equal(got[0], got[1])


def test_render_mesh_of_a_saved_gripper(dev, tmp_path):
    from dgdm_amd import synth
    from dgdm_amd.assets import save_grippers
    x = synth.synth_noise(5, 2, 42).reshape(2, 42, 1).clamp(-1, 1).to(dev)
    dirs = save_grippers(x, str(tmp_path / "sim_model"))
    img = rm.render_mesh(dirs[1])
    assert img.shape == (256, 256, 3) and img.dtype == np.uint8
    batch = rm.render_grippers(engine.finger_mesh_3d(x), engine.finger_mesh_faces(engine.MESH_3D, 25)).cpu().numpy()
    assert batch.shape == (2, 256, 256, 3) and np.array_equal(batch[1], img) and not np.array_equal(batch[0], batch[1])
    drawn = ~(img == 255).all(axis=2)
    r, g, b = (img[..., k].astype(int) for k in range(3))
    left, right = drawn & (r > g + 3) & (g > b + 3), drawn & (g > r + 3) & (r > b + 3)          # the two jaw colours of gripper_render.xml
    assert left.sum() > 200 and right.sum() > 200 and (left | right).sum() == drawn.sum()
    # the left jaw sits at y = -0.18: seen from azimuth 180 (looking along -x with z up, the picture's right is +y) it is on the left half
    assert np.nonzero(left)[1].mean() < 128 < np.nonzero(right)[1].mean()


# ------------------------------------------------------------------------------------------------------------------ the harness
def _mesh_objects(root):
    from dgdm_amd.generator.train import OBJECT_NAMES_3D
    for k, name in enumerate(OBJECT_NAMES_3D):
        v, t = sc.box((-0.03 - 0.005 * k, -0.02, 0.0), (0.025, 0.02 + 0.004 * k, 0.05 + 0.01 * k))
        os.makedirs(os.path.join(root, name))
        engine.write_obj(os.path.join(root, name, "model.obj"), v, t)
    return list(OBJECT_NAMES_3D)


def test_predicted_render(dev, tmp_path, capsys):
    """--predicted_sim --predicted_rollout=2 --predicted_render on mesh-backed objects: the pictures exist under the reference's names,
    and designs, metrics and the CPU generator are exactly those of the run without the flag."""
    from dgdm_amd.dynamics.predicted import PredictedSimulator
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    names = _mesh_objects(str(tmp_path / "objects"))
    common = (f"--mode=test --classifier_guidance --fingers_3d --object_max_num_vertices=512 --ctrlpts_dim=42 --sub_bs=40 --num_fingers=2 --batch_size=2 "
              f"--grid_size=3 --num_pos=3 --num_train_timesteps=15 --num_inference_steps=2 --predicted_sim --predicted_rollout=2 "
              f"--object_dir={tmp_path / 'objects'}")
    runs, models, states = {}, {}, {}
    for tag, extra in (("off", ""), ("on", " --predicted_render")):
        torch.manual_seed(7)
        models[tag], runs[tag] = train(parse(shlex.split(common + extra + f" --save_dir={tmp_path / tag}")))
        states[tag] = torch.get_rng_state()
    for k, v in runs["off"][0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, runs["on"][0][k]), k
    assert torch.equal(states["on"], states["off"])
    assert models["on"].object_mesh_dir == str(tmp_path / "objects") and models["off"].object_mesh_dir is None
    noise_dir = tmp_path / "on" / "val_vis_noise"
    assert sorted(f for f in os.listdir(noise_dir) if f.endswith("_gripper.png")) == sorted(f"{i}_{b}_gripper.png" for i in range(6) for b in range(2))
    assert not [f for _, _, fs in os.walk(tmp_path / "off") for f in fs if f.endswith(".png") and "gripper" in f]

    x = runs["on"][0]["unguided"] if "unguided" in runs["on"][0] else next(v for v in runs["on"][0].values() if isinstance(v, torch.Tensor) and v.dim() == 3)
    x = x.detach().cpu().numpy()[:2]
    objs = names[1:3]
    out = {}
    for tag, flag in (("off", False), ("on", True)):
        sim = PredictedSimulator(models["on"], rollout_interactions=2, render_grippers=flag)
        out[tag] = sim(x, objs, str(tmp_path / ("direct_" + tag)), num_rot=72, ori_range=(-1.0, 1.0), render=False, render_last=True)
    on, off = out["on"], out["off"]
    assert off[0] == [None] * 4 and off[6] == [[], [], [], []] and not os.path.exists(tmp_path / "direct_off")
    assert len(on[1]) == 4 and len(off[1]) == 4
    for ma, mb in zip(on[1], off[1]):
        assert ma.keys() == mb.keys()
        for k in ma:
            assert np.array_equal(ma[k], mb[k]), k
    d = tmp_path / "direct_on"
    assert on[0] == [str(d / f"{i}_{b}_gripper.png") for i in range(2) for b in range(2)] and all(os.path.isfile(p) for p in on[0])
    assert on[6] == [[str(d / f"{i}_{b}" / f"{v}.png") for v in range(2)] for i in range(2) for b in range(2)]
    assert all(os.path.isfile(p) for l in on[6] for p in l)
    from PIL import Image
    g = np.asarray(Image.open(on[0][1]))
    assert g.shape == (256, 256, 3) and np.array_equal(g, np.asarray(Image.open(on[0][3])))          # one gripper, drawn once, on both objects
    frame = np.asarray(Image.open(on[6][0][1]))
    assert frame.shape == (128, 128, 3) and (frame == rm.OVERLAY_COLOUR).all(axis=2).sum() > 30
    for k in (2, 3, 4, 5, 7):
        assert on[k] == off[k]
    # render_last off: the gripper pictures only
    again = PredictedSimulator(models["on"], rollout_interactions=2, render_grippers=True)(x, objs, str(tmp_path / "direct_nolast"), num_rot=72)
    assert again[6] == [[], [], [], []] and all(os.path.isfile(p) for p in again[0])


def test_predicted_render_without_meshes_writes_nothing(dev, tmp_path, capsys):
    from dgdm_amd.generator.train import train
    from dynamics.parser import parse
    common = (f"--mode=test --classifier_guidance --fingers_3d --object_max_num_vertices=512 --ctrlpts_dim=42 --sub_bs=40 --num_fingers=2 --batch_size=2 "
              f"--grid_size=3 --num_pos=3 --num_train_timesteps=15 --num_inference_steps=2 --predicted_sim --predicted_render")
    model, runs = train(parse(shlex.split(common)))
    x = np.zeros((1, 42, 1), dtype=np.float32)
    capsys.readouterr()
    out = model.simulator(x, model._object_ids()[:2], str(tmp_path / "synthetic"), num_rot=36, render_last=True)
    model.simulator(x, model._object_ids()[:1], str(tmp_path / "synthetic"), num_rot=36)
    err = capsys.readouterr().err
    assert err.count("--predicted_render") == 1 and "mesh files" in err
    assert out[0] == [None, None] and out[6] == [[], []] and len(out[1]) == 2 and not os.path.exists(tmp_path / "synthetic")
    with pytest.raises(ValueError, match="--predicted_sim"):
        train(parse(shlex.split(common.replace(" --predicted_sim", ""))))
