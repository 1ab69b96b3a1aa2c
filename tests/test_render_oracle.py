"""The rasteriser's contract on the CPU (tests/render_oracle.py; include/dgdm_hip.h "mesh rendering"): the coverage rule
on cases counted by hand, the two oracles against each other, and the host side of dgdm_amd/sim/render_mesh.py (camera, polyline,
argument errors).  Nothing here touches a GPU."""
import numpy as np
import pytest

from dgdm_amd import engine
from dgdm_amd.sim import render_mesh as rm
from tests import render_oracle as ro
from tests import render_scenes as sc


def cover_sum(tris_px, W, H):
    return sum(ro.cover_mask(sc.snapped_px(t), W, H).astype(int) for t in tris_px)


def test_rectangle_on_pixel_centres_covers_twelve_pixels():
    s = cover_sum(sc.RECTANGLE, 8, 6)
    want = np.zeros((6, 8), dtype=int)
    want[0:3, 0:4] = 1
    assert np.array_equal(s, want) and s.sum() == 12


@pytest.mark.parametrize("flip", [False, True])
def test_shared_edges_and_fans_cover_each_centre_once(flip):
    """The diagonal of the rectangle and the eight spokes of the fan pass through pixel centres; so does the fan's hub."""
    order = (lambda t: [t[0], t[2], t[1]]) if flip else (lambda t: t)
    s = cover_sum([order(t) for t in sc.FAN], 12, 12)
    want = np.zeros((12, 12), dtype=int)
    want[1:9, 1:9] = 1
    assert np.array_equal(s, want)
    quad = [[(1, 1), (7, 1), (7, 7)], [(7, 7), (1, 7), (1, 1)]]
    s = cover_sum([order(t) for t in quad], 9, 9)
    want = np.zeros((9, 9), dtype=int)
    want[1:7, 1:7] = 1
    assert np.array_equal(s, want)


def test_degenerate_triangle_covers_nothing():
    assert not ro.cover_mask([(128, 128), (640, 640), (1152, 1152)], 8, 8).any()


def test_contract_matches_the_float64_rasteriser_on_the_dyadic_scene():
    """Dyadic vertices and matrices: both oracles see the same coverage exactly; depth differs by float32 rounding, a colour by one level."""
    scene = sc.contract_scene()
    ia, da, ca, ra, _ = sc.oracle_a(ro, scene)
    ib, db, cb, rb = sc.oracle_b(ro, scene)
    assert np.array_equal(ia, ib) and np.array_equal(ra, rb) and not ra.any()
    assert len({int(v) for v in ia.ravel()}) == 5                    # the four ids and the background are all seen
    hit = ia >= 0
    assert np.abs(da[hit].astype(np.float64) - db[hit]).max() < 1e-6 and np.isinf(da[~hit]).all()
    assert np.abs(ca.astype(int) - cb.astype(int)).max() <= 1
    assert (ca[~hit] == 255).all()


def test_free_camera():
    W, H = 64, 48
    for az, el in ((180.0, -30.0), (135.0, -45.0), (20.0, 10.0)):
        look = np.array([0.1, -0.05, 0.02])
        M, eye = rm.free_camera(look, 0.9, az, el, W, H)
        f = np.array([np.cos(np.deg2rad(el)) * np.cos(np.deg2rad(az)), np.cos(np.deg2rad(el)) * np.sin(np.deg2rad(az)), np.sin(np.deg2rad(el))])
        assert np.allclose(eye, look - 0.9 * f, atol=1e-15)
        proj = lambda p: (lambda c: c[:3] / c[3])(M @ np.append(p, 1.0))          # noqa: E731
        c = proj(look)
        assert np.allclose(c[:2], [W / 2, H / 2], atol=1e-9)                      # lookat lands on the image centre
        up = proj(look + [0, 0, 0.1])
        assert abs(up[0] - W / 2) < 1e-9 and up[1] < H / 2 - 1                    # a point above lookat lands above it (pixel y points down)
        d = [proj(eye + t * f)[2] for t in (0.02, 0.5, 0.9, 3.0, 40.0)]
        assert all(a < b for a, b in zip(d, d[1:])) and 0.0 < d[0] and d[-1] < 1.0   # depth grows with distance
        ws = np.array([0.5, 1.0, 2.0])
        zs = np.array([proj(eye + w * f)[2] for w in ws])
        assert np.allclose(np.diff(zs) / np.diff(1.0 / ws), (zs[2] - zs[0]) / (1 / ws[2] - 1 / ws[0]))    # affine in 1 / c_3
        # the vertical field of view: a point fovy / 2 above the axis lands on the top row's upper edge
        r = np.cross(f, [0, 0, 1.0])
        u = np.cross(r / np.linalg.norm(r), f)
        top = proj(eye + f + np.tan(np.deg2rad(22.5)) * u)
        assert np.allclose(top[:2], [W / 2, 0.0], atol=1e-9)
    with pytest.raises(ValueError, match="z axis"):
        rm.free_camera((0, 0, 0), 1.0, 0.0, -90.0, 8, 8)
    with pytest.raises(ValueError):
        rm.free_camera((0, 0, 0), 0.0, 0.0, -30.0, 8, 8)
    with pytest.raises(ValueError):
        rm.free_camera((0, 0, 0), 1.0, 0.0, -30.0, 8, 8, near=1.0, far=0.5)


def test_draw_polyline():
    img = np.full((8, 9, 3), 255, dtype=np.uint8)
    out = rm.draw_polyline(img, np.array([[1, 1], [6, 1], [6, 5], [1, 5]], dtype=np.int32), (38, 80, 115))
    assert out is img
    want = np.zeros((8, 9), dtype=bool)
    want[1, 1:7] = want[5, 1:7] = True
    want[1:6, 1] = want[1:6, 6] = True
    assert np.array_equal((img == (38, 80, 115)).all(axis=2), want) and (img[~want] == 255).all()
    one = np.zeros((4, 4, 3), dtype=np.uint8)
    rm.draw_polyline(one, np.array([[2, 1]]), (9, 8, 7))
    assert one[1, 2].tolist() == [9, 8, 7] and int((one != 0).any(axis=2).sum()) == 1
    diag = np.zeros((6, 6, 3), dtype=np.uint8)
    rm.draw_polyline(diag, np.array([[0, 0], [4, 4]]), (1, 1, 1))                 # 8-connected: a diagonal is one pixel per step
    assert int(diag[..., 0].sum()) == 5 and all(diag[k, k, 0] for k in range(5))
    clip = np.zeros((3, 3, 3), dtype=np.uint8)
    rm.draw_polyline(clip, np.array([[-2, 1], [5, 1]]), (1, 1, 1))                # outside pixels are skipped
    assert clip[1, :, 0].tolist() == [1, 1, 1] and int(clip[..., 0].sum()) == 3
    with pytest.raises(ValueError, match="integer"):
        rm.draw_polyline(img, np.array([[0.5, 1.0]]), (0, 0, 0))
    with pytest.raises(ValueError):
        rm.draw_polyline(np.zeros((4, 4)), np.array([[0, 0]]), (0, 0, 0))
    with pytest.raises(ValueError, match="no points"):
        rm.draw_polyline(img, np.zeros((0, 2), dtype=np.int32), (0, 0, 0))


def test_argument_errors_before_any_launch():
    s = sc.engine_args(sc.contract_scene())
    with pytest.raises(ValueError, match="come together"):
        engine.render_meshes(**{**s, "eyes": None})
    with pytest.raises(ValueError, match=r"\(n_inst, 4, 4\)"):
        engine.render_meshes(**{**s, "inst_matrix": s["inst_matrix"][:3]})
    with pytest.raises(ValueError, match="colours"):
        engine.render_meshes(**{**s, "inst_rgb": s["inst_rgb"][:2]})
    with pytest.raises(ValueError, match="view indices"):
        engine.render_meshes(**{**s, "inst_view": np.array([0, 1, 2, 3])})
    with pytest.raises(ValueError, match=r"\(B, 2, V, 3\)"):
        import torch
        rm.render_grippers(torch.zeros(3, 5, 3), np.zeros((1, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="at least one rotation"):
        rm.object_silhouettes(np.zeros((3, 3)), np.zeros((1, 3), dtype=np.int32), [])


def test_reference_module_path():
    import sim.render_mesh as ref_path
    assert ref_path is rm and callable(ref_path.render_mesh) and callable(ref_path.render_object_mesh)
