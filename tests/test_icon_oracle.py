"""CPU tests of the icon-contour oracle (tests/icon_oracle.py, DESIGN.md "Object contours from icon images") against known answers, and
of the host-side decisions around it: argument checks before any launch and the object choice of generator/train.py."""
import argparse

import numpy as np
import pytest
import torch

from tests import icon_oracle as orc


def mask_of(*boxes, size=128):
    """A bool mask with the given filled boxes (x0, y0, x1, y1), inclusive."""
    m = np.zeros((size, size), dtype=bool)
    for x0, y0, x1, y1 in boxes:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


# ------------------------------------------------------------------------------------------------------------------ contours
def test_rectangle_corner_order():
    assert orc.external_contours(mask_of((5, 10, 29, 19))) == [[(5, 10), (5, 19), (29, 19), (29, 10)]]
    assert orc.external_contours(np.ones((128, 128), dtype=bool)) == [[(0, 0), (0, 127), (127, 127), (127, 0)]]


def test_single_pixel_line_and_l_shape():
    assert orc.external_contours(mask_of((4, 3, 4, 3))) == [[(4, 3)]]
    assert orc.external_contours(mask_of((2, 5, 8, 5))) == [[(2, 5), (8, 5)]]           # horizontal: out and back
    assert orc.external_contours(mask_of((7, 1, 7, 9))) == [[(7, 1), (7, 9)]]           # vertical
    diag = np.zeros((128, 128), dtype=bool)
    for i in range(5):
        diag[10 + i, 20 + i] = True
    assert orc.external_contours(diag) == [[(20, 10), (24, 14)]]
    L = mask_of((10, 10, 12, 30), (10, 28, 40, 30))
    # the concave corner is cut diagonally (8-connected border following)
    assert orc.external_contours(L) == [[(10, 10), (10, 30), (40, 30), (40, 28), (13, 28), (12, 27), (12, 10)]]
    # arc lengths: 2 x 6 for the line, the L's perimeter
    assert orc.arc_length([(2, 5), (8, 5)]) == 12.0
    assert orc.arc_length([(10, 10), (10, 30), (40, 30), (40, 28), (13, 28), (12, 27), (12, 10)]) == \
        20 + 30 + 2 + 27 + float(np.sqrt(np.float32(2))) + 17 + 2
    assert orc.arc_length([(4, 3)]) == 0.0
    assert orc.arc_length([(20, 10), (24, 14)]) == 2 * float(np.sqrt(np.float32(32)))


def test_shape_touching_the_edges():
    m = mask_of((0, 0, 127, 3), (120, 0, 127, 127))
    assert orc.external_contours(m) == [[(0, 0), (0, 3), (119, 3), (120, 4), (120, 127), (127, 127), (127, 0)]]


def test_component_in_a_hole_is_ignored():
    # a ring 4 px thick around a 40 x 40 hole; inside it a comb whose perimeter is longer than the ring's
    ring = mask_of((10, 10, 59, 13), (10, 56, 59, 59), (10, 10, 13, 59), (56, 10, 59, 59))
    comb = mask_of(*[(16 + 4 * k, 16, 17 + 4 * k, 53) for k in range(10)], (16, 52, 54, 53))
    cs = orc.external_contours(ring | comb)
    assert len(cs) == 1 and cs[0] == [(10, 10), (10, 59), (59, 59), (59, 10)]
    inner = orc.external_contours(comb)
    assert len(inner) == 1 and orc.arc_length(inner[0]) > orc.arc_length(cs[0])
    assert orc.largest_contour(ring | comb) == cs[0]


def test_two_components_longest_wins_and_ties_go_to_the_later():
    small, big = (5, 5, 10, 10), (30, 40, 60, 70)
    assert orc.largest_contour(mask_of(small, big)) == [(30, 40), (30, 70), (60, 70), (60, 40)]
    assert orc.largest_contour(mask_of(big, (80, 2, 85, 7))) == [(30, 40), (30, 70), (60, 70), (60, 40)]
    # equal squares: the one whose start pixel comes later in raster order wins (cv2 lists contours newest first, argmax the first)
    a, b = (70, 10, 79, 19), (10, 30, 19, 39)
    cs = orc.external_contours(mask_of(a, b))
    assert [c[0] for c in cs] == [(70, 10), (10, 30)] and orc.arc_length(cs[0]) == orc.arc_length(cs[1])
    assert orc.largest_contour(mask_of(a, b)) == cs[1]
    assert orc.largest_contour(np.zeros((128, 128), dtype=bool)) is None


# ------------------------------------------------------------------------------------------------------------------ pixels
def test_resize_constant_identity_area_and_weights():
    rs = np.random.RandomState(0)
    for H, W in ((32, 32), (17, 45), (300, 90), (256, 256), (1, 1)):
        c = rs.randint(0, 256, size=3).astype(np.uint8)
        img = np.broadcast_to(c, (H, W, 3)).copy()
        out = orc.resize(img)
        assert out.shape == (128, 128, 3) and (out == c).all(), (H, W)
    img = rs.randint(0, 256, size=(128, 128, 4)).astype(np.uint8)
    assert np.array_equal(orc.resize(img), img)
    img = rs.randint(0, 256, size=(256, 256, 3)).astype(np.uint8)
    S = img.astype(np.int64)
    assert np.array_equal(orc.resize(img), ((S[::2, ::2] + S[::2, 1::2] + S[1::2, ::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    sx, w0, w1 = orc.linear_taps(32)
    assert list(sx[:6]) == [0, 0, 0, 0, 0, 0] and list(sx[6:10]) == [1, 1, 1, 1] and list(sx[-2:]) == [31, 31]
    assert list(w0[2:6]) == [1792, 1280, 768, 256] and list(w1[2:6]) == [256, 768, 1280, 1792]
    assert set(zip(w0[2:-2].tolist(), w1[2:-2].tolist())) == {(1792, 256), (1280, 768), (768, 1280), (256, 1792)}
    assert (w0 + w1 == 2048).all()


def test_resize_vector_form_differs_from_the_scalar_form():
    """The contract's vertical pass is OpenCV's vector form; the scalar form rounds differently on some pixels."""
    img = np.random.RandomState(1).randint(0, 256, size=(32, 32, 3)).astype(np.uint8)
    v, s = orc.resize(img).astype(int), orc.resize_scalar(img).astype(int)
    assert 0 < int((v != s).sum()) and np.abs(v - s).max() <= 1


def test_grey_threshold_boundary():
    def fg(b, g, r):
        return bool(orc.foreground(np.full((128, 128, 3), (b, g, r), dtype=np.uint8))[0, 0])
    assert orc.grey(np.array([[[240, 240, 240]], [[241, 241, 241]]], dtype=np.uint8)).ravel().tolist() == [240, 241]
    assert fg(240, 240, 240) and not fg(241, 241, 241)
    assert orc.grey(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], dtype=np.uint8)).ravel().tolist() == [29, 150, 76]
    assert not fg(255, 255, 255) and fg(0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------ resample
def test_resample_hand_computed():
    # a 3-4-5 polyline: c = [0, 5, 10], L = 10; n = 5 -> u = 0, 2.5, 5, 7.5, 10
    p = [(0, 0), (3, 4), (6, 8)]
    assert orc.resample(p, 5).tolist() == [[0, 0], [1, 2], [3, 4], [4, 6], [6, 8]]
    assert orc.resample(p, 1).tolist() == [[0, 0]]
    assert orc.resample(p, 2).tolist() == [[0, 0], [6, 8]]
    assert orc.resample([(7, 9)], 3).tolist() == [[7, 9]] * 3                       # K = 1
    assert orc.resample([(7, 9), (7, 9), (7, 9)], 4).tolist() == [[7, 9]] * 4       # L = 0
    # negative coordinates truncate toward zero; repeated points take the last of the tied ones
    assert orc.resample([(0, 0), (-3, -3)], 3).tolist() == [[0, 0], [-1, -1], [-3, -3]]
    assert orc.resample([(0, 0), (0, 0), (10, 0)], 3).tolist() == [[0, 0], [5, 0], [10, 0]]
    assert orc.rescale(np.array([[0, 64, 128]])).tolist() == [[-0.05, 64 / 128 * 0.1 - 0.05, 128 / 128 * 0.1 - 0.05]]


def test_resample_matches_numpy_on_random_polylines():
    rs = np.random.RandomState(2)
    for K, n in ((1, 5), (2, 1), (2, 100), (7, 1000), (50, 100), (300, 2)):
        p = rs.randint(-40, 170, size=(K, 2)).astype(np.int32)
        p[rs.rand(K) < 0.2] = p[0]
        d = np.sqrt(np.sum(np.diff(p, axis=0) ** 2, axis=1))
        c = np.cumsum(np.insert(d, 0, 0))
        u = np.linspace(0, c[-1], n)
        ref = np.vstack((np.interp(u, c, p[:, 0]), np.interp(u, c, p[:, 1]))).T.astype(np.int32)
        assert np.array_equal(orc.resample(p, n), ref), (K, n)


# ------------------------------------------------------------------------------------------------------------------ host decisions
def test_argument_errors_before_any_launch():
    from dgdm_amd import engine
    from dgdm_amd.assets import icon_process
    ok = np.zeros((32, 32, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        icon_process.extract_contours(ok.astype(np.float32))
    with pytest.raises(ValueError, match="shape"):
        icon_process.extract_contours(ok[..., 0])
    with pytest.raises(ValueError, match="shape"):
        icon_process.extract_contours(np.zeros((32, 32, 2), dtype=np.uint8))
    with pytest.raises(ValueError, match="shape"):
        icon_process.extract_contours_batch(ok)
    with pytest.raises(ValueError, match="uint8"):
        engine.icon_contours(torch.zeros((1, 32, 32, 3), dtype=torch.int16))
    with pytest.raises(ValueError, match="shape"):
        engine.icon_contours(torch.zeros((1, 32, 32, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="num_points 0"):
        engine.icon_contours(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="integer"):
        icon_process.resample_contour(np.zeros((3, 1, 2), dtype=np.float64), 10)


def test_objects_2d_without_the_icon_file(tmp_path, capsys):
    from dgdm_amd import synth
    from dgdm_amd.generator.train import OBJECT_IDS, _objects
    missing = str(tmp_path / "nowhere" / "Icons-50.npy")
    objs, ids = _objects(argparse.Namespace(object_dir=missing, object_max_num_vertices=100), False)
    err = capsys.readouterr().err
    assert ids == list(OBJECT_IDS) and "synthetic objects" in err and missing in err and "no such file" in err
    assert torch.equal(objs[0], synth.synth_object_2d(0, 100))
    # a file that is not a pickled dict with 'image': named as unreadable, still the synthetic objects
    bad = str(tmp_path / "Icons-50.npy")
    np.save(bad, np.zeros(3))
    objs, ids = _objects(argparse.Namespace(object_dir=bad, object_max_num_vertices=100), False)
    err = capsys.readouterr().err
    assert "synthetic objects" in err and bad in err and "unreadable" in err and objs.shape == (8, 100, 2)


def test_objects_2d_vertex_count_must_be_100(tmp_path):
    from dgdm_amd.generator.train import _objects
    f = str(tmp_path / "Icons-50.npy")
    np.save(f, {"image": np.zeros((10001, 3, 4, 4), dtype=np.uint8)}, allow_pickle=True)
    with pytest.raises(ValueError, match="object_max_num_vertices=64.*100 points"):
        _objects(argparse.Namespace(object_dir=f, object_max_num_vertices=64), False)
