"""Scenes shared by the rasteriser's CPU and GPU tests (tests/test_render_oracle.py, tests/test_gpu_render.py): plain numpy tables in
the form engine.render_meshes and the oracles of tests/render_oracle.py take."""
import numpy as np

IDENT = np.eye(4)


def concat(meshes):
    """[(verts (V, 3), tris (T, 3) local)] -> verts, tris, (vertex offsets, triangle offsets)."""
    vo = np.cumsum([0] + [len(v) for v, _ in meshes]).astype(np.int64)
    to = np.cumsum([0] + [len(t) for _, t in meshes]).astype(np.int64)
    return (np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 3) for v, _ in meshes]),
            np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1, 3) for _, t in meshes]), (vo, to))


def pixel_tris(tris_px, z=0.5):
    """Triangles given by pixel-CENTRE coordinates ((x, y) = pixel (x, y)'s sample) -> a mesh for the identity matrix."""
    v = np.array([[x + 0.5, y + 0.5, z] for t in tris_px for x, y in t], dtype=np.float64)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def snapped_px(tri_px):
    """The snapped (X, Y) of a triangle given by pixel-centre coordinates."""
    return [(int(round(256 * x)) + 128, int(round(256 * y)) + 128) for x, y in tri_px]


RECTANGLE = [[(0, 0), (4, 0), (4, 3)], [(0, 0), (4, 3), (0, 3)]]                   # corners on the pixel centres (0, 0) and (4, 3)
FAN_RING = [(9, 5), (9, 9), (5, 9), (1, 9), (1, 5), (1, 1), (5, 1), (9, 1)]
FAN = [[(5, 5), FAN_RING[k], FAN_RING[(k + 1) % 8]] for k in range(8)]           # tiles the square (1, 1) .. (9, 9); spokes through centres


def contract_scene():
    """3 views of 40 x 24, 3 meshes, 4 instances (listed out of view order; mesh 1 twice under different matrices).  Every vertex and
    matrix entry is dyadic and every w is a power of two, so projection and snapping are exact in float32 and float64 alike.  Mesh 0: 300
    small random triangles (more than one chunk of 256), each at its own constant depth 0.1 + t / 1024; mesh 1: a sloped quad larger than
    the image, depth 0.6 .. 0.9 (0.3 .. 0.45 under the second matrix, alone in its view); mesh 2: a fan around a pixel centre."""
    rs = np.random.RandomState(11)
    c = rs.randint(-4 * 64, 44 * 64, size=(300, 1, 2)) / 64.0
    c[:, :, 1] = rs.randint(-4 * 64, 28 * 64, size=(300, 1)) / 64.0
    xy = c + rs.randint(-3 * 64, 3 * 64 + 1, size=(300, 3, 2)) / 64.0
    z = 0.1 + np.arange(300) / 1024.0
    v0 = np.concatenate([xy, np.repeat(z[:, None, None], 3, axis=1)], axis=2).reshape(-1, 3)
    t0 = np.arange(900, dtype=np.int32).reshape(-1, 3)
    v1 = np.array([[-6.25, -3.5, 0.6], [50.75, -2.25, 0.7], [47.5, 30.125, 0.9], [-3.125, 27.75, 0.75]])
    t1 = np.array([[0, 1, 2], [0, 3, 2]], dtype=np.int32)                 # the second one is wound the other way
    ring = [(30.5, 4.25), (33.0, 15.5), (22.75, 21.0), (8.25, 17.5), (6.5, 6.125)]
    v2 = np.array([[20.5, 12.5, 0.45]] + [[x, y, 0.55] for x, y in ring])
    t2 = np.array([[0, 1 + k, 1 + (k + 1) % 5] for k in range(5)], dtype=np.int32)
    verts, tris, offsets = concat([(v0, t0), (v1, t1), (v2, t2)])
    m_a = np.eye(4)
    m_b = np.array([[1.0, 0.0, 0.0, -8.0], [0.0, 0.5, 0.0, 4.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 2.0]])      # w = 2: halves everything
    m_c = np.array([[0.0, -1.0, 0.0, 34.0], [1.0, 0.0, 0.0, -8.0], [0.0, 0.0, 0.5, 0.25], [0.0, 0.0, 0.0, 1.0]])   # a quarter turn
    cams = np.stack([m_a, m_b, m_c])
    view = np.array([2, 0, 1, 0], dtype=np.int32)
    mesh = np.array([2, 0, 1, 1], dtype=np.int32)
    return dict(verts=verts, tris=tris, offsets=offsets, inst_view=view, inst_mesh=mesh, inst_matrix=cams[view], inst_id=np.array([9, 7, 5, 3], dtype=np.int32),
                n_views=3, width=40, height=24, inst_rgb=np.array([[0.25, 0.5, 1.0], [1.0, 0.75, 0.125], [0.5, 0.5, 0.5], [0.0, 1.0, 0.375]]),
                eyes=np.array([[20.0, 12.0, -30.0], [-16.0, 40.0, -8.0], [64.0, 2.0, -12.0]]), cams=cams)


def box(lo, hi):
    """An axis-aligned box as 8 vertices and 12 triangles."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = np.array([[x, y, z] for z in (z0, z1) for y in (y0, y1) for x in (x0, x1)], dtype=np.float64)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], dtype=np.int32)


def rot_z(angle, pos=(0.0, 0.0, 0.0)):
    m = np.eye(4)
    c, s = np.cos(angle), np.sin(angle)
    m[:2, :2] = [[c, -s], [s, c]]
    m[:3, 3] = pos
    return m


def sanity_scene(free_camera):
    """A perspective scene (2 views of 56 x 44) of three horizontal plates 0.2 m apart seen from 45 degrees above: where two overlap on
    the screen they are 0.28 m apart along the ray, more than 4e-3 in depth - three orders above float32 interpolation error."""
    quad = lambda h, z: (np.array([[-h, -h, z], [h, -h, z], [h, h, z], [-h, h, z]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))   # noqa: E731
    verts, tris, offsets = concat([quad(0.28125, -0.203125), quad(0.171875, 0.0), quad(0.09375, 0.203125)])
    cam0, eye0 = free_camera((0.0, 0.0, 0.0), 0.8, 135.0, -45.0, 56, 44)
    cam1, eye1 = free_camera((0.015625, 0.0, 0.0), 0.9, 180.0, -30.0, 56, 44)
    view = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    mesh = np.array([0, 1, 2, 2, 1, 0], dtype=np.int32)
    models = np.stack([rot_z(0.3), rot_z(-0.625), rot_z(1.1, (0.03125, 0.0, 0.0)), rot_z(0.2), rot_z(2.0), rot_z(-1.3)])
    cams = np.stack([cam0, cam1])
    return dict(verts=verts, tris=tris, offsets=offsets, inst_view=view, inst_mesh=mesh, inst_matrix=cams[view] @ models,
                inst_id=np.array([1, 2, 3, 4, 5, 6], dtype=np.int32), n_views=2, width=56, height=44,
                inst_rgb=np.array([[0.9, 0.2, 0.2], [0.2, 0.9, 0.2], [0.2, 0.2, 0.9]] * 2), eyes=np.stack([eye0, eye1]), inst_model=models, cams=cams)


def model_eyes(scene):
    """Each instance's eye in its model frame, float32: what engine.render_meshes hands the library."""
    n = len(scene["inst_view"])
    e = np.concatenate([scene["eyes"][scene["inst_view"]], np.ones((n, 1))], axis=1)
    if "inst_model" in scene:
        e = np.einsum('nij,nj->ni', np.linalg.inv(scene["inst_model"]), e)
    return (e[:, :3] / e[:, 3:4]).astype(np.float32)


def oracle_a(ro, scene):
    return ro.render_contract(scene["verts"], scene["tris"], scene["offsets"], scene["inst_view"], scene["inst_mesh"],
                              scene["inst_matrix"].astype(np.float32), scene["inst_id"], scene["n_views"], scene["width"], scene["height"],
                              scene["inst_rgb"].astype(np.float32), model_eyes(scene))


def oracle_b(ro, scene):
    n = len(scene["inst_view"])
    return ro.render_float64(scene["verts"].astype(np.float32), scene["tris"], scene["offsets"], scene["inst_view"], scene["inst_mesh"],
                             scene.get("inst_model", np.tile(IDENT, (n, 1, 1))), scene["cams"], scene["eyes"], scene["inst_id"], scene["inst_rgb"],
                             scene["n_views"], scene["width"], scene["height"])


def engine_args(scene):
    return {k: v for k, v in scene.items() if k != "cams"}
