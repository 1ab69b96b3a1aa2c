"""``sim/render_mesh.py`` of the reference - pictures of grippers and silhouettes of objects - on the library's own rasteriser
(``engine.render_meshes``, csrc/render.hip) instead of MuJoCo's OpenGL renderer, which is not reproduced: the camera
is the reference's (lookat, distance, azimuth, elevation), the lighting is the project's flat shade, and the ground plane of the
reference's render files is not drawn (it is the white background).

* ``render_mesh(gripper_root)``                   -> (256, 256, 3) uint8, the gripper directory's two finger meshes
* ``render_object_mesh(object_root, z_rots)``     -> a list of (100, 2) int32 contours, one per rotation about z
* ``render_grippers`` / ``object_silhouettes``    the batched forms the two above are thin wrappers of, on device tensors
* ``free_camera``, ``draw_polyline``, ``write_png``  host helpers
"""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np
import torch

from .. import engine

# assets/gripper_render.xml of the reference: <body name="left_jaw" pos="0 -0.18 0" euler="0 0 -45"> with rgba 0.9333 0.7804 0.3490 1,
# <body name="right_jaw" pos="0 0.18 0" euler="0 0 45"> with rgba 0.6941 0.7647 0.5059 1 (MuJoCo's default angle unit is the degree)
JAW_POS = ((0.0, -0.18, 0.0), (0.0, 0.18, 0.0))
JAW_ROT_Z_DEG = (-45.0, 45.0)
JAW_RGB = ((0.9333, 0.7804, 0.3490), (0.6941, 0.7647, 0.5059))
JAW_IDS = (0, 1)
GRIPPER_CAMERA = dict(lookat=(0.0, 0.0, 0.0), distance=0.9, azimuth=180.0, elevation=-30.0)      # sim/render_mesh.py:27-30
GRIPPER_SIZE = 256                                                                                # :25
OBJECT_CAMERA = dict(lookat=(0.0, 0.0, 0.0), distance=0.8, azimuth=135.0, elevation=-45.0)       # :44-47
OBJECT_SIZE = 128                                                                                 # :41
OBJECT_RGB = (0.0, 0.0, 0.0)          # color_maps (:17-21) paints the object's segment black and everything else white
SETTLED_RGB = (0.6, 0.6, 0.6)         # the object in a settled-pose frame (the project's choice: the overlay must stay visible on it)
CONTOUR_POINTS = 100                  # :60
OVERLAY_COLOUR = (38, 80, 115)        # dynamics/sim_test_mj_3d.py:222


def free_camera(lookat, distance, azimuth, elevation, width, height, fovy=45.0, near=0.01, far=50.0) -> Tuple[np.ndarray, np.ndarray]:
    """MuJoCo's free camera as one matrix: (M (4, 4) float64, eye (3,)).  M maps a world point (x, y, z, 1) to (c_0, c_1, c_2, c_3) with
    pixel x = c_0 / c_3 (to the right), pixel y = c_1 / c_3 (down; pixel (i, j) is sampled at (i + 0.5, j + 0.5)) and depth c_2 / c_3.
    Angles in degrees.  The forward direction is f = (cos el cos az, cos el sin az, sin el), eye = lookat - distance f, world z is up,
    the vertical field of view is fovy.  c_3 is the distance along f; depth = far / (far - near) (1 - near / c_3): 0 at the near plane,
    1 at the far plane, increasing with distance, affine in 1 / c_3."""
    lookat = np.asarray(lookat, dtype=np.float64).reshape(3)
    width, height = int(width), int(height)
    if not (distance > 0 and width >= 1 and height >= 1 and 0.0 < fovy < 180.0 and 0.0 < near < far):
        raise ValueError(f"free_camera: distance {distance}, size {width} x {height}, fovy {fovy}, near {near}, far {far}")
    az, el = np.deg2rad(float(azimuth)), np.deg2rad(float(elevation))
    f = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    r = np.cross(f, [0.0, 0.0, 1.0])
    if np.linalg.norm(r) < 1e-12:
        raise ValueError(f"free_camera: elevation {elevation} looks along the world's z axis, so 'up' is not defined")
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    eye = lookat - float(distance) * f
    view = np.zeros((4, 4))                      # rows: right, up, forward (camera coordinates), 1
    view[0, :3], view[1, :3], view[2, :3] = r, u, f
    view[:3, 3] = -view[:3, :3] @ eye
    view[3, 3] = 1.0
    fl = 0.5 * height / np.tan(0.5 * np.deg2rad(float(fovy)))       # focal length in pixels
    k = far / (far - near)
    proj = np.array([[fl, 0.0, 0.5 * width, 0.0],
                     [0.0, -fl, 0.5 * height, 0.0],
                     [0.0, 0.0, k, -k * near],
                     [0.0, 0.0, 1.0, 0.0]])
    return proj @ view, eye


def rigid(pos=(0.0, 0.0, 0.0), z_rot=0.0) -> np.ndarray:
    """Model matrix (4, 4) float64: a rotation by z_rot radians about z, then a translation by pos."""
    c, s = np.cos(float(z_rot)), np.sin(float(z_rot))
    m = np.eye(4)
    m[:2, :2] = [[c, -s], [s, c]]
    m[:3, 3] = np.asarray(pos, dtype=np.float64).reshape(3)
    return m


def draw_polyline(image: np.ndarray, points, colour) -> np.ndarray:
    """The closed polyline through integer points (K, 2) as (x, y), drawn into image (H, W, 3) in place (and returned): 8-connected
    Bresenham segments, thickness 1, pixels outside the image skipped.  Host numpy.  One point draws one pixel."""
    if not isinstance(image, np.ndarray) or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"draw_polyline: an (H, W, 3) array expected, got {getattr(image, 'shape', type(image))}")
    p = np.asarray(points)
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"draw_polyline: integer pixel coordinates expected, got {p.dtype}")
    p = p.reshape(-1, 2)
    if len(p) == 0:
        raise ValueError("draw_polyline: no points")
    H, W = image.shape[:2]
    col = np.asarray(colour, dtype=image.dtype).reshape(3)

    def plot(x, y):
        if 0 <= x < W and 0 <= y < H:
            image[y, x] = col
    for a, b in zip(p, np.roll(p, -1, axis=0)):
        x, y, x1, y1 = int(a[0]), int(a[1]), int(b[0]), int(b[1])
        dx, dy = abs(x1 - x), -abs(y1 - y)
        sx, sy = (1 if x < x1 else -1), (1 if y < y1 else -1)
        err = dx + dy
        while True:
            plot(x, y)
            if x == x1 and y == y1:
                break
            e2 = 2 * err
            if e2 >= dy:
                err += dy
                x += sx
            if e2 <= dx:
                err += dx
                y += sy
    return image


def write_png(path: str, image) -> str:
    """An (H, W, 3) uint8 image, RGB, as a PNG file; returns path."""
    from PIL import Image
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8), "RGB").save(path, format="PNG")
    return path


def _raise_rejected(rejected: torch.Tensor, fn: str) -> None:
    r = rejected.cpu().numpy()
    if r.any():
        v = int(np.flatnonzero(r)[0])
        raise ValueError(f"{fn}: view {v}: {int(r[v])} triangles have a vertex behind the camera or off the drawable range (there is no "
                         "near-plane clipping)")


def render_grippers(verts: torch.Tensor, faces) -> torch.Tensor:
    """engine.finger_mesh_2d / _3d output (B, 2 fingers, V, 3) float32 on the device and the faces (T, 3) both fingers share ->
    (B, 256, 256, 3) uint8 on the device: gripper b with its left and right jaw placed and coloured as assets/gripper_render.xml does,
    seen from the reference's camera.  One launch sequence for the whole batch."""
    v = verts.detach().to(dtype=torch.float32)
    if v.dim() != 4 or v.shape[1] != 2 or v.shape[3] != 3 or v.shape[0] < 1:
        raise ValueError(f"render_grippers: vertices of shape (B, 2, V, 3) expected, got {tuple(v.shape)}")
    B, _, V, _ = v.shape
    f = torch.as_tensor(faces).to(device=v.device, dtype=torch.int32).reshape(-1, 3)
    T = f.shape[0]
    offsets = (np.arange(2 * B + 1, dtype=np.int64) * V, np.arange(2 * B + 1, dtype=np.int64) * T)
    cam, eye = free_camera(width=GRIPPER_SIZE, height=GRIPPER_SIZE, **GRIPPER_CAMERA)
    models = [rigid(JAW_POS[k], np.deg2rad(JAW_ROT_Z_DEG[k])) for k in range(2)]
    n = 2 * B
    side = np.arange(n) % 2
    _, _, rgb, rejected = engine.render_meshes(
        v.reshape(-1, 3).contiguous(), f.repeat(n, 1).contiguous(), offsets, inst_view=np.arange(n) // 2, inst_mesh=np.arange(n),
        inst_matrix=np.stack([cam @ models[k] for k in side]), inst_id=np.asarray(JAW_IDS)[side], n_views=B, width=GRIPPER_SIZE, height=GRIPPER_SIZE,
        inst_rgb=np.asarray(JAW_RGB)[side], eyes=np.tile(eye, (B, 1)), inst_model=np.stack([models[k] for k in side]))
    _raise_rejected(rejected, "render_grippers")
    return rgb


def render_mesh(gripper_root: str) -> np.ndarray:
    """sim/render_mesh.py:render_mesh: the picture (256, 256, 3) uint8 of the gripper whose fingerl.obj and fingerr.obj lie in
    gripper_root (what save_grippers / prepare_gripper leave there), camera 0.9 / 180 / -30."""
    vl, fl = engine.read_obj(os.path.join(gripper_root, "fingerl.obj"))
    vr, fr = engine.read_obj(os.path.join(gripper_root, "fingerr.obj"))
    if vl.shape != vr.shape or not np.array_equal(fl, fr):
        raise ValueError(f"render_mesh: {gripper_root}: fingerl.obj and fingerr.obj do not share one face table")
    dev = torch.device("cuda", torch.cuda.current_device())
    v = torch.from_numpy(np.stack([vl, vr])[None].astype(np.float32)).to(dev)
    return render_grippers(v, fl)[0].cpu().numpy()


def object_views(verts, tris, z_rots, positions=None, rgb=OBJECT_RGB) -> torch.Tensor:
    """One object mesh (verts (V, 3), tris (T, 3)), one view per entry of z_rots: the object rotated by z_rots[k] radians about the
    world's z axis through the origin, then moved by positions[k] (n, 3) metres (nothing when None), seen from the reference's object camera
    (0.8 / 135 / -45) -> (n, 128, 128, 3) uint8 on the device, the object in `rgb` (flat-shaded; the default black stays black) on white."""
    z = np.asarray(z_rots, dtype=np.float64).reshape(-1)
    n = len(z)
    if n < 1:
        raise ValueError("object_silhouettes: need at least one rotation")
    pos = np.zeros((n, 3)) if positions is None else np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    if len(pos) != n:
        raise ValueError(f"object_silhouettes: {n} rotations and {len(pos)} positions")
    v = torch.as_tensor(verts).reshape(-1, 3)
    t = torch.as_tensor(tris).reshape(-1, 3)
    cam, eye = free_camera(width=OBJECT_SIZE, height=OBJECT_SIZE, **OBJECT_CAMERA)
    models = np.stack([rigid(pos[k], z[k]) for k in range(n)])
    offsets = (np.array([0, v.shape[0]], dtype=np.int64), np.array([0, t.shape[0]], dtype=np.int64))
    _, _, img, rejected = engine.render_meshes(v, t, offsets, inst_view=np.arange(n), inst_mesh=np.zeros(n, dtype=np.int32),
                                               inst_matrix=cam[None] @ models, inst_id=np.zeros(n, dtype=np.int32), n_views=n, width=OBJECT_SIZE,
                                               height=OBJECT_SIZE, inst_rgb=np.tile(np.asarray(rgb, dtype=np.float64), (n, 1)),
                                               eyes=np.tile(eye, (n, 1)), inst_model=models)
    _raise_rejected(rejected, "object_silhouettes")
    return img


def object_silhouettes(verts, tris, z_rots, positions=None) -> torch.Tensor:
    """The 100-point contours (n, 100, 2) int32, on the device, of the silhouettes of object_views(verts, tris, z_rots, positions):
    extract_contours(..., num_points=100, rescale=False) of every view in one batch; the images never leave the device.  A view in which
    the object is not seen raises ValueError naming it."""
    return engine.icon_contours(object_views(verts, tris, z_rots, positions), CONTOUR_POINTS, rescale=False)


def render_object_mesh(object_root: str, z_rots) -> List[np.ndarray]:
    """sim/render_mesh.py:render_object_mesh: model.obj of object_root at the origin, rotated by each of z_rots (radians) about z,
    rendered as a segmentation image (128 x 128, camera 0.8 / 135 / -45, object black on white) -> its contour (100, 2) int32 per
    rotation."""
    v, t = engine.read_obj(os.path.join(object_root, "model.obj"))
    return list(object_silhouettes(v, t, z_rots).cpu().numpy())
