"""Object contours from icon images (reference: assets/icon_process.py) without cv2: the reference's extract_contours and
resample_contour under their own signatures, computed on the GPU (csrc/contour.hip) under the contract of DESIGN.md §4.5b; and the
icon as a simulator object without triangle, trimesh or V-HACD: generate_icon_mesh / save_icon_mesh under their own signatures and the
batched save_icon_objects, on the exact-integer triangulation and convex pieces of csrc/polygon.hip.
draw_contour needs cv2's rasteriser and stays with the simulator setup."""
from __future__ import annotations

import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import engine
from .finger_mesh import FingerMesh
from .object_sampler import generate_object_xml


def _points_dtype_check(a: np.ndarray, fn: str) -> None:
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{fn}: integer pixel coordinates expected (cv2 contours are int32), got {a.dtype}")


def _host_images(images, fn: str, rank: int):
    """numpy or torch uint8 images; anything else raises before a launch."""
    a = images if isinstance(images, torch.Tensor) else np.asarray(images)
    if a.dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"{fn}: uint8 images expected, got {a.dtype}")
    if a.ndim != rank or a.shape[-1] not in (3, 4):
        shape = "(H, W, 3|4)" if rank == 3 else "(M, H, W, 3|4)"
        raise ValueError(f"{fn}: an image of shape {shape} expected (channel 0 blue, as cv2 reads it), got {tuple(a.shape)}")
    return a


def resample_contour(contour, num_points):
    """(K, ..., 2) integer points -> (num_points, 1, 2) int32, evenly spaced by arc length along the open polyline."""
    c = np.asarray(contour).reshape(-1, 2)
    _points_dtype_check(c, "resample_contour")
    if len(c) == 0:
        raise ValueError("resample_contour: empty contour")
    out = engine.resample_contours(c, [0, len(c)], int(num_points))
    return out[0].cpu().numpy().reshape(-1, 1, 2)


def extract_contours_batch(images, num_points=100, rescale=True):
    """extract_contours of every image of an (M, H, W, 3|4) uint8 stack in one device call: (M, num_points, 2), float64 in
    [-0.05, 0.05] when rescale, else int32 pixel coordinates on the 128 x 128 grid.  An image without foreground raises ValueError
    naming its index."""
    a = _host_images(images, "extract_contours_batch", 4)
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return engine.icon_contours(a, int(num_points), bool(rescale)).cpu().numpy()


def extract_contours(image, num_points=100, rescale=True):
    """The longest external contour of one (H, W, 3|4) uint8 image resized to 128 x 128, resampled to num_points: (num_points, 2),
    float64 in [-0.05, 0.05] when rescale, else int32."""
    a = _host_images(image, "extract_contours", 3)
    return extract_contours_batch(a[None], num_points, rescale)[0]


# ------------------------------------------------------------------------------------------------------------------ icon meshes
def _rescale(points: np.ndarray) -> np.ndarray:
    """extract_contours' own statement on integer points: the float64 values extract_contours(rescale=True) returns, bit for bit."""
    return points / 128 * 0.1 - 0.05


def _extrude(xy32: np.ndarray, height: float) -> np.ndarray:
    """(k, 2) float32 -> (2 k, 3) float32: the ring at z = 0, then the ring at z = height."""
    k = len(xy32)
    v = np.zeros((2 * k, 3), dtype=np.float32)
    v[:k, :2] = v[k:, :2] = xy32
    v[k:, 2] = np.float32(height)
    return v


def _prism_faces(order: np.ndarray, cap: np.ndarray, k: int) -> np.ndarray:
    """Faces of the prism over vertices 0 .. k - 1 (z = 0) and k .. 2 k - 1 (z = height), counter-clockwise seen from outside
    (DESIGN.md §4.5c): per edge a -> b of the counter-clockwise `order` the side triangles (a, b, b + k), (a, b + k, a + k); then the cap
    triangles at z = height; then the same triangles at z = 0 with reversed winding."""
    a, b = order, np.roll(order, -1)
    sides = np.stack([np.stack([a, b, b + k], -1), np.stack([a, b + k, a + k], -1)], 1).reshape(-1, 3)
    return np.concatenate([sides, cap + k, cap[:, ::-1]]).astype(np.int32)


def signed_volume(verts: np.ndarray, faces: np.ndarray) -> float:
    """sum_t v0 . (v1 x v2) / 6 in float64."""
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def icon_prisms(points: np.ndarray, ring: np.ndarray, area2: int, triangles: np.ndarray, pieces: Sequence[Tuple[int, ...]], height: float):
    """One valid ring of engine.polygon_decompose -> ((vertices (2 M, 3) float32, faces (4 M - 4, 3) int32), [the same per piece]).
    points (n, 2) integers, ring the M original indices kept, triangles (M - 2, 3) and pieces in original indices.  Vertex k of the
    mesh is kept point k: float32 of its rescaled float64 coordinates.  A piece's prism stands on the piece's corners - a vertex at
    which the piece goes straight (cross == 0, in integers) is left out, so that float32 rounding cannot dent the hull."""
    M = len(ring)
    where = np.full(len(points), -1, dtype=np.int64)
    where[ring] = np.arange(M)
    xy32 = _rescale(np.asarray(points)[ring]).astype(np.float32)
    order = np.arange(M) if area2 > 0 else np.arange(M)[::-1]
    mesh = (_extrude(xy32, height), _prism_faces(order, where[np.asarray(triangles, dtype=np.int64)], M))
    out = []
    for piece in pieces:
        q = np.asarray(points, dtype=np.int64)[list(piece)]
        u, w = q - np.roll(q, 1, axis=0), np.roll(q, -1, axis=0) - q
        corner = where[np.asarray(piece)[u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0] != 0]]
        k = len(corner)
        fan = np.stack([np.zeros(k - 2, dtype=np.int64), np.arange(1, k - 1), np.arange(2, k)], -1)
        out.append((_extrude(xy32[corner], height), _prism_faces(np.arange(k), fan, k)))
    return mesh, out


def _decompose(images, num_points: int):
    """One device pass over an (B, H, W, 3|4) uint8 stack: (integer contours (B, n, 2), per-ring host results)."""
    a = _host_images(images, "save_icon_objects", 4)
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    pts = engine.icon_contours(a, int(num_points), rescale=False)
    dec = engine.polygon_decompose(pts)
    pieces = engine.canonical_pieces(dec["piece_count"], dec["piece_offsets"], dec["piece_index"])
    host = {k: dec[k].cpu().numpy() for k in ("status", "count", "ring", "area2", "triangles")}
    return pts.cpu().numpy(), host, pieces


def _ring_of(host, b):
    M = int(host["count"][b])
    return host["ring"][b, :M], int(host["area2"][b]), host["triangles"][b, :max(M - 2, 0)]


def generate_icon_mesh(img, height, num_points=100):
    """(mesh, contour) of one (H, W, 3|4) uint8 icon: contour is extract_contours(img, num_points); mesh the prism of height `height`
    over its M cleaned points - 2 M side triangles, the cap at z = height, the cap at z = 0 - with `vertices`, `faces`, `is_watertight`
    and `export(path)`.  An icon whose contour is refused (fewer than three points, no area, not simple) raises
    ValueError naming the status."""
    a = _host_images(img, "generate_icon_mesh", 3)
    pts, host, pieces = _decompose(a[None], num_points)
    if host["status"][0] != 0:
        raise ValueError(f"generate_icon_mesh: the contour cannot be meshed (status {int(host['status'][0])})")
    ring, a2, tris = _ring_of(host, 0)
    (v, f), _ = icon_prisms(pts[0], ring, a2, tris, [], float(height))
    dev = torch.device("cuda", torch.cuda.current_device())
    stats = engine.finger_mesh_stats(torch.from_numpy(v).to(dev), f).cpu().numpy()
    return FingerMesh(v, f, stats), _rescale(pts[0])


def save_icon_mesh(img, height, num_points, save_dir):
    """generate_icon_mesh, exported as <save_dir>/object.obj: (contour, mesh_path)."""
    os.makedirs(save_dir, exist_ok=True)
    mesh, contour = generate_icon_mesh(img, height, num_points)
    mesh_path = os.path.join(save_dir, 'object.obj')
    mesh.export(mesh_path)
    return contour, mesh_path


def save_icon_objects(images, model_root, object_ids, height=0.02, num_points=100, skip_invalid=False) -> List[int]:
    """What prepare_icon_object leaves behind (sim/sim_2d.py:103-111) for a whole stack of icons, (B, H, W, 3|4) uint8, object b under
    the index object_ids[b]:
        <model_root>/objects/<idx>/object.obj         the watertight prism over the icon's contour
        <model_root>/objects/<idx>/objectNNN.obj      one prism per convex piece (a k-gon: 2 k vertices, 4 k - 4 triangles)
        <model_root>/objects/<idx>/mesh.json          M, area2, the volume, the piece count
        <model_root>/object_<idx>.xml                 the MuJoCo object file naming them
    Contours, triangulation and pieces are one device pass for the batch; the files are written by at most 16 host threads.  An object
    whose directory exists is left alone, as the reference does.  A refused contour raises ValueError naming the object id and the
    status before anything is written; with skip_invalid the others are written.  Returns the refused ids."""
    ids = [int(i) for i in object_ids]
    pts, host, pieces = _decompose(images, num_points)
    if len(ids) != len(pts):
        raise ValueError(f"save_icon_objects: {len(pts)} images and {len(ids)} object ids")
    refused = [b for b in range(len(ids)) if host["status"][b] != 0]
    if refused and not skip_invalid:
        raise ValueError("save_icon_objects: " + ", ".join(f"object {ids[b]} cannot be meshed (status {int(host['status'][b])})" for b in refused)
                         + "; nothing was written")

    def write(b):
        idx, d = ids[b], os.path.join(model_root, 'objects', str(ids[b]))
        if os.path.exists(d):
            return
        ring, a2, tris = _ring_of(host, b)
        (v, f), prisms = icon_prisms(pts[b], ring, a2, tris, pieces[b], float(height))
        os.makedirs(d)
        engine.write_obj(os.path.join(d, "object.obj"), v, f)
        for k, (pv, pf) in enumerate(prisms):
            engine.write_obj(os.path.join(d, f"object{k:03d}.obj"), pv, pf)
        with open(os.path.join(d, "mesh.json"), "w") as fh:
            json.dump({"M": len(ring), "area2": a2, "volume": signed_volume(v, f), "pieces": len(prisms), "height": float(height)}, fh, indent=1)
        generate_object_xml(len(prisms), idx, os.path.join(model_root, 'object_%d.xml' % idx))

    todo = [b for b in range(len(ids)) if host["status"][b] == 0]
    if todo:
        os.makedirs(model_root, exist_ok=True)
        with ThreadPoolExecutor(max_workers=min(16, len(todo))) as ex:
            list(ex.map(write, todo))
    return [ids[b] for b in refused]
