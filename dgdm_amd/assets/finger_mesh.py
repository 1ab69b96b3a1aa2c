"""Designed fingers as files a mesh viewer, a printer or a simulator opens: watertight OBJ meshes, convex collision pieces and the
MuJoCo gripper file - where the reference goes through trimesh, geomdl's exporter and an external V-HACD run per finger
(assets/finger_sampler.py:7-64, assets/finger_3d.py:38-80, dynamics/sim_test_mj.py:57-104, sim_test_mj_3d.py:47-92).

Vertices, statistics and pieces are computed on the device for a whole batch (csrc/finger_mesh.hip); files are written by host threads."""
from __future__ import annotations

import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import engine
from . import gripper_xml

AREA_EPS = 1e-12           # m^2: a triangle below this (micrometre-sized edges) is degenerate for printing and for a simulator's hulls
PIECES_2D, PIECES_3D = 16, (8, 2)      # the reference's V-HACD hull caps: -h 16 (2-D), -h 32 = 2 * 8 * 2 (3-D)
_closed = {}


def is_closed(faces: np.ndarray) -> bool:
    """Every directed edge occurs exactly once and its reverse exactly once: closed, manifold and consistently oriented."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = e[:, 0] * (int(f.max()) + 1) + e[:, 1]
    rev = e[:, 1] * (int(f.max()) + 1) + e[:, 0]
    return len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(rev))


class FingerMesh:
    """The subset of trimesh.Trimesh the reference touches - ``vertices``, ``faces``, ``export(path)`` - plus ``volume``, ``area`` and
    ``is_watertight``.  Volume and area are the device statistics of the float32 vertices (csrc/finger_mesh.hip)."""

    def __init__(self, vertices32: np.ndarray, faces: np.ndarray, stats: Sequence[float]):
        self._v32 = np.ascontiguousarray(vertices32, dtype=np.float32)
        self.vertices = self._v32.astype(np.float64)
        self.faces = np.asarray(faces, dtype=np.int32)
        self.volume, self.area, self.min_triangle_area = float(stats[0]), float(stats[1]), float(stats[2])

    @property
    def is_watertight(self) -> bool:
        key = self.faces.tobytes()
        if key not in _closed:
            _closed[key] = is_closed(self.faces)
        return _closed[key] and self.volume > 0.0

    def export(self, path: str) -> None:
        engine.write_obj(path, self._v32, self.faces)


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def finger_meshes(y, mode: str, n: int, width: float, height: float = 0.02) -> Tuple[FingerMesh, FingerMesh]:
    """Both fingers of one gripper from control values already in metres (left finger's first)."""
    s = torch.from_numpy(np.asarray(y, dtype=np.float32).reshape(1, -1)).to(_device())
    if mode == 'point_3d':
        v, kind = engine.finger_mesh_3d(s, int(n), width=width, scale=1.0, offset=0.0), engine.MESH_3D
    else:
        v, kind = engine.finger_mesh_2d(s, int(n), width=width, height=height, scale=1.0, offset=0.0), engine.MESH_2D
    faces = engine.finger_mesh_faces(kind, int(n))
    st = engine.finger_mesh_stats(v, faces, AREA_EPS).cpu().numpy()
    v = v.cpu().numpy()
    return FingerMesh(v[0, 0], faces, st[0, 0]), FingerMesh(v[0, 1], faces, st[0, 1])


def save_grippers(samples: torch.Tensor, model_root: str, first_idx: int = 0, mode: Optional[str] = None, pieces=None, num_points: int = 200,
                  sample_size: int = 25, width: Optional[float] = None, height: float = 0.02, area_eps: float = AREA_EPS) -> List[str]:
    """A sampler batch (B, L, 1) in [-1, 1] -> for gripper b, index idx = first_idx + b:
        <model_root>/grippers/<idx>/fingerl.obj, fingerr.obj         the watertight finger meshes
        <model_root>/grippers/<idx>/fingerlNNN.obj, fingerrNNN.obj   the convex collision pieces
        <model_root>/grippers/<idx>/mesh.json                        volume, area, piece count and chord_err of each finger
        <model_root>/gripper_<idx>.xml                               the MuJoCo gripper file naming them (where prepare_finger puts it)
    what prepare_finger / prepare_gripper leave behind (dynamics/sim_test_mj.py:85-104, sim_test_mj_3d.py:75-92).  mode 'point' (2-D,
    pieces = an int, default 16) or 'point_3d' (pieces = (pu, pv), default (8, 2)); by default decided from L == 42.  Vertices,
    statistics and pieces are one launch each for the batch; the files are written by at most 16 host threads.  A gripper whose
    directory exists is left alone, as the reference does.  A finger with a triangle below area_eps, or without positive volume,
    raises ValueError naming the gripper index before anything is written.  Returns the B gripper directories."""
    B, L = samples.shape[0], int(np.prod(samples.shape[1:]))
    mode = mode or ('point_3d' if L == 42 else 'point')
    if mode == 'point_3d':
        pu, pv = PIECES_3D if pieces is None else pieces
        n, kind, pkind = int(sample_size), engine.MESH_3D, engine.PIECE_3D
        verts = engine.finger_mesh_3d(samples, n, width=0.1 if width is None else width)
        pc, chord = engine.finger_pieces_3d(verts, pu, pv)
        write_xml = gripper_xml.generate_gripper_3d_xml
    elif mode == 'point':
        n, kind, pkind = int(num_points), engine.MESH_2D, engine.PIECE_2D
        verts = engine.finger_mesh_2d(samples, n, width=0.03 if width is None else width, height=height)
        pc, chord = engine.finger_pieces_2d(verts, PIECES_2D if pieces is None else int(pieces))
        write_xml = gripper_xml.generate_xml
    else:
        raise ValueError('model type not supported')
    faces, pfaces = engine.finger_mesh_faces(kind, n), engine.finger_mesh_faces(pkind)
    stats = engine.finger_mesh_stats(verts, faces, area_eps).cpu().numpy()
    verts, pc, chord = verts.cpu().numpy(), pc.cpu().numpy(), chord.cpu().numpy()
    for b in range(B):
        for f, side in enumerate("lr"):
            vol, _, amin, small = stats[b, f]
            if not (small == 0 and vol > 0):
                raise ValueError(f"gripper {first_idx + b}: finger{side} is degenerate ({int(small) if small == small else 'nan'} triangles below "
                                 f"{area_eps} m^2, smallest {amin}, volume {vol}); nothing was written")
    dirs = [os.path.join(model_root, 'grippers', str(first_idx + b)) for b in range(B)]

    def write(b):
        idx, d = first_idx + b, dirs[b]
        if os.path.exists(d):
            return
        os.makedirs(d)
        info = {"mode": mode, "vertices": int(faces.max()) + 1, "triangles": len(faces)}
        for f, side in enumerate("lr"):
            engine.write_obj(os.path.join(d, f"finger{side}.obj"), verts[b, f], faces)
            for k in range(pc.shape[2]):
                engine.write_obj(os.path.join(d, f"finger{side}{k:03d}.obj"), pc[b, f, k], pfaces)
            info[f"finger{side}"] = {"volume": float(stats[b, f, 0]), "area": float(stats[b, f, 1]), "min_triangle_area": float(stats[b, f, 2]),
                                     "pieces": int(pc.shape[2]), "chord_err": float(chord[b, f])}
        with open(os.path.join(d, "mesh.json"), "w") as fh:
            json.dump(info, fh, indent=1)
        write_xml(pc.shape[2], pc.shape[2], idx, os.path.join(model_root, 'gripper_%d.xml' % idx))

    if B:
        os.makedirs(model_root, exist_ok=True)
        with ThreadPoolExecutor(max_workers=min(16, B)) as ex:
            list(ex.map(write, range(B)))
    return dirs
