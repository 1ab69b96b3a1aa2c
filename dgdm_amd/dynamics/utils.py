"""Object point clouds from scanned meshes (reference: dynamics/utils.py:14-18, ``sample_pts_from_mesh``, open3d's
``read_triangle_mesh`` + ``sample_points_uniformly``).  The OBJ files are parsed on the host by the library's reader and sampled on the
device (csrc/mesh.hip) under the contract of DESIGN.md "Object clouds from meshes": the same object name gives the same cloud in
guided sampling, in dynamics training and on every rank, whatever else is in the batch."""
from __future__ import annotations

import os
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Sequence

import numpy as np

from .. import engine

MESH_FILE = "model.obj"
SEED = 0


def mesh_key(name: str) -> int:
    """The Philox key of an object: crc32 of its name (the directory that holds its model.obj)."""
    return zlib.crc32(name.encode("utf-8"))


def sample_meshes(files: Sequence[str], keys: Sequence[int], num_points: int) -> np.ndarray:
    """(len(files), num_points, 3) float64: every OBJ parsed on a few host threads (the reader releases the GIL), one device call."""
    with ThreadPoolExecutor(max_workers=min(8, len(files))) as ex:
        meshes = list(ex.map(engine.read_obj, files))
    verts, tris, offsets = engine.concat_meshes(meshes)
    return engine.sample_mesh_points(verts, tris, offsets, np.asarray(keys, dtype=np.uint64), num_points, SEED).cpu().numpy()


def sample_pts_from_mesh(mesh_file: str, num_points: int = 1024) -> np.ndarray:
    """(num_points, 3) float64 surface points of one OBJ, keyed by the name of the directory that holds it (dynamics/utils.py:14-18)."""
    name = os.path.basename(os.path.dirname(os.path.abspath(mesh_file)))
    return sample_meshes([mesh_file], [mesh_key(name)], num_points)[0]


def sample_object_clouds(object_dir: str, names: Sequence[str], num_points: int) -> np.ndarray:
    """(len(names), num_points, 3) float64: ``<object_dir>/<name>/model.obj`` for each name, in one batched device call."""
    files = [os.path.join(object_dir, n, MESH_FILE) for n in names]
    return sample_meshes(files, [mesh_key(n) for n in names], num_points)
