"""3-D finger surfaces from control points (reference: assets/finger_3d.py:60-98), on the MI355X.

``generate_3d_ctrlpts`` / ``generate_3d_finger_vertices`` / ``generate_3d_gripper`` keep the reference's names and return
values; ``generate_3d_grippers`` is the batched form for the sampler's output (dynamics/sim_test_mj_3d.py:233-237).
``generate_3d_finger_mesh`` / ``save_3d_gripper`` and the XML writers keep the reference's names too; ``save_grippers`` (finger_mesh.py)
is the batched exporter."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import engine
from .finger_mesh import FingerMesh, finger_meshes, save_grippers  # noqa: F401
from .gripper_xml import create_geom_elements, create_mesh_elements, generate_gripper_3d_xml, generate_scene_3d_xml  # noqa: F401


def _net():
    # x = linspace(-0.12, 0.12, 7), z = linspace(0, 0.12, 3), control point (i, j) -> index 3 i + j  (finger_3d.py:77-80)
    x = np.linspace(-0.12, 0.12, 7)
    z = np.linspace(0, 0.12, 3)
    x_n, z_n = np.meshgrid(x, z)
    return x_n.T.reshape(-1), z_n.T.reshape(-1)


def generate_3d_ctrlpts(yl, yr):
    xs, zs = _net()
    return np.concatenate((np.stack([xs, np.asarray(yl, dtype=np.float64), zs], -1),
                           np.stack([xs, np.asarray(yr, dtype=np.float64), zs], -1)), axis=0)


def generate_3d_grippers(samples: torch.Tensor, sample_size: int = 25) -> torch.Tensor:
    """Sampler output (B, 42, 1) in [-1, 1] -> (B, 2, sample_size^2, 3): both finger surfaces in metres."""
    return engine.finger_decode_3d(samples, sample_size)


def generate_3d_finger_vertices(control_points, degree_u=3, degree_v=2, sample_size=25):
    """One finger: (21, 3) control points on the reference's net -> (sample_size^2, 3) surface points."""
    if (degree_u, degree_v) != (3, 2):
        raise NotImplementedError("the device decode is built for the reference's degrees (3, 2)")
    cp = np.asarray(control_points, dtype=np.float64).reshape(21, 3)
    xs, zs = _net()
    if not (np.allclose(cp[:, 0], xs, rtol=0, atol=1e-9) and np.allclose(cp[:, 2], zs, rtol=0, atol=1e-9)):
        raise NotImplementedError("device decode supports the reference's 7 x 3 control net (finger_3d.py:77-80)")
    y = np.concatenate([cp[:, 1], cp[:, 1]]).astype(np.float32)
    dev = torch.device("cuda", torch.cuda.current_device())
    return engine.finger_decode_3d(torch.from_numpy(y).reshape(1, -1).to(dev), int(sample_size), scale=1.0, offset=0.0)[0, 0].cpu().numpy().astype(np.float64)


def generate_3d_gripper(yl, yr, sample_size=25):
    """Returns (ctrlpts (42, 3), vertices (2 sample_size^2, 3)) like the reference."""
    y = np.concatenate([np.asarray(yl, dtype=np.float32), np.asarray(yr, dtype=np.float32)])
    dev = torch.device("cuda", torch.cuda.current_device())
    v = engine.finger_decode_3d(torch.from_numpy(y).reshape(1, -1).to(dev), int(sample_size), scale=1.0, offset=0.0)[0].cpu().numpy()
    return generate_3d_ctrlpts(yl, yr), np.concatenate([v[0], v[1]], 0).astype(np.float64)


def _control_y(control_points, degree_u, degree_v) -> np.ndarray:
    if (degree_u, degree_v) != (3, 2):
        raise NotImplementedError("the device decode is built for the reference's degrees (3, 2)")
    cp = np.asarray(control_points, dtype=np.float64).reshape(21, 3)
    xs, zs = _net()
    if not (np.allclose(cp[:, 0], xs, rtol=0, atol=1e-9) and np.allclose(cp[:, 2], zs, rtol=0, atol=1e-9)):
        raise NotImplementedError("device decode supports the reference's 7 x 3 control net (finger_3d.py:77-80)")
    return cp[:, 1]


def generate_3d_finger_mesh(control_points, degree_u=3, degree_v=2, sample_size=25, width=0.12):
    """Returns (mesh, surf_vertices (sample_size^2, 3)) like the reference (assets/finger_3d.py:38-57): the surface and its copy shifted
    by ``width`` in y, closed by side walls, as a watertight ``FingerMesh``.  The triangulation is this project's."""
    y = _control_y(control_points, degree_u, degree_v)
    mesh, _ = finger_meshes(np.concatenate([y, y]), 'point_3d', sample_size, width)
    return mesh, mesh.vertices[:sample_size * sample_size].copy()


def save_3d_gripper(yl, yr, width=0.12, sample_size=25, save_gripper_dir=''):
    """Writes fingerl.obj / fingerr.obj into ``save_gripper_dir`` and returns (ctrlpts (42, 3), surface vertices (2 sample_size^2, 3))
    like the reference (assets/finger_3d.py:69-80)."""
    y = np.concatenate([np.asarray(yl, dtype=np.float32), np.asarray(yr, dtype=np.float32)])
    mesh_l, mesh_r = finger_meshes(y, 'point_3d', sample_size, width)
    os.makedirs(save_gripper_dir, exist_ok=True)
    mesh_l.export(os.path.join(save_gripper_dir, 'fingerl.obj'))
    mesh_r.export(os.path.join(save_gripper_dir, 'fingerr.obj'))
    N = sample_size * sample_size
    return generate_3d_ctrlpts(yl, yr), np.concatenate([mesh_l.vertices[:N], mesh_r.vertices[:N]], 0)
