"""2-D finger curves and extruded finger meshes from control points (reference: assets/finger_sampler.py), on the MI355X.

``generate_gripper`` keeps the reference's name, arguments and return values for one gripper; ``generate_grippers`` is the
batched form the sampler's output goes through (dynamics/sim_test_mj.py:254-262 does the same per gripper on the host).
``generate_finger_shape`` / ``save_gripper`` and the XML writers keep the reference's names too; ``save_grippers`` (finger_mesh.py) is the
batched exporter."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import engine
from .finger_mesh import FingerMesh, finger_meshes, save_grippers  # noqa: F401
from .gripper_xml import create_geom_elements, create_mesh_elements, generate_scene_xml, generate_xml, generate_xml_optimized  # noqa: F401


def generate_grippers(samples: torch.Tensor, num_points: int = 200) -> torch.Tensor:
    """Sampler output (B, L, 1) in [-1, 1] -> (B, 2, num_points, 2): the left and right finger curves in metres."""
    return engine.finger_decode_2d(samples, num_points)


def generate_gripper(finger_x, finger_yl, finger_yr, num_points):
    """Returns (ctrlpts (2K, 2), allpts (2 num_points, 2)) like the reference.  ``finger_x`` must be the abscissae the reference
    always passes, ``np.linspace(-0.12, 0.12, K)`` (sim_test_mj.py:257): the device decode has that grid built in."""
    finger_x = np.asarray(finger_x, dtype=np.float64)
    K = finger_x.shape[0]
    if not np.allclose(finger_x, np.linspace(-0.12, 0.12, K), rtol=0, atol=1e-9):
        raise NotImplementedError("device decode supports finger_x = linspace(-0.12, 0.12, K) (the reference's only call site)")
    y = np.concatenate([np.asarray(finger_yl, dtype=np.float32), np.asarray(finger_yr, dtype=np.float32)])
    dev = torch.device("cuda", torch.cuda.current_device())
    pts = engine.finger_decode_2d(torch.from_numpy(y).reshape(1, -1).to(dev), int(num_points), scale=1.0, offset=0.0)[0].cpu().numpy()
    ctrl = np.concatenate([np.stack([finger_x, np.asarray(finger_yl, dtype=np.float64)], -1),
                           np.stack([finger_x, np.asarray(finger_yr, dtype=np.float64)], -1)], 0)
    return ctrl, np.concatenate([pts[0], pts[1]], 0).astype(np.float64)


def _check_x(finger_x) -> np.ndarray:
    finger_x = np.asarray(finger_x, dtype=np.float64)
    if not np.allclose(finger_x, np.linspace(-0.12, 0.12, finger_x.shape[0]), rtol=0, atol=1e-9):
        raise NotImplementedError("device decode supports finger_x = linspace(-0.12, 0.12, K) (the reference's only call site)")
    return finger_x


def generate_finger_shape(x, y, width, height, num_points=100):
    """Returns (mesh, x_new, y_new) like the reference (assets/finger_sampler.py:7-36): the curve through (x, y) extruded by
    ``width`` in y and ``height`` in z as a watertight ``FingerMesh``.  ``x`` is restricted as in ``generate_gripper``."""
    _check_x(x)
    y = np.asarray(y, dtype=np.float32)
    mesh, _ = finger_meshes(np.concatenate([y, y]), 'point', num_points, width, height)
    return mesh, mesh.vertices[:num_points, 0].copy(), mesh.vertices[:num_points, 1].copy()


def save_gripper(finger_x, finger_yl, finger_yr, width, height, num_points, save_gripper_dir):
    """Writes fingerl.obj / fingerr.obj into ``save_gripper_dir`` and returns (ctrlpts (2K, 2), allpts (2 num_points, 2)) like the
    reference (assets/finger_sampler.py:52-64).  ``finger_x`` is restricted as in ``generate_gripper``."""
    finger_x = _check_x(finger_x)
    os.makedirs(save_gripper_dir, exist_ok=True)
    y = np.concatenate([np.asarray(finger_yl, dtype=np.float32), np.asarray(finger_yr, dtype=np.float32)])
    meshl, meshr = finger_meshes(y, 'point', num_points, width, height)
    meshl.export(os.path.join(save_gripper_dir, 'fingerl.obj'))
    meshr.export(os.path.join(save_gripper_dir, 'fingerr.obj'))
    ctrl = np.concatenate([np.stack([finger_x, np.asarray(finger_yl, dtype=np.float64)], -1),
                           np.stack([finger_x, np.asarray(finger_yr, dtype=np.float64)], -1)], 0)
    return ctrl, np.concatenate([meshl.vertices[:num_points, :2], meshr.vertices[:num_points, :2]], 0)
