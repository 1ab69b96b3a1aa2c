"""Object contours from icon images (reference: assets/icon_process.py) without cv2: the reference's extract_contours and
resample_contour under their own signatures, computed on the GPU (csrc/contour.hip) under the contract of DESIGN.md §4.5b.
draw_contour and the mesh export (generate_icon_mesh / save_icon_mesh: trimesh, triangle) stay with the simulator setup."""
from __future__ import annotations

import numpy as np
import torch

from .. import engine


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
