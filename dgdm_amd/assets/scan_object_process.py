"""The scanned 3-D objects' side of the model root (reference: assets/scan_object_process.py): the object file over
objects/<idx>/model.obj and its model_collision_<i>.obj pieces, and the lists of object names.  The bounding-box helpers (get_bbox,
filter_object) need open3d and are not carried."""
from __future__ import annotations

import os

from .object_sampler import _object


def read_object_names(test=False, root='assets'):
    """The names listed one per line in <root>/object_names_test.txt (test) or <root>/object_names.txt; the reference reads them from
    'assets' under the working directory."""
    filename = os.path.join(root, 'object_names_test.txt' if test else 'object_names.txt')
    with open(filename, 'r') as f:
        return [line.strip() for line in f.readlines()]


def generate_object_3d_xml(num_collision, object_idx, save_path):
    _object(num_collision, object_idx, save_path, "objects/%d/model.obj", lambda idx, i: f"objects/{idx}/model_collision_{i}.obj")
