"""The MuJoCo model file of one object (reference: assets/object_sampler.py, assets/scan_object_process.py): ``object_<idx>.xml``, the
body with a free joint, its visual mesh and its convex collision pieces, which the scene file of gripper_xml.py includes by name.

Written from the files the reference's writers produce (recorded under tests/golden/object_xml/ by
tests/golden/make_golden_object_xml.py; tests/test_object_xml_host.py compares element by element), as a table of
(tag, attributes, children) like gripper_xml.py."""
from __future__ import annotations

import xml.etree.ElementTree as ET

from .gripper_xml import _build


def _object(num_collision, object_idx, save_path, visual_file, piece_file):
    names = [f"object{i:03d}" for i in range(num_collision)]
    root = ("mujoco", {"model": "object"}, [
        ("asset", {}, [("mesh", {"name": "object", "file": visual_file % object_idx}, [])]
         + [("mesh", {"name": n, "file": piece_file(object_idx, i)}, []) for i, n in enumerate(names)]),
        ("worldbody", {}, [("body", {"name": "object"}, [
            ("freejoint", {"name": "object_root"}, []),
            ("geom", {"mesh": "object", "type": "mesh", "class": "visual"}, [])]
            + [("geom", {"mesh": n, "type": "mesh", "class": "collision"}, []) for n in names])]),
    ])
    ET.ElementTree(_build(root)).write(save_path)


def generate_object_xml(num_collision, object_idx, save_path):
    """The 2-D (icon) object: objects/<idx>/object.obj and its pieces objects/<idx>/object000.obj ..."""
    _object(num_collision, object_idx, save_path, "objects/%d/object.obj", lambda idx, i: f"objects/{idx}/object{i:03d}.obj")
