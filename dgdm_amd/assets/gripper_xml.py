"""The MuJoCo model files that go with an exported gripper: ``gripper_<idx>.xml`` (the two finger bodies, their visual mesh and
collision pieces, one slide joint and one position actuator each) and the scene file that includes it next to an object.

Written from the files the reference's writers produce (recorded under tests/golden/gripper_xml/ by
tests/golden/make_golden_gripper_xml.py; tests/test_finger_mesh_host.py compares element by element), as tables of
(tag, attributes, children) rather than call by call."""
from __future__ import annotations

import xml.etree.ElementTree as ET

# what differs between the 2-D and the 3-D gripper file: the model name, how far apart the jaws start, the colour of the visual geoms
_GRIPPER = {
    "gripper_2d": {"jaw_y": "0.15", "rgba": (None, None)},
    "gripper_3d": {"jaw_y": "0.23", "rgba": ("0.9333 0.7804 0.3490 1", "0.6941 0.7647 0.5059 1")},
}


def _build(node) -> ET.Element:
    tag, attrib, children = node
    e = ET.Element(tag, dict(attrib))
    for c in children:
        e.append(c if isinstance(c, ET.Element) else _build(c))
    return e


def create_mesh_elements(num_meshes, mesh_prefix, gripper_idx):
    """<mesh name="fingerl003" file="grippers/<idx>/fingerl003.obj"/> for piece 0 .. num_meshes - 1."""
    return [ET.Element("mesh", {"name": f"{mesh_prefix}{i:03d}", "file": f"grippers/{gripper_idx}/{mesh_prefix}{i:03d}.obj"})
            for i in range(num_meshes)]


def create_geom_elements(num_meshes, mesh_prefix):
    """<geom mesh="fingerl003" type="mesh" class="collision"/> for piece 0 .. num_meshes - 1."""
    return [ET.Element("geom", {"mesh": f"{mesh_prefix}{i:03d}", "type": "mesh", "class": "collision"}) for i in range(num_meshes)]


def _jaw(side, name, num_pieces, pos, rgba):
    visual = {"mesh": name, "type": "mesh", "class": "visual"}
    if rgba:
        visual["rgba"] = rgba
    return ("body", {"name": f"{side}_jaw", "pos": pos},
            [("joint", {"name": f"{side}_grip"}, []), ("geom", visual, [])] + create_geom_elements(num_pieces, name))


def _gripper(model, num_left, num_right, gripper_idx, save_path):
    cfg = _GRIPPER[model]
    visual = [ET.Element("mesh", {"name": n, "file": f"grippers/{gripper_idx}/{n}.obj"}) for n in ("fingerl", "fingerr")]
    root = ("mujoco", {"model": model}, [
        ("asset", {}, visual + create_mesh_elements(num_left, "fingerl", gripper_idx) + create_mesh_elements(num_right, "fingerr", gripper_idx)),
        ("default", {}, [("joint", {"type": "slide", "axis": "0 1 0", "damping": "1"}, [])]),
        ("worldbody", {}, [("body", {"name": "fingers", "pos": "0 0 0"}, [
            _jaw("left", "fingerl", num_left, f"0 -{cfg['jaw_y']} 0", cfg["rgba"][0]),
            _jaw("right", "fingerr", num_right, f"0 {cfg['jaw_y']} 0", cfg["rgba"][1])])]),
        ("actuator", {}, [("position", {"name": "left", "joint": "left_grip", "ctrlrange": "0 0.1", "kp": "10"}, []),
                          ("position", {"name": "right", "joint": "right_grip", "ctrlrange": "-0.1 0", "kp": "10"}, [])]),
    ])
    ET.ElementTree(_build(root)).write(save_path)


def generate_xml(left_num_collision_meshes, right_num_collision_meshes, gripper_idx, save_path):
    _gripper("gripper_2d", left_num_collision_meshes, right_num_collision_meshes, gripper_idx, save_path)


# the reference keeps two writers of the same file (they differ in attribute order only)
generate_xml_optimized = generate_xml


def generate_gripper_3d_xml(left_num_collision_meshes, right_num_collision_meshes, gripper_idx, save_path):
    _gripper("gripper_3d", left_num_collision_meshes, right_num_collision_meshes, gripper_idx, save_path)


def generate_scene_xml(object_idx, gripper_idx, save_path):
    """The scene: the collision / visual geom classes, the object and gripper files included by name, a ground plane."""
    root = ("mujoco", {"model": "scene"}, [
        ("default", {}, [
            ("default", {"class": "collision"}, [("geom", {"group": "3", "condim": "4", "friction": "1.0 0.005 0.0001"}, [])]),
            ("default", {"class": "visual"}, [("geom", {"group": "2", "contype": "0", "conaffinity": "0"}, [])])]),
        ("include", {"file": "object_%d.xml" % object_idx}, []),
        ("include", {"file": "gripper_%d.xml" % gripper_idx}, []),
        ("worldbody", {}, [("body", {"name": "plane", "pos": "0 0 -0.01"},
                            [("geom", {"type": "plane", "size": "1 1 0.1", "rgba": "1.0 1.0 1.0 1"}, [])])]),
    ])
    ET.ElementTree(_build(root)).write(save_path)


generate_scene_3d_xml = generate_scene_xml          # the 2-D and 3-D scene files are the same
