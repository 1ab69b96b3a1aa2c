#!/usr/bin/env python
"""Record the MuJoCo XML files the REFERENCE's writers produce, as fixtures under tests/golden/gripper_xml/.

    python tests/golden/make_golden_gripper_xml.py <reference checkout>

The writers (assets/finger_sampler.py: generate_xml, generate_xml_optimized, generate_scene_xml; assets/finger_3d.py:
generate_gripper_3d_xml, generate_scene_3d_xml) are plain xml.etree code, but their modules import trimesh and geomdl at the top,
which are not dependencies of this project: empty stand-in modules are registered for those imports, the reference's modules are
loaded from their files and its functions called.  Only the files they write are committed (scene data, a few hundred bytes each);
nothing of the reference's text is stored.  tests/test_finger_mesh_host.py compares this project's writers with them element by element.

Collision-piece counts (left, right): (0, 0), (3, 5) - unequal, so that a left/right mix-up shows - and (16, 16), the reference's V-HACD
hull cap in 2-D.  Gripper index 7, object index 4."""
import importlib.util
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gripper_xml")
COUNTS = [(0, 0), (3, 5), (16, 16)]
GRIPPER_IDX, OBJECT_IDX = 7, 4


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    for missing in ("trimesh",):
        if missing not in sys.modules:
            _stand_in(missing)
    if "geomdl" not in sys.modules:
        sub = {n: _stand_in("geomdl." + n) for n in ("BSpline", "utilities", "exchange")}
        _stand_in("geomdl", **sub)
    fs = _load(ref, os.path.join("assets", "finger_sampler.py"), "_ref_finger_sampler")
    f3 = _load(ref, os.path.join("assets", "finger_3d.py"), "_ref_finger_3d")
    os.makedirs(OUT, exist_ok=True)
    for nl, nr in COUNTS:
        fs.generate_xml(nl, nr, GRIPPER_IDX, os.path.join(OUT, f"gripper_2d_{nl}_{nr}.xml"))
        fs.generate_xml_optimized(nl, nr, GRIPPER_IDX, os.path.join(OUT, f"gripper_2d_optimized_{nl}_{nr}.xml"))
        f3.generate_gripper_3d_xml(nl, nr, GRIPPER_IDX, os.path.join(OUT, f"gripper_3d_{nl}_{nr}.xml"))
    fs.generate_scene_xml(OBJECT_IDX, GRIPPER_IDX, os.path.join(OUT, "scene_2d.xml"))
    f3.generate_scene_3d_xml(OBJECT_IDX, GRIPPER_IDX, os.path.join(OUT, "scene_3d.xml"))
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
