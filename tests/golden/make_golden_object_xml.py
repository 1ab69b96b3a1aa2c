#!/usr/bin/env python
"""Record the MuJoCo object files the REFERENCE's writers produce, as fixtures under tests/golden/object_xml/.

    python tests/golden/make_golden_object_xml.py <reference checkout>

The writers (assets/object_sampler.py: generate_object_xml; assets/scan_object_process.py: generate_object_3d_xml) are plain
xml.etree code, but the second module imports open3d, matplotlib and tqdm at the top, which are not dependencies of this project:
empty stand-in modules are registered for those imports (and for cv2, trimesh and triangle, which their neighbours import), the
reference's modules are loaded from their files and its functions called.  Only the files they write are committed (scene data, a few
hundred bytes each); nothing of the reference's text is stored.  tests/test_object_xml_host.py compares this project's writers with
them element by element.

Collision-piece counts 0, 3 and 16 (the reference's V-HACD hull cap in 2-D); object index 4, the one the recorded scene files include."""
import importlib.util
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "object_xml")
COUNTS = [0, 3, 16]
OBJECT_IDX = 4


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
    for missing in ("open3d", "cv2", "trimesh", "triangle"):
        if missing not in sys.modules:
            _stand_in(missing)
    if "tqdm" not in sys.modules:
        _stand_in("tqdm", tqdm=None)                 # `from tqdm import tqdm`; the writers never call it
    if "matplotlib" not in sys.modules:
        _stand_in("matplotlib", pyplot=_stand_in("matplotlib.pyplot"))
    o2 = _load(ref, os.path.join("assets", "object_sampler.py"), "_ref_object_sampler")
    o3 = _load(ref, os.path.join("assets", "scan_object_process.py"), "_ref_scan_object_process")
    os.makedirs(OUT, exist_ok=True)
    for k in COUNTS:
        o2.generate_object_xml(k, OBJECT_IDX, os.path.join(OUT, f"object_2d_{k}.xml"))
        o3.generate_object_3d_xml(k, OBJECT_IDX, os.path.join(OUT, f"object_3d_{k}.xml"))
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
