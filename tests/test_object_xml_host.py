"""CPU tests of the object files of an exported model root (dgdm_amd/assets/object_sampler.py, scan_object_process.py): the XML writers
against the files recorded from the reference (tests/golden/object_xml/, by tests/golden/make_golden_object_xml.py), element by element,
and the list of object names."""
import os

import pytest

from assets import object_sampler, scan_object_process
from tests import finger_mesh_oracle as fmo

WRITERS = {"object_2d": object_sampler.generate_object_xml, "object_3d": scan_object_process.generate_object_3d_xml}


@pytest.mark.parametrize("count", [0, 3, 16])
@pytest.mark.parametrize("name", sorted(WRITERS))
def test_object_xml_matches_the_reference_files(name, count, golden_dir, tmp_path):
    """tag, attribute dict and child order of every element."""
    out = str(tmp_path / "o.xml")
    WRITERS[name](count, 4, out)
    assert fmo.xml_tree(out) == fmo.xml_tree(os.path.join(golden_dir, "object_xml", f"{name}_{count}.xml"))


def test_the_scene_includes_the_object_file(golden_dir):
    """The recorded scene includes object_4.xml, and the recorded object file names its meshes under objects/4/."""
    scene = fmo.xml_tree(os.path.join(golden_dir, "gripper_xml", "scene_2d.xml"))
    assert ("include", {"file": "object_4.xml"}, []) in scene[2]
    asset = fmo.xml_tree(os.path.join(golden_dir, "object_xml", "object_2d_3.xml"))[2][0]
    assert [c[1]["file"] for c in asset[2]] == ["objects/4/object.obj"] + [f"objects/4/object{i:03d}.obj" for i in range(3)]


def test_read_object_names(tmp_path, monkeypatch):
    d = tmp_path / "assets"
    d.mkdir()
    (d / "object_names.txt").write_text("BABY_CAR\n 3D_Dollhouse_Swing \n")
    (d / "object_names_test.txt").write_text("Squirt_Strain_Fruit_Basket\n")
    monkeypatch.chdir(tmp_path)
    assert scan_object_process.read_object_names() == ["BABY_CAR", "3D_Dollhouse_Swing"]
    assert scan_object_process.read_object_names(test=True) == ["Squirt_Strain_Fruit_Basket"]
    assert scan_object_process.read_object_names(root=str(d)) == ["BABY_CAR", "3D_Dollhouse_Swing"]
