"""Host side of the sliced-squeeze labels for 3-D fingers: the composed oracle (tests/squeeze3d_oracle.py, then
tests/squeeze_label_oracle.py) against the closed-form result of tests/test_squeeze_label_host.py, the 'squeeze_3d' source in
LabelStats' files, and the command line's refusals.  No GPU."""
import json

import numpy as np
import pytest

from dgdm_amd import label as lb
from dgdm_amd.dynamics.dataloader import POS_NORM, SCORE_STD, SCORE_THRESHOLD
from dgdm_amd.dynamics.parser import parse
from dgdm_amd.generator import train as gtrain
from dgdm_amd.sim import squeeze
from tests import resample_squeeze_oracle as rso
from tests import squeeze3d_oracle as so3
from tests import squeeze_label_oracle as slo
from tests import squeeze_oracle as so

THR, STD = [float(v) for v in SCORE_THRESHOLD[1]], [float(v) for v in SCORE_STD[1]]       # the closed form's, as the 2-D test states it
GX = np.array([-0.12, -0.07, 0.0, 0.03, 0.12])
GZ = np.array([0.0, 0.02, 0.05])


def rectangle_prism(z0=-0.01, z1=0.06):
    """The 0.06 x 0.03 m rectangle extruded from z0 to z1: two triangles per wall."""
    poly = np.array([[-0.03, -0.015], [0.03, -0.015], [0.03, 0.015], [-0.03, 0.015]])
    v = np.concatenate([np.c_[poly, np.full(4, z0)], np.c_[poly, np.full(4, z1)]])
    f = []
    for i in range(4):
        j = (i + 1) % 4
        f += [[i, j, 4 + j], [i, 4 + j, 4 + i]]
    return v, np.array(f, dtype=np.int32)


@pytest.mark.parametrize("k,R", [(6, 2), (3, 1)])
def test_composed_oracle_gives_the_closed_form(k, R):
    """test_rectangle_between_flat_jaws_closed_form with the rectangle as a prism through all three levels between flat faces on GX x GZ:
    every level holds the 2-D problem, so the least gap over the levels is the 2-D one and the assertions are that test's, unchanged."""
    T, X, G, ori = 360, 5, 37, (-0.3, 0.3)
    starts = np.concatenate([rso.start_grid(G, 1, ori), squeeze.start_orientations(G, ori)])
    rot = so.rotation_table(T)
    flat = np.stack([np.full((len(GZ), len(GX)), -0.12), np.full((len(GZ), len(GX)), 0.15)])[None]
    seg, off = so3.slice_meshes([rectangle_prism()], GZ)
    assert np.diff(off, axis=1).tolist() == [[8, 8, 8]]
    out = so3.squeeze_map_3d(flat, GX, seg, off, [(0, 0)], rot, starts, x_cells=X, x_half=0.06, window=R, closing_steps=k, travel_max=0.2)
    d = 3 * np.abs(np.arange(G) - 18)
    a0, ak, af = (out["cells"][0, :, j] // X for j in range(3))
    assert np.array_equal(a0[:G], 126 + 3 * np.arange(G)) and (af == 180).all()
    assert np.array_equal(np.abs(ak - a0)[:G], np.minimum(d, k * R)) and np.array_equal(np.abs(ak[:G] - 180), d - np.minimum(d, k * R))
    rows, counts = slo.label_rows(out["cells"], out["y"], out["flags"], starts, G, 1, rot, T, X, 0.06, THR, STD, POS_NORM)
    r = rows[0].astype(np.float64)
    f = float(np.float32(18.0 / 37.0))
    assert rows.shape == (1, 15) and rows.dtype == np.float32
    assert r[0] == f and r[1] == f and r[2] == 0 and r[3] == 0 and r[4] == 0 and r[5] == 1
    want = np.minimum(d, k * R).sum() * (2.0 * np.pi / 360.0) / 0.0565 / 37.0
    assert abs(r[6]) < 1e-6 and abs(r[7] - want) <= 1e-6 * want and r[8] == 0
    assert abs(r[9] - (0.015 + POS_NORM) / STD[2]) <= 1e-6 * r[9]
    assert abs(r[10] - 1.0) < 1e-6 and r[11] == -1.0 and abs(r[12]) < 1e-12 and abs(r[13] - 0.5) < 1e-6 and r[14] == 0
    assert not counts.any() and counts.shape == (1, 3)


def test_label_stats_squeeze_3d_round_trip(tmp_path):
    thr3 = [float(v) for v in SCORE_THRESHOLD[0]]
    recipe = {"G": 9, "P": 3, "ori_range": [-1.0, 1.0], "score_std": [float(v) for v in SCORE_STD[0]], "source": "squeeze_3d",
              "squeeze_config": {"theta_cells": 90, "x_cells": 33, "window": 2, "closing_steps": 6, "x_half": 0.06, "travel_max": 0.1, "finger_half_len": 0.12},
              "sample_size": 25, "width": 0.1, "settled": True, "threshold": thr3}
    assert "squeeze_3d" in lb.SOURCES
    cols = lb.TALLY_COLUMNS + lb.SETTLED_COLUMNS
    st = lb.LabelStats(cols, "mean", ["a", "b"], recipe).fit(np.random.RandomState(5).uniform(0, 1, (9, 15)))
    assert st.source == "squeeze_3d"
    f = str(tmp_path / "rows.json")
    st.save(f)
    d = json.load(open(f))
    assert d["source"] == "squeeze_3d" and d["simulated"] == "squeeze" and "predicted" not in d and "friction" not in d
    assert d["squeeze_config"] == recipe["squeeze_config"] and d["sample_size"] == 25 and d["width"] == 0.1 and d["settled"] is True and d["threshold"] == thr3
    back = lb.LabelStats.load(f)
    assert back.source == "squeeze_3d" and back.columns == cols and all(back.recipe[k] == v for k, v in recipe.items())
    assert np.array_equal(back.target({"frac_up": 0.7}), st.target({"frac_up": 0.7}))
    back.save(str(tmp_path / "again.json"))
    assert open(f, "rb").read() == open(tmp_path / "again.json", "rb").read()
    d["source"] = "mujoco"                                                # an unknown source is refused as before
    json.dump(d, open(tmp_path / "bad.json", "w"))
    with pytest.raises(ValueError, match="cond_stats"):
        lb.LabelStats.load(str(tmp_path / "bad.json"))


def test_flag_refusals_before_any_gpu_work(tmp_path, monkeypatch):
    """Every refusal of --label_source squeeze_3d is raised by train() before anything is built, with a message that names the flag."""
    rows = str(tmp_path / "rows.npy")
    on = f"--mode=label --label_source squeeze_3d --fingers_3d --label_out {rows}"
    assert parse(on.split()).label_source == "squeeze_3d"

    def refused(flags, match):
        with pytest.raises(ValueError, match=match):
            gtrain.train(parse(flags.split() + ["--num_fingers=8", "--batch_size=4", "--ctrlpts_dim=42"]))
    refused(f"--mode=label --label_source squeeze_3d --label_out {rows}", "--fingers_3d")
    refused("--mode=label --label_source squeeze_3d --fingers_3d", "--label_out")
    refused(f"--mode=label --label_source mujoco --label_out {rows}", "label_source.*squeeze_3d")
    refused(on + " --squeeze_friction 0.5", "--squeeze_friction.*2-D only")
    refused(on + " --label_rollout 3", "label_rollout")
    refused(on + " --label_squeeze_cells 90", "label_squeeze_cells")
    refused(on + " --squeeze_window 0", "window")
    refused(on + " --squeeze_closing_steps -1", "negative")
    refused(on + " --label_layout median", "label_layout")
    refused(on + f" --global_cond {rows}", "--global_cond")
    refused("--mode=test --fingers_3d --label_source squeeze_3d", "--mode=label")
    refused(on + f" --object_dir {tmp_path}", "model.obj")                # no mesh files there: SqueezeSimulator3D's refusal
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    refused(on, "one process")
    monkeypatch.delenv("WORLD_SIZE")
    # accepted by the flag checks: the squeeze flags belong to this source too, which needs no --classifier_guidance
    args = parse((on + " --label_settled --label_squeeze_cells 90,33 --squeeze_closing_steps 4 --squeeze_window 1").split())
    assert gtrain.check_label_flags(args) == (None, None) and gtrain.squeeze_from_args(args) is None
    assert gtrain.label_squeeze_config(args) == ({"theta_cells": 90, "x_cells": 33, "closing_steps": 4, "window": 1}, 0.0)
    # the existing refusals keep their text
    refused(f"--mode=label --label_source squeeze --fingers_3d --label_out {rows}", "2-D only.*out of scope")
    # statistics of squeeze_3d rows: the run needs --fingers_3d
    st = lb.LabelStats(lb.TALLY_COLUMNS, "mean", ["a", "b"], {"G": 9, "P": 3, "source": "squeeze_3d"}).fit(np.random.RandomState(6).uniform(0, 1, (5, 10)))
    stats = str(tmp_path / "rows.json")
    st.save(stats)
    refused(f"--mode=test --cond_stats {stats} --cond_target frac_up=0.7", "--fingers_3d")
    got, requested = gtrain.check_label_flags(parse(f"--mode=test --fingers_3d --cond_stats {stats} --cond_target frac_up=0.7".split()))
    assert got.source == "squeeze_3d" and requested == {"frac_up": 0.7}
    refused(f"--mode=test --fingers_3d --cond_stats {stats} --cond_target frac_up=0.7 --object_dir {tmp_path}", "model.obj")
