"""Host side of the squeeze-simulator labels: the oracle tests/squeeze_label_oracle.py against a closed-form result, the label source in
LabelStats' files, and the command line's refusals.  No GPU."""
import json
import os

import numpy as np
import pytest

from dgdm_amd import label as lb
from dgdm_amd.dynamics.dataloader import POS_NORM, SCORE_STD, SCORE_THRESHOLD
from dgdm_amd.dynamics.parser import parse
from dgdm_amd.generator import train as gtrain
from dgdm_amd.sim import squeeze
from tests import resample_squeeze_oracle as rso
from tests import squeeze_label_oracle as slo
from tests import squeeze_oracle as so

THR, STD = [float(v) for v in SCORE_THRESHOLD[1]], [float(v) for v in SCORE_STD[1]]
RECT = np.array([[-0.03, -0.015], [0.03, -0.015], [0.03, 0.015], [-0.03, 0.015]])       # 0.06 x 0.03 m


@pytest.mark.parametrize("k,R", [(6, 2), (3, 1)])
def test_rectangle_between_flat_jaws_closed_form(k, R):
    """Flat jaws (L = -0.12, U = 0.15), 360 x 5 cells, travel_max 0.2; 37 start orientations within +-54 degrees of 180, inside its basin
    (edged at atan 2 = 63.43 degrees): a start d cells away turns min(d, k R) cells toward it, and settles on it."""
    T, X, G, ori, m = 360, 5, 37, (-0.3, 0.3), 16
    starts = np.concatenate([rso.start_grid(G, 1, ori), squeeze.start_orientations(G, ori)])
    rot = so.rotation_table(T)
    out = so.squeeze_pair(np.full(m, -0.12), np.full(m, 0.15), RECT, rot, starts, X, 0.06, R, k, 0.2)
    d = 3 * np.abs(np.arange(G) - 18)
    a0, ak, af = (out["cells"][:, j] // X for j in range(3))
    assert np.array_equal(a0[:G], 126 + 3 * np.arange(G)) and (af == 180).all()
    assert np.array_equal(np.abs(ak - a0)[:G], np.minimum(d, k * R)) and np.array_equal(np.abs(ak[:G] - 180), d - np.minimum(d, k * R))
    rows, counts = slo.label_rows(out["cells"][None], out["y"][None], out["flags"][None], starts, G, 1, rot, T, X, 0.06, THR, STD, POS_NORM)
    r = rows[0].astype(np.float64)
    f = float(np.float32(18.0 / 37.0))
    assert rows.shape == (1, 15) and rows.dtype == np.float32
    assert r[0] == f and r[1] == f and r[2] == 0 and r[3] == 0 and r[4] == 0 and r[5] == 1      # class counts 18 / 1 / 18; y = 0.015 from y0 < 0
    want = np.minimum(d, k * R).sum() * (2.0 * np.pi / 360.0) / 0.0565 / 37.0
    assert abs(r[6]) < 1e-6 and abs(r[7] - want) <= 1e-6 * want and r[8] == 0
    assert abs(r[9] - (0.015 + POS_NORM) / STD[2]) <= 1e-6 * r[9]            # P = 1: the grid's only position is (-POS_NORM, -POS_NORM)
    assert abs(r[10] - 1.0) < 1e-6 and r[11] == -1.0 and abs(r[12]) < 1e-12 and abs(r[13] - 0.5) < 1e-6 and r[14] == 0
    assert not counts.any() and counts.shape == (1, 3)


def test_oracle_layouts_and_wave_order():
    """'per_object' blocks are the 'mean' rows of each object alone; 'mean' sums the counts before the one division; the sums follow the
    64-lane stride (a reordering of the starts changes their bits, not the counts)."""
    T, X = 24, 9
    rs = np.random.RandomState(4)
    n, nt = 156, 150
    cells = rs.randint(0, T * X, (4, n, 3))
    y = rs.uniform(-0.02, 0.02, (4, n, 2))
    flags = rs.randint(0, 8, (4, n))
    starts = np.concatenate([rso.start_grid(6, 5, (-1.0, 1.0)), squeeze.start_orientations(6, (-1.0, 1.0))])
    rot = so.rotation_table(T)
    args = (rot, T, X, 0.06, THR, STD, POS_NORM)
    per, counts = slo.label_rows(cells, y, flags, starts, nt, 2, *args, layout="per_object")
    mean, counts_m = slo.label_rows(cells, y, flags, starts, nt, 2, *args, layout="mean")
    assert per.shape == (2, 30) and mean.shape == (2, 15) and np.array_equal(counts, counts_m)
    for p in range(4):
        alone, _ = slo.label_rows(cells[p:p + 1], y[p:p + 1], flags[p:p + 1], starts, nt, 1, *args)
        assert np.array_equal(alone[0].view(np.int32), per[p // 2, 15 * (p % 2):15 * (p % 2 + 1)].view(np.int32))
    cls, sums, flag, settle = slo.pair_partials(cells, y, flags, starts, nt, *args)
    assert np.array_equal(mean[:, :6], ((cls[0::2] + cls[1::2]) / float(2 * nt)).astype(np.float32))
    assert np.array_equal(counts, flag[0::2] + flag[1::2]) and settle.shape == (4, 5)
    perm = np.concatenate([rs.permutation(nt), np.arange(nt, n)])
    cls2, sums2, _, _ = slo.pair_partials(cells[:, perm], y[:, perm], flags[:, perm], starts[perm], nt, *args)
    assert np.array_equal(cls, cls2) and np.allclose(sums, sums2, rtol=1e-12, atol=1e-12) and not np.array_equal(sums, sums2)
    tally_only, _ = slo.label_rows(cells[:, :nt], y[:, :nt], flags[:, :nt], starts[:nt], nt, 2, *args)
    assert tally_only.shape == (2, 10) and np.array_equal(tally_only.view(np.int32), mean[:, :10].view(np.int32))


def test_label_stats_source_round_trip(tmp_path):
    recipe = {"G": 9, "P": 3, "ori_range": [-1.0, 1.0], "score_std": STD, "source": "squeeze",
              "squeeze_config": {"theta_cells": 90, "x_cells": 33, "window": 2, "closing_steps": 6, "x_half": 0.06, "travel_max": 0.1, "finger_half_len": 0.12},
              "friction": 0.25, "settled": True, "threshold": THR}
    cols = lb.TALLY_COLUMNS + lb.SETTLED_COLUMNS
    st = lb.LabelStats(cols, "mean", [3, 4], recipe).fit(np.random.RandomState(5).uniform(0, 1, (9, 15)))
    assert st.source == "squeeze"
    f = str(tmp_path / "rows.json")
    st.save(f)
    d = json.load(open(f))
    assert d["simulated"] == "squeeze" and "predicted" not in d and d["source"] == "squeeze"
    assert d["squeeze_config"] == recipe["squeeze_config"] and d["friction"] == 0.25 and d["settled"] is True and d["threshold"] == THR
    back = lb.LabelStats.load(f)
    assert back.source == "squeeze" and back.columns == cols and all(back.recipe[k] == v for k, v in recipe.items())
    assert np.array_equal(back.target({"frac_up": 0.7}), st.target({"frac_up": 0.7}))
    back.save(str(tmp_path / "again.json"))
    assert open(f, "rb").read() == open(tmp_path / "again.json", "rb").read()
    d["source"] = "mujoco"
    json.dump(d, open(tmp_path / "bad.json", "w"))
    with pytest.raises(ValueError, match="cond_stats"):
        lb.LabelStats.load(str(tmp_path / "bad.json"))


def test_a_file_without_source_is_the_models(tmp_path):
    """The files of model labels are what they were: no 'source' key, 'predicted': true; one written before the key existed loads as
    'model' and is saved again byte for byte."""
    recipe = {"G": 9, "P": 3, "ori_range": [-1.0, 1.0], "threshold_std": [0.5, 0.7, 0.6], "score_std": [0.05, 0.002, 0.004], "K": 0, "timestep": 0,
              "seed": 5, "contraction_dtype": "f32"}
    st = lb.LabelStats(lb.TALLY_COLUMNS, "mean", [10000, 2009], recipe).fit(np.random.RandomState(5).uniform(0, 1, (9, 10)))
    old = {"columns": st.columns, "mean": st.mean.tolist(), "std": st.std.tolist(), "min": st.min.tolist(), "max": st.max.tolist(), "layout": "mean",
           "object_ids": [10000, 2009], **recipe, "predicted": True}                       # to_dict before the key, spelt out
    f = tmp_path / "old.json"
    with open(f, "w") as fh:
        json.dump(old, fh, indent=1)
    st.save(str(tmp_path / "new.json"))
    assert open(f, "rb").read() == open(tmp_path / "new.json", "rb").read()
    back = lb.LabelStats.load(str(f))
    assert back.source == "model" and "source" not in back.recipe and back.recipe == recipe
    back.save(str(tmp_path / "again.json"))
    assert open(f, "rb").read() == open(tmp_path / "again.json", "rb").read()
    assert list(lb.LabelStats(lb.TALLY_COLUMNS, "mean", [1], {"source": "model"}).to_dict())[-1] == "predicted"


def test_flag_refusals_before_any_gpu_work(tmp_path, monkeypatch):
    """Every refusal of --label_source / --label_settled / --label_squeeze_cells is raised by train() before anything is built."""
    a = parse([])
    assert a.label_source == "model" and not a.label_settled and a.label_squeeze_cells is None
    rows = str(tmp_path / "rows.npy")
    on = f"--mode=label --label_source squeeze --label_out {rows}"

    def refused(flags, match):
        with pytest.raises(ValueError, match=match):
            gtrain.train(parse(flags.split() + ["--num_fingers=8", "--batch_size=4"]))
    refused("--mode=label --label_source squeeze", "--label_out")
    refused(f"--mode=label --label_source mujoco --label_out {rows}", "label_source")
    refused(on + " --fingers_3d", "2-D only.*out of scope")
    refused(on + " --label_rollout 3", "label_rollout")
    refused(f"--mode=label --classifier_guidance --label_out {rows} --label_settled", "--label_source squeeze")
    refused(f"--mode=label --classifier_guidance --label_out {rows} --label_squeeze_cells 90,33", "--label_source squeeze")
    refused("--mode=test --label_settled", "--label_source squeeze")
    refused("--mode=test --label_source squeeze", "--mode=label")
    refused(on + " --label_squeeze_cells 90", "label_squeeze_cells")
    refused(on + " --label_squeeze_cells 0,5", "label_squeeze_cells")
    refused(on + " --squeeze_window 0", "window")
    refused(on + " --squeeze_closing_steps -1", "negative")
    refused(on + " --squeeze_friction -0.5", "finite non-negative")
    refused(on + " --label_layout median", "label_layout")
    refused(on + f" --global_cond {rows}", "--global_cond")
    refused(f"--mode=label --label_out {rows} --squeeze_friction 0.5", "--squeeze_friction needs")       # the model's labels use no squeeze flag
    refused(f"--mode=label --label_out {rows}", "--classifier_guidance")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    refused(on, "one process")
    monkeypatch.delenv("WORLD_SIZE")
    # accepted: the squeeze flags belong to --label_source squeeze, which needs no --classifier_guidance
    args = parse((on + " --label_settled --label_squeeze_cells 90,33 --squeeze_closing_steps 4 --squeeze_window 1 --squeeze_friction 0.25").split())
    assert gtrain.check_label_flags(args) == (None, None) and gtrain.squeeze_from_args(args) is None
    assert gtrain.label_squeeze_config(args) == ({"theta_cells": 90, "x_cells": 33, "closing_steps": 4, "window": 1}, 0.25)
    # statistics of squeeze rows: 2-D only, and the run's grid is not the report's
    st = lb.LabelStats(lb.TALLY_COLUMNS, "mean", [1, 2], {"G": 9, "P": 3, "source": "squeeze"}).fit(np.random.RandomState(6).uniform(0, 1, (5, 10)))
    stats = str(tmp_path / "rows.json")
    st.save(stats)
    refused(f"--mode=test --fingers_3d --cond_stats {stats} --cond_target frac_up=0.7", "2-D only")
    got, requested = gtrain.check_label_flags(parse(f"--mode=test --classifier_guidance --grid_size=8 --cond_stats {stats} --cond_target frac_up=0.7".split()))
    assert got.source == "squeeze" and requested == {"frac_up": 0.7}
    assert os.path.exists(stats) and not os.path.exists(rows)
