"""CPU tests of the labelling layer (dgdm_amd/label.py, the --mode=label / --cond_target flags) and of the numpy oracle the GPU tests use."""
import json

import numpy as np
import pytest

from dgdm_amd import label as lb
from dgdm_amd.dynamics.parser import parse
from dgdm_amd.generator import train as gtrain
from tests import label_oracle as lo


def one_bin(d0, d1, d2, n):
    c = np.zeros((3, 3, 3), dtype=np.int32)
    c[d0, d1, d2] = n
    return c


def test_oracle_every_cell_in_one_bin():
    """All n cells in bin (0, 2, 1): clockwise and down on the whole grid, no left / right - fractions of exactly 1 and 0."""
    n = 81
    row = lo.tally_block(one_bin(0, 2, 1, n)[None], np.array([[-8.1, 8.1, 4.05, 0.0]], dtype=np.float32), n)
    assert row.dtype == np.float32 and row.shape == (10,)
    assert row[:6].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert row[6] == np.float32(np.float64(np.float32(-8.1)) / 81.0) and row[7] == -row[6] and row[9] == 0.0
    # two objects in opposite corners: each marginal holds half of the 2 n cells
    both = np.stack([one_bin(0, 0, 0, n), one_bin(2, 2, 2, n)])
    row = lo.tally_block(both, np.zeros((2, 4), dtype=np.float32), n)
    assert row[:6].tolist() == [0.5] * 6 and row[6:].tolist() == [0.0] * 4
    # the layouts: (M, B) tallies -> (B, 10) and (B, M, 10)
    counts = both[:, None].repeat(3, axis=1)
    sums = np.zeros((2, 3, 4), dtype=np.float32)
    assert lo.tally_rows(counts, sums, n, "mean").shape == (3, 10)
    per = lo.tally_rows(counts, sums, n, "per_object")
    assert per.shape == (3, 2, 10) and per[1, 0, :6].tolist() == [1, 0, 1, 0, 1, 0] and per[1, 1, :6].tolist() == [0, 1, 0, 1, 0, 1]


def test_oracle_settled_columns():
    G = 8
    same = np.tile(np.array([[-0.5, 0.3, 0.4]]), (G, 1))                        # every start settles at theta = pi / 2, 0.5 from the centre
    left = np.array([-1, -1, 3, -1, 0, -1, -1, -1])
    row = lo.settled_block(same[None], left[None])
    assert abs(row[0] - 1.0) <= 2 ** -23 and abs(row[1]) <= 2 ** -23 and abs(row[2] - 1.0) <= 2 ** -23
    assert row[3] == np.float32(0.5) and row[4] == np.float32(0.25)
    spread = same.copy()
    spread[:, 0] = np.linspace(-1.0, 1.0, G, endpoint=False)                    # evenly round the circle: no concentration
    assert abs(lo.settled_block(spread[None], left[None])[0]) < 1e-6
    bad = same.copy()
    bad[2, 1] = np.inf
    row = lo.settled_block(np.stack([same, bad]), np.stack([left, left]))
    assert np.isnan(row[:4]).all() and row[4] == np.float32(0.25)
    final = np.stack([same, spread]).reshape(2, G, 1, 3).repeat(2, axis=2).reshape(2, G * 2, 3)     # row = g * B + b, B = 2
    lf = np.stack([left, left]).reshape(2, G, 1).repeat(2, axis=2).reshape(2, G * 2)
    assert lo.settled_rows(final, lf, 2, "mean").shape == (2, 5) and lo.settled_rows(final, lf, 2, "per_object").shape == (2, 2, 5)


def test_column_names_both_layouts():
    assert len(lb.TALLY_COLUMNS) == 10 and len(lb.SETTLED_COLUMNS) == 5
    assert lb.column_names("mean", [7, 9]) == lb.TALLY_COLUMNS
    assert lb.column_names("mean", [7, 9], rollout=3) == lb.TALLY_COLUMNS + lb.SETTLED_COLUMNS
    names = lb.column_names("per_object", [10000, "cup"], rollout=2)
    assert len(names) == 30 and names[2] == "frac_up@10000" and names[10] == "settle_concentration@10000" and names[15] == "frac_clockwise@cup"
    with pytest.raises(ValueError, match="layout"):
        lb.column_names("median", [1])
    assert lb.cond_dim("per_object", 17, 5) == 255
    with pytest.raises(ValueError, match="256"):
        lb.cond_dim("per_object", 18, 5)
    with pytest.raises(ValueError, match="256"):
        lb.cond_dim("per_object", 26, 0)


def stats_mean():
    raw = np.random.RandomState(3).uniform(0, 1, (20, 10)).astype(np.float32)
    raw[:, 4] = 0.25                                                            # a constant column
    return lb.LabelStats(lb.column_names("mean", [1, 2]), "mean", [1, 2], {"G": 9, "P": 3}).fit(raw), raw


def test_label_stats_fit_apply_target():
    st, raw = stats_mean()
    r64 = raw.astype(np.float64)
    assert np.array_equal(st.mean, r64.mean(0)) and np.array_equal(st.std, r64.std(0))
    assert st.constant.tolist() == [False] * 4 + [True] + [False] * 5
    z = st.apply(raw)
    assert z.dtype == np.float32 and z.shape == raw.shape and np.isfinite(z).all()
    assert (z[:, 4] == 0).all()                                                 # the constant column standardises to 0
    keep = ~st.constant
    assert np.abs(z[:, keep].astype(np.float64).mean(0)).max() < 1e-6 and np.abs(z[:, keep].astype(np.float64).std(0) - 1).max() < 1e-6
    t = st.target({"frac_clockwise": 0.9, "frac_up": 0.7})
    assert t.dtype == np.float32 and t.shape == (10,)
    assert t[0] == np.float32((0.9 - st.mean[0]) / st.std[0]) and t[2] == np.float32((0.7 - st.mean[2]) / st.std[2])
    assert (np.delete(t, [0, 2]) == 0).all()                                    # unnamed columns: the dataset mean
    assert (st.target({"frac_left": 0.9}) == 0).all()                           # a constant column carries no information
    with pytest.raises(ValueError, match="10 columns"):
        st.apply(raw[:, :9])
    with pytest.raises(ValueError, match="non-finite"):
        lb.LabelStats(lb.TALLY_COLUMNS).fit(np.full((2, 10), np.nan))


def test_label_stats_aliases_and_refusals():
    st, _ = stats_mean()
    assert len(lb.ALIASES) == 14
    assert st.requested({"clockwise_up": 0.8}) == {"frac_clockwise": 0.8, "frac_up": 0.8}
    assert st.requested({"rotate_counterclockwise": 0.6}) == {"frac_counterclockwise": 0.6}
    assert st.requested({"shift_right": 0.5}) == {"frac_right": 0.5}
    assert st.requested({"counterclockwise_down": 0.5}) == {"frac_counterclockwise": 0.5, "frac_down": 0.5}
    with pytest.raises(ValueError, match="frac_clockwise and frac_counterclockwise"):
        st.target({"rotate": 0.9})
    with pytest.raises(ValueError, match="settle_concentration"):
        st.target({"convergence": 0.9})
    with pytest.raises(ValueError, match="unknown column 'frac_sideways'"):
        st.target({"frac_sideways": 0.9})
    with pytest.raises(ValueError, match="unknown column 'settle_concentration'"):      # these rows were labelled without a roll-out
        st.target({"settle_concentration": 1.0})
    # per_object: a bare name (or an alias) sets the column for every object, a full name one
    raw = np.random.RandomState(4).uniform(0, 1, (6, 20))
    po = lb.LabelStats(lb.column_names("per_object", [7, 9]), "per_object", [7, 9]).fit(raw)
    assert po.requested({"frac_up": 0.7}) == {"frac_up@7": 0.7, "frac_up@9": 0.7}
    assert po.requested({"frac_up@9": 0.7}) == {"frac_up@9": 0.7}
    assert set(po.requested({"clockwise_left": 0.3})) == {"frac_clockwise@7", "frac_left@7", "frac_clockwise@9", "frac_left@9"}
    t = po.target({"frac_up@9": 0.7})
    assert np.count_nonzero(t) == 1 and t[12] == np.float32((0.7 - po.mean[12]) / po.std[12])
    with pytest.raises(ValueError, match="unknown column"):
        po.target({"frac_up@8": 0.7})
    assert lb.parse_target("frac_clockwise=0.9, frac_up=0.7") == {"frac_clockwise": 0.9, "frac_up": 0.7}
    for bad in ("frac_up", "frac_up=", "=0.3", "frac_up=high", "frac_up=0.1,frac_up=0.2", "frac_up=nan"):
        with pytest.raises(ValueError, match="cond_target"):
            lb.parse_target(bad)


def test_label_stats_json_round_trip(tmp_path):
    recipe = {"G": 9, "P": 3, "ori_range": [-1.0, 1.0], "threshold_std": [0.5, 0.7, 0.6], "score_std": [0.05, 0.002, 0.004], "K": 0, "timestep": 0,
              "seed": 5, "contraction_dtype": "f32"}
    raw = np.random.RandomState(5).uniform(0, 1, (9, 10))
    st = lb.LabelStats(lb.TALLY_COLUMNS, "mean", [10000, 2009], recipe).fit(raw)
    f = str(tmp_path / "rows.json")
    st.save(f)
    d = json.load(open(f))
    assert d["predicted"] is True and d["layout"] == "mean" and d["object_ids"] == [10000, 2009] and d["columns"] == lb.TALLY_COLUMNS
    assert all(k in d for k in ("mean", "std", "min", "max", "G", "P", "ori_range", "threshold_std", "score_std", "K", "timestep", "seed", "contraction_dtype"))
    back = lb.LabelStats.load(f)
    assert back.columns == st.columns and back.layout == st.layout and back.object_ids == st.object_ids and back.recipe == st.recipe
    for k in ("mean", "std", "min", "max"):
        assert np.array_equal(getattr(back, k), getattr(st, k)), k               # repr of a double round-trips through JSON
    assert np.array_equal(back.target({"frac_up": 0.7}), st.target({"frac_up": 0.7}))
    (tmp_path / "bad.json").write_text("{\"columns\": [\"a\"]}")
    with pytest.raises(ValueError, match="cond_stats"):
        lb.LabelStats.load(str(tmp_path / "bad.json"))
    with pytest.raises(ValueError, match="cond_stats"):
        lb.LabelStats.load(str(tmp_path / "missing.json"))


def test_flag_refusals_before_any_gpu_work(tmp_path, monkeypatch):
    """Every refusal of the command line is raised by train() before a model, an object or a handle is built (this test has no GPU)."""
    a = parse([])
    assert a.label_out is None and a.label_layout == "mean" and a.label_rollout == 0 and a.cond_stats is None and a.cond_target is None
    st = lb.LabelStats(lb.TALLY_COLUMNS, "mean", [1, 2], {"G": 9, "P": 3}).fit(np.random.RandomState(6).uniform(0, 1, (5, 10)))
    stats = str(tmp_path / "rows.json")
    st.save(stats)
    rows = str(tmp_path / "rows.npy")
    np.save(rows, np.zeros((8, 10), dtype=np.float32))

    def refused(flags, match):
        with pytest.raises(ValueError, match=match):
            gtrain.train(parse(flags.split() + ["--num_fingers=8", "--batch_size=4"]))
    refused("--mode=test --cond_target frac_up=0.7", "needs --cond_stats")
    refused(f"--mode=test --cond_stats {stats}", "needs --cond_target")
    refused(f"--mode=test --cond_stats {stats} --cond_target frac_up=0.7 --global_cond {rows}", "--global_cond")
    refused(f"--mode=test --cond_stats {stats} --cond_target frac_sideways=0.7", "unknown column 'frac_sideways'")
    refused(f"--mode=test --cond_stats {stats} --cond_target rotate=0.7", "frac_clockwise and frac_counterclockwise")
    refused(f"--mode=test --cond_stats {stats} --cond_target convergence=0.7", "settle_concentration")
    refused(f"--mode=test --cond_stats {stats} --cond_target frac_up", "NAME=NUMBER")
    refused(f"--mode=test --cond_stats {tmp_path / 'none.json'} --cond_target frac_up=0.7", "cannot read")
    refused(f"--mode=train --cond_stats {stats} --cond_target frac_up=0.7", "--mode=test")
    refused(f"--mode=test --classifier_guidance --grid_size=8 --num_pos=3 --cond_stats {stats} --cond_target frac_up=0.7", "9 x 3\\^2 grid")
    refused(f"--mode=test --classifier_guidance --grid_size=9 --num_pos=5 --cond_stats {stats} --cond_target frac_up=0.7", "9 x 3\\^2 grid")
    refused("--mode=label --classifier_guidance", "--label_out")
    refused(f"--mode=label --label_out {rows}", "--classifier_guidance")
    refused(f"--mode=label --classifier_guidance --label_out {rows} --label_layout median", "label_layout")
    refused(f"--mode=label --classifier_guidance --label_out {rows} --label_rollout=-1", "label_rollout")
    refused(f"--mode=label --classifier_guidance --label_out {rows} --global_cond {rows}", "--global_cond")
    refused(f"--mode=test --label_out {rows}", "--mode=label")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    refused(f"--mode=label --classifier_guidance --label_out {rows}", "one process")
    # --cfg_weight is the target's to use: with --cond_target it needs no --global_cond
    monkeypatch.delenv("WORLD_SIZE")
    gtrain.check_cond_flags(parse(["--cond_target", "frac_up=0.7", "--cfg_weight", "2"]))
