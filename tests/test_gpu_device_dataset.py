"""Training from a device-resident dataset on the GPU (csrc/dataset.hip through dgdm_amd/dynamics/device_dataset.py): the rows the
store writes against main.batch_rows of the collated batch (bit-equal), the agreement counts against numpy (equal integers), and the
driver with --device_dataset against the driver without it (same log, same checkpoint)."""
import glob
import os

import numpy as np
import pytest
import torch
from torch.utils.data import default_collate

from tests import util

pytestmark = pytest.mark.gpu


def _dataset(root, **kw):
    from dynamics.dataloader import DynamicsDataset
    return DynamicsDataset(str(root), **kw)


def _check_rows(ds, store, ids, fingers_3d=False):
    from dgdm_amd.dynamics.main import batch_rows
    want = batch_rows(default_collate([ds[i] for i in ids]), fingers_3d)
    got = store.batch_rows(ids)
    torch.cuda.synchronize()
    for name, w, g in zip(("ctrl", "score", "ori", "pos", "obj"), want, got):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w.shape, (name, g.shape, w.shape)
        assert torch.equal(g.cpu().view(torch.int32), w.contiguous().view(torch.int32)), name        # bit for bit (-0.0 and NaN included)


@pytest.mark.parametrize("max_vertices", [5, 100])
def test_rows_2d(tmp_path, max_vertices):
    """Row width 10 (no multiple of four: the groups of four straddle rows and samples) and 200 with 14 control ordinates; repeated and
    unordered ids, a single sample."""
    from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore
    util.write_synth_dataset(str(tmp_path), 4, n_files=5, cells=5, n_ctrl=14, n_verts=(5, 7, 4) if max_vertices == 100 else (5, 4, 3))
    ds = _dataset(tmp_path, object_max_num_vertices=max_vertices)
    store = DeviceDynamicsStore(ds, threads=3, batch_size=4)
    assert len(store) == 5 and store.cells == 5 and store.n_objects == 5
    assert store.nbytes == 4 * 5 * (14 * 2 + 2 * max_vertices + 5 * 6)
    for ids in ([3, 0, 3, 4], [2], torch.tensor([4, 4, 1])):
        _check_rows(ds, store, ids)


def test_rows_2d_issue_vertices(tmp_path):
    """The issue's first case as written: contours of 5, 7 and 4 vertices cannot be padded to 5, and the dataset says so itself; with a
    store over the files that fit (5 and 4 vertices) the rows are those of the host path."""
    from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore
    util.write_synth_dataset(str(tmp_path), 4, n_files=5, cells=5, n_verts=(5, 7, 4))
    ds = _dataset(tmp_path, object_max_num_vertices=5)
    with pytest.raises(Exception):
        ds[1]
    ds.data_files = [f for i, f in enumerate(ds.data_files) if i % 3 != 1]
    store = DeviceDynamicsStore(ds)
    _check_rows(ds, store, [2, 0, 2])


def test_rows_2d_across_workgroups(tmp_path):
    """nb = 4, cells = 700: 2800 rows; every output but ori spans several workgroups, and the 10-wide object rows start off a 16-byte
    boundary in every other sample."""
    from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore
    util.write_synth_dataset(str(tmp_path), 6, n_files=4, cells=700, n_ctrl=9, n_verts=(5, 3))
    ds = _dataset(tmp_path, object_max_num_vertices=5)
    _check_rows(ds, DeviceDynamicsStore(ds), [1, 3, 0, 1])


def _write_3d(root, n_files, cells, n_ctrl, N, names):
    util.write_synth_dataset(str(root), 8, n_files=n_files, cells=cells, n_ctrl=n_ctrl)
    rs = np.random.RandomState(9)
    clouds = {n: rs.uniform([-0.1, -0.1, 0.0], [0.1, 0.1, 0.12], (N + 2, 3)) for n in sorted(set(names))}
    for f, name in zip(sorted(glob.glob(os.path.join(str(root), "*.npz"))), names):
        d = np.load(f, allow_pickle=True)["arr_0"].item()
        d["ctrlpts"] = np.concatenate([d["ctrlpts"], rs.uniform(0.0, 0.12, (n_ctrl, 1))], axis=1)
        d["object_name"], d["object_points"] = name, clouds[name]
        del d["object_vertices"]
        np.savez(f, d)


def test_rows_3d(tmp_path):
    """The driver's 3-D ordering: control points and clouds cell-major (row = cell * samples + sample), scores and poses sample-major.
    Two files share an object name: the store holds that cloud once."""
    from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore
    _write_3d(tmp_path, 4, 5, 6, 8, ["mug", "bowl", "mug", "can"])
    ds = _dataset(tmp_path, object_max_num_vertices=8, fingers_3d=True)
    store = DeviceDynamicsStore(ds, threads=2)
    assert store.fingers_3d and store.n_objects == 3 and sorted(store.object_names) == ["bowl", "can", "mug"]
    assert tuple(store.objects.shape) == (3, 8, 3) and tuple(store.ctrl.shape) == (4, 6, 3)
    for ids in ([2, 1, 0], [3, 3, 2], [0]):
        _check_rows(ds, store, ids, fingers_3d=True)


def test_bad_ids_raise_and_launch_nothing(tmp_path):
    from dgdm_amd import _lib
    from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore
    util.write_synth_dataset(str(tmp_path), 4, n_files=3, cells=5)
    ds = _dataset(tmp_path, object_max_num_vertices=8)
    store = DeviceDynamicsStore(ds)
    for ids in ([-1], [0, len(store)], [1, -1, 2], []):
        with pytest.raises(_lib.DgdmError):
            store.batch_rows(ids)
    torch.cuda.synchronize()
    _check_rows(ds, store, [2, 0])


THR = np.array([0.03, 0.002, 0.003]) / np.array([0.0565, 0.0026, 0.0047])


def _agreement_case(rows):
    rs = np.random.RandomState(rows)
    t = THR.astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    out = []
    for _ in range(2):
        v = (rs.normal(0, 1, (rows, 3)) * t).astype(np.float32)
        pick = rs.randint(0, 12, (rows, 3))
        v = np.where(pick == 0, t, np.where(pick == 1, -t, np.where(pick == 2, np.nextafter(t, np.float32(np.inf)), v)))
        v = np.where((pick >= 3) & (pick < 8), special[np.clip(pick - 3, 0, 4)], v).astype(np.float32)
        out.append(v)
    return out


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 70001])
def test_agreement_counts(rows):
    """Values at exactly +-thr (middle class), +-inf and NaN (middle class, as in torch) in both tensors: the integer counts are numpy's
    and the accuracies are class_accuracy's Python floats."""
    from dgdm_amd.dynamics.device_dataset import class_accuracy_device, class_agreement
    from dgdm_amd.dynamics.main import class_accuracy
    s, p = _agreement_case(rows)
    t = THR.astype(np.float32)
    cls = lambda v: (v > t).astype(np.int64) - (v < -t).astype(np.int64)               # noqa: E731
    want = (cls(s) == cls(p)).sum(axis=0)
    if rows > 200:
        assert np.isnan(s).any() and np.isnan(p).any() and (s == t).any() and (p == -t).any() and np.isinf(s).any() and 0 < want.min() and want.max() < rows
    sd, pd = torch.from_numpy(s).cuda(), torch.from_numpy(p).cuda()
    got = class_agreement(sd, pd, THR)
    assert got.dtype == torch.int64 and got.cpu().tolist() == want.tolist()
    assert class_agreement(sd, pd, THR).cpu().tolist() == want.tolist()                  # overwritten, not accumulated
    assert class_accuracy_device(sd, pd, THR) == class_accuracy(torch.from_numpy(s), torch.from_numpy(p), THR)


def _driver_args(tmp_path, save, extra=()):
    from dgdm_amd.dynamics.parser import parse
    return parse([f"--save_dir={save}", "--ctrlpts_dim=14", "--batch_size=4", "--object_max_num_vertices=100", f"--data_dir={tmp_path / 'train'}",
                  f"--test_data_dir={tmp_path / 'val'}", "--learning_rate=1e-3", "--weight_decay=0", "--num_epochs=3", "--val_step=1",
                  "--save_ckpt_step=1000", "--patience=100", "--num_workers=0", "--num_train_timesteps=15", "--num_inference_steps=5",
                  "--num_timesteps_per_batch=1", *extra])


def _run_driver(tmp_path, name, extra=()):
    from dgdm_amd.dynamics import main
    save = tmp_path / name
    torch.manual_seed(7)
    trainer = main.train(_driver_args(tmp_path, save, extra))
    trainer._join_ahead()
    torch.cuda.synchronize()
    return open(save / "log.jsonl").read().splitlines(), torch.load(save / "best.pt", map_location="cpu")


def test_driver_with_device_dataset_is_the_host_driver(tmp_path):
    """12 training and 4 validation files of 48 cells, 3 epochs of batch_size 4, in process under torch.manual_seed(7): the host path
    twice (it must reproduce itself bit for bit, or the comparison below would mean nothing), then --device_dataset: log.jsonl equal
    line for line - every batch loss, accuracy and validation figure - and best.pt equal tensor for tensor.  --mode=validate returns the
    same tuple with and without the flag."""
    from dgdm_amd.dynamics import main
    util.write_synth_dataset(str(tmp_path / "train"), 21, n_files=12, cells=48)
    util.write_synth_dataset(str(tmp_path / "val"), 22, n_files=4, cells=48)
    log_a, ck_a = _run_driver(tmp_path, "host_a")
    log_b, ck_b = _run_driver(tmp_path, "host_b")
    assert len(log_a) == 3 * (3 + 1 + 1)
    assert log_a == log_b and all(torch.equal(ck_a[k], ck_b[k]) for k in ck_a), "the host path does not reproduce itself"
    log_d, ck_d = _run_driver(tmp_path, "device", ["--device_dataset"])
    assert log_d == log_a
    assert set(ck_d) == set(ck_a) and all(torch.equal(ck_a[k], ck_d[k]) for k in ck_a)
    ckpt = f"--checkpoint_path={tmp_path / 'host_a' / 'best.pt'}"
    vals = []
    for extra in ([], ["--device_dataset"]):
        torch.manual_seed(7)
        vals.append(main.train(_driver_args(tmp_path, tmp_path / "val_out", ["--mode=validate", ckpt, *extra])))
    assert len(vals[0]) == 4 and vals[0] == vals[1]
