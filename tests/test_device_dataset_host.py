"""Host side of training from a device-resident dataset (dgdm_amd/dynamics/device_dataset.py, --device_dataset): CPU only."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

from tests import util


def test_flag_parses_and_defaults_to_off():
    from dgdm_amd.dynamics.parser import parse
    assert parse([]).device_dataset is False
    assert parse(["--device_dataset"]).device_dataset is True


class _Own(Dataset):
    """Returns its own index and draws nothing, like DynamicsDataset."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


@pytest.mark.parametrize("n,batch_size,shuffle,drop_last,workers", [(13, 4, True, False, 0), (13, 4, True, False, 2), (13, 4, False, False, 0),
                                                                     (13, 4, True, True, 0), (3, 8, True, False, 0)])
def test_index_loader_is_the_drivers_loader(n, batch_size, shuffle, drop_last, workers):
    """Same batches in the same order as the driver's DataLoader under a fixed seed, and the global CPU generator is left in the same
    state: the next torch.rand after two epochs is the same number."""
    from dgdm_amd.dynamics.device_dataset import index_loader
    torch.manual_seed(11)
    host = DataLoader(_Own(n), batch_size=batch_size, shuffle=shuffle, num_workers=workers, drop_last=drop_last)
    want = [[b.tolist() for b in host] for _ in range(2)]
    after = torch.rand(3)
    torch.manual_seed(11)
    mine = index_loader(n, batch_size, shuffle, drop_last)
    got = [[b.tolist() for b in mine] for _ in range(2)]
    assert got == want and len(mine) == len(host)
    assert torch.equal(torch.rand(3), after)
    assert all(b.dtype == torch.int64 for b in mine)
    if shuffle and n > 3:
        assert want[0] != want[1]                                                        # the epochs were reshuffled, so the seeds were drawn


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched before the dataset was validated")
    for name in ("is_available", "current_device", "mem_get_info", "memory_reserved", "memory_allocated"):
        monkeypatch.setattr(torch.cuda, name, boom)


def test_ragged_cells_raise_before_any_device_use(tmp_path, monkeypatch):
    from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore
    from dynamics.dataloader import DynamicsDataset
    util.write_synth_dataset(str(tmp_path / "a"), 1, n_files=2, cells=6)
    util.write_synth_dataset(str(tmp_path / "b"), 2, n_files=1, cells=7)
    ds = DynamicsDataset(str(tmp_path), object_max_num_vertices=8)
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=r"b.sample_00\.npz has 7 pose cells"):
        DeviceDynamicsStore(ds)


def test_differing_control_shapes_raise_before_any_device_use(tmp_path, monkeypatch):
    from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore
    from dynamics.dataloader import DynamicsDataset
    util.write_synth_dataset(str(tmp_path / "a"), 1, n_files=2, cells=6, n_ctrl=14)
    util.write_synth_dataset(str(tmp_path / "b"), 2, n_files=2, cells=6, n_ctrl=10)
    ds = DynamicsDataset(str(tmp_path), object_max_num_vertices=8)
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=r"b.sample_00\.npz has control points of shape \(10, 2\)"):
        DeviceDynamicsStore(ds, threads=3)


def test_accuracy_from_counts_is_the_host_accuracy():
    """count / rows in float32 == class_accuracy's float32 mean, as Python floats, for counts numpy makes on the CPU."""
    from dgdm_amd.dynamics.main import class_accuracy
    rs = np.random.RandomState(5)
    thr = np.array([0.03, 0.002, 0.003]) / np.array([0.0565, 0.0026, 0.0047])
    for rows in (1, 7, 255, 70001):
        s, p = rs.normal(0, 1, (rows, 3)).astype(np.float32), rs.normal(0, 1, (rows, 3)).astype(np.float32)
        t = thr.astype(np.float32)
        cls = lambda v: (v > t).astype(np.int64) - (v < -t).astype(np.int64)               # noqa: E731
        counts = (cls(s) == cls(p)).sum(axis=0)
        assert [float(np.float32(c) / np.float32(rows)) for c in counts] == class_accuracy(torch.from_numpy(s), torch.from_numpy(p), thr)
