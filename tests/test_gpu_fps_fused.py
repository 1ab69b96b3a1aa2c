"""The fused FPS table launch (pointnet.hip fps_table_kernel, one pass of 512 iterations per start that also writes sa2's 128-table):
the 128-table is the first 128 columns of the 512-table for every start index.  The values themselves and the tie flags are held to the
reference by tests/test_gpu_indices.py; here the clouds of that file plus one with exact duplicate points."""
import numpy as np
import pytest
import torch

from dgdm_amd import engine, synth
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dgdm_amd import _lib
    _lib.device_init(0)
    return torch.device("cuda:0")


def _clouds():
    g = util.load("g4_pointnet.npz")
    out = [torch.from_numpy(g["clouds"][ci]) for ci in range(g["clouds"].shape[0])]
    dup = synth.synth_object_3d(32).clone()
    dup[9] = dup[400]
    dup[10] = dup[400]
    out += [synth.synth_object_3d(31), dup, synth.synth_object_3d(8)]
    eight = synth.synth_object_3d(5).clone()          # 64 distinct coordinates, each eight times: used up at iteration 63 of every start
    eight[64:] = eight[:64].repeat(7, 1)
    out.append(eight)
    return out


def test_fps128_is_prefix_of_fps512(dev):
    dyn = engine.Dynamics(3, util.dyn3d_sd(33), 42)
    clouds = _clouds()
    for i, cloud in enumerate(clouds):
        idx = engine.debug_pointnet_indices(dyn, cloud.to(dev))
        n = cloud.shape[0]
        assert idx["fps512"].shape == (n, 512) and idx["fps128"].shape == (n, 128)
        assert np.array_equal(idx["fps128"], idx["fps512"][:, :128]), i
        assert np.array_equal(idx["fps512"][:, 0], np.arange(n)), i            # a sequence begins at its start index
        assert set(np.unique(idx["fps128_flags"])) <= {0, 1}, i
        if i == len(clouds) - 1:
            # all distances are 0 from iteration 63 on: inside the 128-sequence's tie tests (0..126), so every start is flagged, and the
            # sequence goes on with point 0 as the reference's argmax does
            assert idx["fps128_flags"].all()
            assert (idx["fps512"][:, 64:] == 0).all()
