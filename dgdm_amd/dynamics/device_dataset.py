"""Training and validation of the dynamics model from a device-resident dataset (``python dynamics/main.py --device_dataset``).

The host loop of dynamics/main.py re-reads ``batch_size`` files for every step, replicates each sample's control ordinates and object over
its pose cells in host memory and uploads about 1 GB of rows per 1.15 M-row step.  A sample is 216 KB of grid plus a few hundred bytes,
so a whole dataset fits in HBM many times over: ``DeviceDynamicsStore`` reads every file ONCE (through ``dataset[i]``, so the values are the
host path's float32 values), keeps the samples as device arrays, and ``batch_rows`` writes a batch's row tensors on the GPU from a list
of sample indices (csrc/dataset.hip, one launch) - bit-equal to ``main.batch_rows`` of the collated batch.  ``class_accuracy_device``
counts the class agreements on the GPU, so that per step only the loss and three integers come back.  ``index_loader`` is the
DataLoader of the host loop over the indices alone: same batches, same use of the global CPU generator."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import _lib
from .._lib import check, dptr, lib, stream_ptr

MAX_THREADS = 16
_KEYS = ('ctrlpts', 'scores', 'input_ori', 'input_pos', 'object_vertices')


def _file_of(dataset, i: int) -> str:
    files = getattr(dataset, 'data_files', None)
    return str(files[i]) if files is not None else 'item %d' % i


class DeviceDynamicsStore:
    """Every sample of `dataset` on the device.  2-D: ctrl [S, L, 2], objects [S, V, 2] (one zero-padded contour per file).  3-D: ctrl
    [S, L, 3], objects [O, N, 3] - each distinct cloud once, keyed by the name the dataset caches it under - and the object of every sample.
    scores [S, cells, 3], ori [S, cells], pos [S, cells, 2].  batch_size: the largest batch `batch_rows` will be asked for, counted in
    the memory check."""

    def __init__(self, dataset, device=None, threads: int = 8, batch_size: int = 1):
        n = len(dataset)
        if n == 0:
            raise ValueError("DeviceDynamicsStore: the dataset has no samples")
        threads = max(1, min(int(threads), MAX_THREADS, n))
        with ThreadPoolExecutor(max_workers=threads) as ex:
            items = list(ex.map(dataset.__getitem__, range(n)))
        self.fingers_3d = bool(getattr(dataset, 'fingers_3d', items[0]['ctrlpts'].shape[-1] == 3))
        first = items[0]
        for i, it in enumerate(items):                                                    # all before any device allocation
            if it['scores'].shape[0] != first['scores'].shape[0]:
                raise ValueError(f"DeviceDynamicsStore: {_file_of(dataset, i)} has {it['scores'].shape[0]} pose cells, {_file_of(dataset, 0)} has "
                                 f"{first['scores'].shape[0]}: a device-resident dataset needs one grid size (use the host path)")
            if it['ctrlpts'].shape != first['ctrlpts'].shape:
                raise ValueError(f"DeviceDynamicsStore: {_file_of(dataset, i)} has control points of shape {tuple(it['ctrlpts'].shape)}, "
                                 f"{_file_of(dataset, 0)} of {tuple(first['ctrlpts'].shape)} (use the host path)")
            if it['object_vertices'].shape != first['object_vertices'].shape:
                raise ValueError(f"DeviceDynamicsStore: {_file_of(dataset, i)} has an object of shape {tuple(it['object_vertices'].shape)}, "
                                 f"{_file_of(dataset, 0)} of {tuple(first['object_vertices'].shape)} (use the host path)")
            if it['input_ori'].shape[0] != it['scores'].shape[0] or it['input_pos'].shape[0] != it['scores'].shape[0]:
                raise ValueError(f"DeviceDynamicsStore: {_file_of(dataset, i)}: poses and scores differ in length")
        width = 3 if self.fingers_3d else 2
        if first['ctrlpts'].shape[-1] != width or first['object_vertices'].shape[-1] != width:
            raise ValueError(f"DeviceDynamicsStore: control points {tuple(first['ctrlpts'].shape)} / object {tuple(first['object_vertices'].shape)} "
                             f"are not {width}-D")
        self.n_samples, self.cells = n, int(first['scores'].shape[0])
        self.n_ctrl, self.n_object_points = int(first['ctrlpts'].shape[0]), int(first['object_vertices'].shape[0])
        if self.fingers_3d:
            names = getattr(dataset, 'object_name_of', {})
            slot, objects, of_sample = {}, [], np.empty(n, dtype=np.int32)
            for i, it in enumerate(items):
                key = names[i] if i in names else ('#', it['object_vertices'].numpy().tobytes())
                if key not in slot:
                    slot[key] = len(objects)
                    objects.append(it['object_vertices'])
                of_sample[i] = slot[key]
            self.object_names = [k if isinstance(k, str) else None for k in slot]
            self._object_of_sample = np.ascontiguousarray(of_sample)
        else:
            objects, self.object_names, self._object_of_sample = [it['object_vertices'] for it in items], None, None
        self.n_objects = len(objects)
        host = {'ctrl': torch.stack([it['ctrlpts'] for it in items]), 'objects': torch.stack(objects),
                'scores': torch.stack([it['scores'] for it in items]), 'ori': torch.stack([it['input_ori'].reshape(-1) for it in items]),
                'pos': torch.stack([it['input_pos'] for it in items])}
        del items
        host = {k: v.to(torch.float32).contiguous() for k, v in host.items()}
        self.nbytes = int(sum(v.numel() * 4 for v in host.values()))
        # ------------------------------------------------------------ the device, from here on
        if not torch.cuda.is_available():
            raise RuntimeError("dgdm_amd runs on an MI355X through libdgdm_hip.so; no GPU is visible and there is no CPU path")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        need = self.nbytes + self.batch_nbytes(batch_size)
        free = torch.cuda.mem_get_info(self.device)[0] + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if need > free:
            raise RuntimeError(f"DeviceDynamicsStore: the dataset ({self.nbytes / 2 ** 30:.2f} GiB) and one batch of {batch_size} samples' rows "
                               f"({self.batch_nbytes(batch_size) / 2 ** 30:.2f} GiB) do not fit in the {free / 2 ** 30:.2f} GiB of free device memory: "
                               "train without --device_dataset (the host path streams the files)")
        self.ctrl, self.objects, self.scores, self.ori, self.pos = (host[k].to(self.device) for k in ('ctrl', 'objects', 'scores', 'ori', 'pos'))
        self._c = _lib.DynamicsStore(dptr(self.ctrl), dptr(self.objects), dptr(self.scores), dptr(self.ori), dptr(self.pos),
                                     None if self._object_of_sample is None else self._object_of_sample.ctypes.data,
                                     self.n_samples, self.n_objects, self.cells, self.n_ctrl, self.n_object_points, int(self.fingers_3d))

    def __len__(self) -> int:
        return self.n_samples

    def batch_nbytes(self, batch_size: int) -> int:
        """Bytes of the five row tensors of a batch of `batch_size` samples."""
        dims = 3 if self.fingers_3d else 2
        per_row = (dims if self.fingers_3d else 1) * self.n_ctrl + dims * self.n_object_points + 3 + 1 + 2
        return int(batch_size) * self.cells * per_row * 4

    def batch_rows(self, sample_ids: Sequence[int]):
        """(ctrl, score, ori, pos, obj) of main.batch_rows for the batch made of these samples, as device tensors."""
        ids = np.ascontiguousarray(torch.as_tensor(sample_ids).reshape(-1).numpy() if isinstance(sample_ids, torch.Tensor)
                                   else np.asarray(sample_ids).reshape(-1), dtype=np.int64)
        nb = int(ids.shape[0])
        rows, f = nb * self.cells, dict(dtype=torch.float32, device=self.device)
        if self.fingers_3d:
            ctrl, obj = torch.empty((rows, 3, self.n_ctrl), **f), torch.empty((rows, 3, self.n_object_points), **f)
        else:
            ctrl, obj = torch.empty((rows, self.n_ctrl), **f), torch.empty((rows, 2 * self.n_object_points), **f)
        score, ori, pos = torch.empty((rows, 3), **f), torch.empty((rows, 1), **f), torch.empty((rows, 2), **f)
        ids_dev = torch.empty(2 * max(nb, 1), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().dgdm_dynamics_batch_rows(C.byref(self._c), ids.ctypes.data, nb, dptr(ids_dev), dptr(ctrl), dptr(obj), dptr(score), dptr(ori),
                                                 dptr(pos), stream_ptr()))
        return ctrl, score, ori, pos, obj

    def index_loader(self, batch_size: int, shuffle: bool = False, drop_last: bool = False) -> DataLoader:
        return index_loader(self.n_samples, batch_size, shuffle, drop_last)


def index_loader(n_samples: int, batch_size: int, shuffle: bool = False, drop_last: bool = False) -> DataLoader:
    """The driver's DataLoader over the sample indices instead of the samples: the same batches in the same order, and the same draws
    from the global CPU generator (one base seed per iterator and one sampler seed per shuffled epoch - neither depends on what the
    dataset returns or on num_workers, as long as __getitem__ draws nothing, which DynamicsDataset's does not)."""
    return DataLoader(range(int(n_samples)), batch_size=batch_size, shuffle=shuffle, num_workers=0, drop_last=drop_last)


def class_agreement(score: torch.Tensor, pred: torch.Tensor, threshold_std) -> torch.Tensor:
    """int64 [3] on the device: per output, the rows whose three-way class agrees (dgdm_class_agreement)."""
    if score.shape != pred.shape or score.dim() != 2 or score.shape[1] != 3:
        raise ValueError(f"class_agreement: score {tuple(score.shape)} and pred {tuple(pred.shape)} must both be (rows, 3)")
    f = lambda t: t.detach().to(device=score.device, dtype=torch.float32).contiguous()       # noqa: E731
    score, pred = f(score), f(pred)
    thr = (C.c_float * 3)(*[float(v) for v in np.asarray(threshold_std, dtype=np.float32).reshape(3)])
    agree = torch.empty(3, dtype=torch.int64, device=score.device)
    with torch.cuda.device(score.device):
        check(lib().dgdm_class_agreement(dptr(score), dptr(pred), int(score.shape[0]), thr, dptr(agree), stream_ptr()))
    return agree


def class_accuracy_device(score: torch.Tensor, pred: torch.Tensor, threshold_std) -> List[float]:
    """main.class_accuracy from the device counts: count / rows in float32, which for rows <= 2**24 is the float32 mean of the 0 / 1
    agreements that the host path takes (every partial sum is an exact integer)."""
    rows = np.float32(score.shape[0])
    return [float(np.float32(c) / rows) for c in class_agreement(score, pred, threshold_std).cpu().tolist()]
