"""Wall clock per step of the 2-D dynamics-training DRIVER (dgdm_amd/dynamics/main.py), host loop against --device_dataset, on an MI355X.

Writes a synthetic dataset in the simulator's format to a temporary directory (256 files x 9000 pose cells, 100 contour vertices,
compressed .npz), then runs the body of main.train's epoch loop - loader, rows, Trainer.step, class accuracy - with the flags of
dynamics/train_dynamics_2d.sh (batch_size 128 -> 1 152 000 rows per step): first the host loop (DataLoader over the files, main.batch_rows,
upload, CPU accuracy), then the device loop (DeviceDynamicsStore, rows and accuracy counts on the GPU), each `--steps` steps after
`--warmup` steps, a device synchronise on either side of the timed region.  Also reports the store's build time and what the CPU-generator
draws of one step cost on this host (they stay on the host in both loops: Trainer._draw makes them one step ahead on a worker thread).
One process; prints one JSON line last.

python scripts/bench_train_driver.py [--files 256] [--cells 9000] [--batch_size 128] [--steps 3] [--warmup 1] [--num_workers 8]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgdm_amd import _lib  # noqa: E402
from dgdm_amd.dynamics import main  # noqa: E402
from dgdm_amd.dynamics.dataloader import DynamicsDataset  # noqa: E402
from dgdm_amd.dynamics.device_dataset import DeviceDynamicsStore  # noqa: E402
from dgdm_amd.dynamics.parser import parse  # noqa: E402
from dgdm_amd.dynamics.trainer import Trainer  # noqa: E402


def write_dataset(root, files, cells, n_vertices, seed=0):
    rs = np.random.RandomState(seed)
    for i in range(files):
        d = {"ctrlpts": np.stack([np.linspace(-0.12, 0.12, 14), rs.uniform(-0.045, 0.015, 14)], 1),
             "delta_theta": rs.normal(0, 0.05, cells), "delta_pos": rs.normal(0, 0.003, (cells, 2)),
             "obj_theta": rs.uniform(0, 2 * np.pi, cells), "obj_pos": rs.uniform(-0.03, 0.03, (cells, 3)),
             "object_vertices": rs.uniform(-0.05, 0.05, (n_vertices, 2))}
        np.savez_compressed(os.path.join(root, "sample_%04d.npz" % i), d)


def run_loop(args, trainer, loader, store, threshold_std, warmup, steps):
    """main.train's loop body; returns (seconds per timed step, last loss)."""
    done, t0, loss = 0, None, float("nan")
    while True:
        for (ctrl, score, ori, pos, obj), cells in main._row_batches(args, loader, store):
            if done == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            loss, pred = trainer.step(ctrl, score, ori, pos, obj, rows_per_sample=cells)
            main._accuracy(score, pred, threshold_std)
            done += 1
            if done == warmup + steps:
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps, loss


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--cells", type=int, default=9000)
    ap.add_argument("--vertices", type=int, default=100)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--num_workers", type=int, default=8)
    ap.add_argument("--skip_host", action="store_true", help="time the device loop only")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 1:
        ap.error("--steps and --warmup must be at least 1")
    _lib.device_init(0)
    out = {"metric": "train_driver_2d_seconds_per_step", "files": a.files, "cells": a.cells, "batch_size": a.batch_size,
           "rows_per_step": a.batch_size * a.cells, "steps": a.steps, "warmup": a.warmup, "num_workers": a.num_workers,
           "torch_threads": torch.get_num_threads()}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_dataset(root, a.files, a.cells, a.vertices)
        out["write_dataset_s"] = round(time.perf_counter() - t0, 3)
        # the flags of dynamics/train_dynamics_2d.sh
        args = parse(["--ctrlpts_dim=14", f"--batch_size={a.batch_size}", f"--object_max_num_vertices={a.vertices}", f"--data_dir={root}",
                      "--learning_rate=1e-4", "--weight_decay=0", "--num_epochs=100", f"--num_workers={a.num_workers}", "--num_train_timesteps=15",
                      "--num_inference_steps=5", "--num_timesteps_per_batch=1"])
        ds = DynamicsDataset(root, object_max_num_vertices=a.vertices)
        threshold_std = ds.threshold / ds.std
        rows = a.batch_size * a.cells

        t0 = time.perf_counter()
        for _ in range(3):
            torch.randn((rows, args.ctrlpts_dim))
            torch.randint(0, args.num_train_timesteps, (rows,)).long()
        out["cpu_draws_ms_per_step"] = round((time.perf_counter() - t0) / 3 * 1e3, 1)

        def fresh_trainer():
            torch.manual_seed(0)
            t = Trainer(args)
            t.create_model()
            return t

        if not a.skip_host:
            trainer = fresh_trainer()
            loader = DataLoader(ds, batch_size=a.batch_size, shuffle=True, num_workers=a.num_workers, drop_last=False)
            sec, loss = run_loop(args, trainer, loader, None, threshold_std, a.warmup, a.steps)
            trainer._join_ahead()
            out["host_loop_ms_per_step"], out["host_loop_last_loss"] = round(sec * 1e3, 1), loss
            del trainer, loader
            print(json.dumps(out), flush=True)

        trainer = fresh_trainer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = DeviceDynamicsStore(ds, threads=max(a.num_workers, 1), batch_size=a.batch_size)
        torch.cuda.synchronize()
        out["store_build_s"], out["store_gib"] = round(time.perf_counter() - t0, 3), round(store.nbytes / 2 ** 30, 3)
        loader = store.index_loader(a.batch_size, shuffle=True)
        sec, loss = run_loop(args, trainer, loader, store, threshold_std, a.warmup, a.steps)
        out["device_loop_ms_per_step"], out["device_loop_last_loss"] = round(sec * 1e3, 1), loss
        # the parts of a device-loop step, each alone
        ids = list(range(a.batch_size))
        store.batch_rows(ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            r = store.batch_rows(ids)
        torch.cuda.synchronize()
        out["batch_rows_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        pred = torch.zeros_like(r[1])
        t0 = time.perf_counter()
        for _ in range(5):
            main._accuracy(r[1], pred, threshold_std)
        out["device_accuracy_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        trainer._join_ahead()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main_()
