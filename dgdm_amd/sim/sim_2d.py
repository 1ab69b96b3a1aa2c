"""Data generation for the 2-D dynamics model (reference: sim/sim_2d.py) with the squeeze simulator in MuJoCo's place.

``generate`` writes one ``<object>_<gripper>.npz`` per pair in the reference's format (sim/sim_2d.py:139-182: ``np.savez_compressed(path,
dict)`` with the keys and order below) on its 360 x 5 x 5 pose grid, so that ``python dynamics/main.py`` trains on data made here:

    ctrlpts [14, 2], allpts [400, 2], object_vertices [nv, 2], obj_pos [9000, 3], obj_theta [9000] float32,
    delta_theta [9000] float32 (folded as continuous_signed_delta), delta_pos [9000, 3]

Poses run theta-major, then x, then y.  The motion is ONE closing of the squeeze model (sim/squeeze.py): a frictionless,
quasi-static idealisation, not MuJoCo's scene - its deltas are multiples of the table's cell sizes in theta and x and differ in scale
from the reference's data.  ``stats.json`` beside the files holds the configuration and the standard deviations of the three deltas;
``generate(..., friction=mu)`` / ``--friction MU`` squeezes with Coulomb friction (sim/squeeze.py: jammed poses stay where they are;
this model's own rule, 2-D only); stats.json records ``"friction"``.  ``dynamics/main.py --score_stats stats.json`` normalises with them (with the MuJoCo constants of dynamics/dataloader.py the squeeze
deltas are merely scaled oddly).  The class thresholds and the generator's ``Diffusion.std`` are not retuned here.
"""
from __future__ import annotations

import json
import os
import sys
from typing import List, Sequence

import numpy as np

from .squeeze import SIMULATED, fold

NUM_ROT, NUM_POS, POS_HALF = 360, 5, 0.03              # sim/sim_2d.py:139-141
NUM_CTRL, NUM_POINTS = 7, 200                           # :75-86


def pose_grid() -> np.ndarray:
    """(9000, 3) start poses (theta, x, y), theta-major, then x, then y (sim/sim_2d.py:139-146, 176-177)."""
    z_rots = np.arange(0.0, 2 * np.pi, 2 * np.pi / NUM_ROT)
    locs = -POS_HALF + 2 * POS_HALF * np.arange(NUM_POS) / (NUM_POS - 1)
    th, x, y = np.meshgrid(z_rots, locs, locs, indexing='ij')
    return np.stack([th.reshape(-1), x.reshape(-1), y.reshape(-1)], axis=1)


def gripper_design(gripper_idx: int):
    """(x, yl, yr) of gripper `gripper_idx`, in metres (prepare_gripper, sim/sim_2d.py:73-77)."""
    rs = np.random.RandomState(int(gripper_idx))
    x = np.linspace(-0.12, 0.12, NUM_CTRL)
    yl = rs.uniform(-0.045, 0.015, size=(NUM_CTRL))
    yr = rs.uniform(-0.045, 0.015, size=(NUM_CTRL))
    return x, yl, yr


def generate(out_dir: str, gripper_ids: Sequence[int], contours, object_ids: Sequence[int], friction: float = 0.0, **config) -> List[str]:
    """Writes ``<out_dir>/<object>_<gripper>.npz`` for every (gripper, object) and ``<out_dir>/stats.json``; returns the data files.
    contours (O, nv, 2): the objects' contours in metres (extract_contours' output), object_ids their names.  config: the squeeze
    model's (engine.SQUEEZE_DEFAULTS); friction: its Coulomb coefficient (0: frictionless), recorded in stats.json.  One device call for
    all pairs."""
    from .. import engine
    from ..assets import finger_sampler
    from . import squeeze
    friction = squeeze.check_friction(friction, "generate")
    contours = np.asarray(contours, dtype=np.float64)
    if contours.ndim != 3 or contours.shape[2] != 2 or len(contours) != len(object_ids):
        raise ValueError(f"generate: contours of shape {contours.shape} for {len(object_ids)} objects (need (O, nv, 2))")
    designs = [gripper_design(g) for g in gripper_ids]
    shapes = [finger_sampler.generate_gripper(x, yl, yr, NUM_POINTS) for x, yl, yr in designs]
    samples = np.stack([np.concatenate([yl, yr]) for _, yl, yr in designs]).astype(np.float32)
    starts = pose_grid()
    out = squeeze.squeeze_map(samples, contours, starts, scale=1.0, offset=0.0, num_points=NUM_POINTS, friction=friction, **config)
    return write_map(out_dir, out, gripper_ids, object_ids, lambda f, o, start, closed: pair_record(*shapes[f], contours[o], starts, start, closed),
                     engine.squeeze_config(**config), friction)


def record(ctrlpts, allpts, object_key: str, object_value, starts, start, closed) -> dict:
    """The dict of one data file, keys in the reference's order (sim/sim_2d.py:172-180, sim/sim_3d.py:162-170), the object under
    `object_key`.  starts (n, 3): the start poses; start (n, 2): the (theta, x) of the cells they snapped to; closed (n, 3): the pose after
    one closing.  Host code."""
    starts, start, closed = (np.asarray(a, dtype=np.float64) for a in (starts, start, closed))
    zeros = np.zeros(len(starts))
    return {
        "ctrlpts": ctrlpts,
        "allpts": allpts,
        object_key: object_value,
        "obj_pos": np.stack([starts[:, 1], starts[:, 2], zeros], axis=1),
        "obj_theta": starts[:, 0].astype(np.float32),
        "delta_theta": fold(closed[:, 0] - start[:, 0], 2.0 * np.pi).astype(np.float32),
        "delta_pos": np.stack([closed[:, 1] - start[:, 1], closed[:, 2] - starts[:, 2], zeros], axis=1),
    }


def pair_record(ctrlpts, allpts, contour, starts, start, closed) -> dict:
    """`record` of a 2-D pair: the object is its contour, ``object_vertices``."""
    return record(ctrlpts, allpts, "object_vertices", np.asarray(contour, dtype=np.float64), starts, start, closed)


def write_map(out_dir: str, out, gripper_ids: Sequence[int], object_ids: Sequence[int], record_of, cfg, friction=None, friction_3d=None) -> List[str]:
    """write_dataset of a squeeze map's pairs: record_of(finger, object, start, closed) is the pair's data file; the loose starts are
    counted from the flags."""
    start, closed = out["start"].cpu().numpy(), out["closed"].cpu().numpy()
    records = [(int(object_ids[o]), int(gripper_ids[f]), record_of(f, o, start[p], closed[p])) for p, (f, o) in enumerate(out["pairs"])]
    return write_dataset(out_dir, records, cfg, int(np.count_nonzero(out["flags"].cpu().numpy() & 1)), friction, friction_3d)


def write_dataset(out_dir: str, records, cfg, loose_starts: int = 0, friction=None, friction_3d=None) -> List[str]:
    """records: (object_id, gripper_id, pair_record) per pair -> the data files and stats.json (the configuration and the standard
    deviations of delta_theta, delta_pos x and delta_pos y over all files: DynamicsDataset's score_std; "friction": the squeeze's Coulomb
    coefficient, when one is given; "friction_3d": the 3-D fingers' rule's, likewise).  Host code."""
    os.makedirs(out_dir, exist_ok=True)
    files, deltas = [], []
    for object_id, gripper_id, save_data in records:
        path = os.path.join(out_dir, "%d_%d.npz" % (object_id, gripper_id))
        np.savez_compressed(path, save_data)
        files.append(path)
        deltas.append(np.stack([save_data["delta_theta"].astype(np.float64), save_data["delta_pos"][:, 0], save_data["delta_pos"][:, 1]], axis=1))
    stats = {"simulated": SIMULATED, "config": {k: getattr(cfg, k) for k, _ in cfg._fields_}, "num_files": len(files),
             "gripper_ids": sorted({g for _, g, _ in records}), "object_ids": sorted({o for o, _, _ in records}),
             "loose_starts": int(loose_starts), "score_std": np.concatenate(deltas).std(axis=0).tolist()}
    if friction is not None:
        stats["friction"] = float(friction)
    if friction_3d is not None:
        stats["friction_3d"] = float(friction_3d)
    with open(os.path.join(out_dir, "stats.json"), "w") as fh:
        json.dump(stats, fh, indent=1)
    return files


def cli_parser(description: str):
    """The parser sim_2d.py and sim_3d.py start from: the reference's seven positional arguments and the squeeze model's two flags."""
    import argparse
    p = argparse.ArgumentParser(description=description)
    for name, kind in (("model_root", str), ("gripper_idx", int), ("object_idx", int), ("num_gripper_parallel", int), ("num_object_parallel", int),
                       ("save_dir", str), ("num_cpus", int)):
        p.add_argument(name, type=kind)
    p.add_argument("--squeeze_closing_steps", type=int, default=None)
    p.add_argument("--squeeze_window", type=int, default=None)
    return p


def cli_config(a) -> dict:
    """generate's config keys from cli_parser's two squeeze flags: those that were given."""
    return {k: v for k, v in (("closing_steps", a.squeeze_closing_steps), ("window", a.squeeze_window)) if v is not None}


def main(argv=None):
    """python sim/sim_2d.py MODEL_ROOT GRIPPER_IDX OBJECT_IDX NUM_GRIPPERS NUM_OBJECTS SAVE_DIR NUM_CPUS --object_dir Icons-50.npy: the
    reference's positional arguments (sim/sim_2d.py:184-191; MODEL_ROOT and NUM_CPUS are accepted and unused - no scene files, no Ray),
    plus the icon file, which the reference keeps in a constant."""
    p = cli_parser(main.__doc__)
    p.add_argument("--object_dir", required=True, help="the Icons-50 .npy file")
    p.add_argument("--friction", type=float, default=0.0, help="Coulomb friction coefficient of the squeeze (default 0: frictionless)")
    a = p.parse_args(argv)
    from .squeeze import check_friction
    check_friction(a.friction, "--friction")
    from .. import _lib
    from ..assets import icon_process
    _lib.device_init(0)
    object_ids = list(range(a.object_idx, a.object_idx + a.num_object_parallel))
    images = np.load(a.object_dir, allow_pickle=True).item()['image'][object_ids].transpose((0, 2, 3, 1))
    contours = icon_process.extract_contours_batch(images)
    files = generate(a.save_dir, list(range(a.gripper_idx, a.gripper_idx + a.num_gripper_parallel)), contours, object_ids, friction=a.friction,
                     **cli_config(a))
    print(f"[dgdm_amd] wrote {len(files)} files and stats.json to {a.save_dir}")


if __name__ == "__main__":
    main(sys.argv[1:])
