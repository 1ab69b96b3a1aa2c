"""Data generation for the 3-D dynamics model (reference: sim/sim_3d.py) with the sliced squeeze in MuJoCo's place.

``generate`` writes one ``<object>_<gripper>.npz`` per pair in the reference's format (sim/sim_3d.py:162-172: ``np.savez_compressed(path,
dict)`` with the keys and order below) on its 360 x 5 x 5 pose grid, so that ``python dynamics/main.py --fingers_3d`` trains on data made
here:

    ctrlpts [42, 3], allpts [1250, 3], object_name str, obj_pos [9000, 3], obj_theta [9000] float32,
    delta_theta [9000] float32 (folded as continuous_signed_delta), delta_pos [9000, 3]

Poses run rotation-major, then x, then y.  The motion is ONE closing of the sliced squeeze (sim/squeeze.py, DESIGN.md §4.1d "3-D form"): a
frictionless, quasi-static idealisation that compares object and jaws on the finger grid's 25 horizontal planes only - not MuJoCo's
scene.  The object neither tilts nor lifts (delta_pos z = 0; the reference drops poses whose object fell over, this model has none).
``stats.json`` beside the files holds the configuration and the standard deviations of the three deltas for ``dynamics/main.py
--score_stats``.  The dataset reads the object's cloud from ``<object_mesh_dir>/<object_name>/model.obj``.
"""
from __future__ import annotations

import os
import sys
from typing import List, Sequence

import numpy as np

from .sim_2d import cli_config, cli_parser, pose_grid, record, write_map
from .squeeze import FINGER_WIDTH_3D

NUM_CTRL, SAMPLE_SIZE = 21, 25                          # sim/sim_3d.py:73-83


def gripper_design(gripper_idx: int):
    """(yl, yr) of gripper `gripper_idx`, in metres (prepare_gripper, sim/sim_3d.py:73-75)."""
    rs = np.random.RandomState(int(gripper_idx))
    yl = rs.uniform(-0.1, 0, size=(NUM_CTRL))
    yr = rs.uniform(-0.1, 0, size=(NUM_CTRL))
    return yl, yr


def generate(out_dir: str, gripper_ids: Sequence[int], meshes, object_ids: Sequence[int], object_names: Sequence[str], friction=None,
             friction_3d=None, **config) -> List[str]:
    """Writes ``<out_dir>/<object>_<gripper>.npz`` for every (gripper, object) and ``<out_dir>/stats.json``; returns the data files.
    meshes: (vertices (nv, 3) in metres, triangles (nt, 3)) per object, object_ids / object_names their numbers and names.  config: the
    squeeze model's (engine.SQUEEZE_DEFAULTS).  One device call for all pairs.  The 2-D ``friction`` argument is refused
    (squeeze.FRICTION_2D_ONLY).  friction_3d: the Coulomb coefficient of the 3-D antipodal jamming rule (squeeze.squeeze_map_3d; this
    project's own model, untuned, nothing claimed about MuJoCo); None: frictionless, today's files; when given, stats.json records it as
    ``"friction_3d"``."""
    from .. import engine
    from ..assets import finger_3d
    from . import squeeze
    if friction is not None:
        raise ValueError(f"sim_3d.generate: {squeeze.FRICTION_2D_ONLY}")
    fmu = None if friction_3d is None else squeeze.check_friction(friction_3d, "sim_3d.generate: friction_3d")
    meshes = list(meshes)
    if not (len(meshes) == len(object_ids) == len(object_names)):
        raise ValueError(f"generate: {len(meshes)} meshes for {len(object_ids)} object ids and {len(object_names)} names")
    designs = [gripper_design(g) for g in gripper_ids]
    shapes = [finger_3d.generate_3d_gripper(yl, yr, sample_size=SAMPLE_SIZE) for yl, yr in designs]
    samples = np.stack([np.concatenate([yl, yr]) for yl, yr in designs]).astype(np.float32)
    starts = pose_grid()
    extra = {} if fmu is None else {"friction_3d": fmu}
    out = squeeze.squeeze_map_3d(samples, meshes, starts, sample_size=SAMPLE_SIZE, width=FINGER_WIDTH_3D, scale=1.0, offset=0.0, **extra, **config)
    return write_map(out_dir, out, gripper_ids, object_ids, lambda f, o, start, closed: pair_record(*shapes[f], object_names[o], starts, start, closed),
                     engine.squeeze_config(**config), friction_3d=fmu)


def pair_record(ctrlpts, allpts, object_name, starts, start, closed) -> dict:
    """sim_2d.record of a 3-D pair: the object is its name, ``object_name`` (sim/sim_3d.py:162-170)."""
    return record(ctrlpts, allpts, "object_name", str(object_name), starts, start, closed)


def object_names_in(object_dir: str, names_file: str = "") -> List[str]:
    """The objects of a directory of ``<name>/model.obj``: the names listed in `names_file`, one per line, or every sub-directory that
    holds a mesh - numbered ones (the reference's MODEL_ROOT/objects/<idx>) in numeric order, then the rest by name."""
    from ..dynamics.utils import MESH_FILE
    if names_file:
        with open(names_file) as fh:
            return [line.strip() for line in fh if line.strip()]
    names = [n for n in os.listdir(object_dir) if os.path.isfile(os.path.join(object_dir, n, MESH_FILE))]
    return sorted(names, key=lambda n: (0, int(n), "") if n.isdigit() else (1, 0, n))


def main(argv=None):
    """python sim/sim_3d.py MODEL_ROOT GRIPPER_IDX OBJECT_IDX NUM_GRIPPERS NUM_OBJECTS SAVE_DIR NUM_CPUS: the reference's positional arguments
    (sim/sim_3d.py:174-181; NUM_CPUS is accepted and unused - no Ray).  The objects are ``<object_dir>/<name>/model.obj``; --object_dir
    defaults to MODEL_ROOT/objects, where the reference's prepare_object copies them; OBJECT_IDX counts through --object_names (a file
    of names, one per line) or the directory's listing."""
    p = cli_parser(main.__doc__)
    p.add_argument("--object_dir", default=None, help="directory of <name>/model.obj (default: MODEL_ROOT/objects)")
    p.add_argument("--object_names", default="", help="file of object names, one per line (default: the directory's listing)")
    p.add_argument("--friction", type=float, default=None, help="refused: friction is 2-D only (sim_2d.py --friction)")
    p.add_argument("--friction_3d", type=float, default=None,
                   help="the Coulomb coefficient of the 3-D antipodal jamming rule (DESIGN.md 4.1d '3-D friction'): poses whose two contacts hold the "
                        "object are jammed and stay where they are; this project's own model, untuned, nothing claimed about MuJoCo (default: "
                        "none, the frictionless model)")
    a = p.parse_args(argv)
    if a.friction is not None:
        from .squeeze import FRICTION_2D_ONLY
        raise ValueError(f"sim_3d --friction: {FRICTION_2D_ONLY}")
    if a.friction_3d is not None:
        from .squeeze import check_friction
        check_friction(a.friction_3d, "--friction_3d")
    from .. import _lib, engine
    from ..dynamics.utils import MESH_FILE
    _lib.device_init(0)
    object_dir = a.object_dir or os.path.join(a.model_root, "objects")
    if not os.path.isdir(object_dir):
        raise ValueError(f"sim_3d: no object directory at {object_dir} (--object_dir)")
    names = object_names_in(object_dir, a.object_names)
    object_ids = list(range(a.object_idx, a.object_idx + a.num_object_parallel))
    if not names or object_ids[-1] >= len(names):
        raise ValueError(f"sim_3d: objects {object_ids[0]} .. {object_ids[-1]} asked for, {len(names)} found under {object_dir}")
    meshes = [engine.read_obj(os.path.join(object_dir, names[i], MESH_FILE)) for i in object_ids]
    files = generate(a.save_dir, list(range(a.gripper_idx, a.gripper_idx + a.num_gripper_parallel)), meshes, object_ids, [names[i] for i in object_ids],
                     friction_3d=a.friction_3d, **cli_config(a))
    print(f"[dgdm_amd] wrote {len(files)} files and stats.json to {a.save_dir}")


if __name__ == "__main__":
    main(sys.argv[1:])
