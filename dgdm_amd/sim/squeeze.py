"""Squeeze simulator: a model-free 2-D closing simulator on the GPU (csrc/squeeze.hip, include/dgdm_hip.h "squeeze simulator",
DESIGN.md §4.1d) - a frictionless, quasi-static parallel-jaw squeeze of the object contour by the two decoded finger profiles.

It is this package's own idealisation and is NOT pinned to the reference's MuJoCo scene (assets/finger_sampler.py:154-177: friction 1.0,
soft position actuators; this model has neither).  What pins it are closed-form results of frictionless squeezing (the diameter function
of a rectangle between flat jaws, a disc in a V) and the float64 restatement tests/squeeze_oracle.py, which the device reproduces bit for
bit.  A jaw that touches alone is assumed to carry the object along y without turning it.  ``window`` and ``closing_steps`` are untuned.

Coulomb friction is an opt-in (``friction=mu``; include/dgdm_hip.h "squeeze simulator with Coulomb friction", DESIGN.md §4.1d "friction";
tests/squeeze_friction_oracle.py): a cell whose two contacts hold the object against any squeezing force (the two-contact antipodal
condition) is jammed and stays where it is; everything else moves as without friction - friction decides whether, not where, which is an
assumption of the model.  ``friction=0`` is the frictionless model, bit for bit.  2-D only.

* ``squeeze_map``        designs x contours -> closed and settled poses per start pose, on device tensors;
* ``SqueezeSimulator``   a callable with the ``sim_test_batch`` signature for ``Diffusion(simulator=...)``: the tables that
                         ``--predicted_sim`` fills with the dynamics model's opinion, filled by this model instead and marked
                         ``'simulated': 'squeeze'`` (never ``'predicted'``).

For 3-D fingers the same model runs sliced (DESIGN.md §4.1d "3-D form"; tests/squeeze3d_oracle.py): object meshes are cut on the finger
grid's horizontal planes and the 2-D contract applies on each plane; what lies between two planes is not seen, and the object neither
tilts nor lifts.

* ``finger_surfaces_3d`` designs -> the abscissae, the levels and the two jaw faces on them;
* ``squeeze_map_3d``     designs x meshes -> ``squeeze_map``'s outputs;
* ``SqueezeSimulator3D`` the callable with the ``sim_test_batch_3d`` signature (``--squeeze_sim_3d``).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..dynamics.dataloader import SCORE_THRESHOLD

# where the two jaw surfaces stand at jaw travel 0 (assets/finger_sampler.py:7-21,126-137): the lower jaw's body at y = -0.15, its profile
# extruded 0.03 toward the object; the upper jaw's body at y = +0.15
LOWER_OFFSET, UPPER_OFFSET = -0.12, 0.15
OBJECT_HALF_BOX_2D = 0.05           # metres per unit of Diffusion.object_vertices (generator/train.py:111-124)
DEG, CM = 180.0 / np.pi, 100.0
SIMULATED = 'squeeze'
SIMULATED_3D = 'squeeze_3d'      # label.SOURCES' name for the sliced form's rows; their 'simulated' mark is SIMULATED all the same


def _decode_units(scale: Optional[float], offset: Optional[float]) -> Dict[str, float]:
    """The decoders' scale / offset keywords: those that were given (the decoders' defaults are the sampler's units)."""
    return {k: float(v) for k, v in (("scale", scale), ("offset", offset)) if v is not None}


def finger_surfaces(samples, num_points: int = 200, scale: Optional[float] = None, offset: Optional[float] = None):
    """(B, L[, 1]) control values -> surfaces (B, 2, num_points) float64 on the device: L_j = yl_j - 0.12 and U_j = yr_j + 0.15 over
    dgdm_finger_decode_2d's curves.  scale / offset default to DGDM_DECODE_2D_* (sampler units); 1, 0 takes metres."""
    import torch
    from .. import engine
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.as_tensor(samples).to(dev)
    y = engine.finger_decode_2d(s, int(num_points), **_decode_units(scale, offset))[..., 1].double()
    return torch.stack([y[:, 0] + LOWER_OFFSET, y[:, 1] + UPPER_OFFSET], dim=1).contiguous()


def all_pairs(n_fingers: int, n_objects: int) -> np.ndarray:
    """(finger, object) of every combination, object-major, gripper-minor (the simulator's order)."""
    return np.array([(f, o) for o in range(n_objects) for f in range(n_fingers)], dtype=np.int32).reshape(-1, 2)


def fold(delta, period: float):
    """continuous_signed_delta (dynamics/utils.py:6-12) of arrays: folded once into [-period / 2, period / 2]."""
    d = np.asarray(delta, dtype=np.float64)
    return np.where(d > period / 2, d - period, np.where(d < -period / 2, d + period, d))


def add_poses(out: Dict[str, Any], pairs, **config) -> None:
    """engine.squeeze_tables' cells and y -> out's start (P, N, 2), closed and settled (P, N, 3): the cells' (theta rad, x m) and y; and
    out's pairs."""
    import torch
    from .. import engine
    cfg = engine.squeeze_config(**config)
    T, X = cfg.theta_cells, cfg.x_cells
    cells = out["cells"].long()
    theta = (cells // X).double() * (2.0 * np.pi) / float(T)
    x = -cfg.x_half + (cells % X).double() * (2.0 * cfg.x_half / (X - 1))
    out["start"] = torch.stack([theta[..., 0], x[..., 0]], dim=-1)
    out["closed"] = torch.stack([theta[..., 1], x[..., 1], out["y"][..., 0]], dim=-1)
    out["settled"] = torch.stack([theta[..., 2], x[..., 2], out["y"][..., 1]], dim=-1)
    out["pairs"] = pairs


def squeeze_map(samples, contours, starts, pairs=None, num_points: int = 200, scale: Optional[float] = None, offset: Optional[float] = None,
                tables: bool = False, workspace_bytes: Optional[int] = None, friction: float = 0.0, **config) -> Dict[str, Any]:
    """samples (B, L[, 1]) designs, contours (O, nv, 2) polygons in metres, starts (N, 3) = (theta0 rad, x0 m, y0 m) shared by all pairs,
    pairs (P, 2) (finger, object) or None = all, object-major.  config: engine.SQUEEZE_DEFAULTS' keys.  Device tensors:
      closed, settled (P, N, 3) float64 = (theta rad, x m, y m) after one closing and settled;  start (P, N, 2) = the snapped start cell's
      (theta, x);  cells (P, N, 3) int32;  flags (P, N) int32 (1 loose at the start, 2 ended loose, 4 cut by the x range);  with tables:
      S, touch_l, touch_r (P, theta_cells, x_cells), succ.  friction: the Coulomb coefficient mu (0: frictionless); with mu > 0 flags also
      carries 8 (the start cell is jammed) and 16 (the settled cell is), and tables adds jam and contact (engine.squeeze_tables)."""
    import torch
    from .. import engine
    sf = finger_surfaces(samples, num_points, scale, offset)
    ob = torch.as_tensor(contours)
    pr = all_pairs(sf.shape[0], ob.shape[0]) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    out = engine.squeeze_tables(sf, ob, pr, starts, tables=tables, workspace_bytes=workspace_bytes, friction=check_friction(friction, "squeeze_map"),
                                **config)
    add_poses(out, pr, **config)
    return out


def check_friction(friction, who: str) -> float:
    """The Coulomb coefficient as a float; ValueError for a negative or non-finite one.  Host code."""
    mu = float(friction)
    if not (np.isfinite(mu) and mu >= 0.0):
        raise ValueError(f"{who}: friction {friction!r} is not a finite non-negative number")
    return mu


def steps_from_args(args) -> Dict[str, int]:
    """--squeeze_closing_steps K / --squeeze_window R -> the config keys of those that were given; ValueError for K < 0 or R < 1.
    Host code."""
    k, r = getattr(args, "squeeze_closing_steps", None), getattr(args, "squeeze_window", None)
    if k is not None and k < 0:
        raise ValueError(f"--squeeze_closing_steps={k}: the number of steps cannot be negative")
    if r is not None and r < 1:
        raise ValueError(f"--squeeze_window={r}: the window is at least 1 cell")
    return {key: int(v) for key, v in (("closing_steps", k), ("window", r)) if v is not None}


def squeeze_metric(start, closed, settled, flags, y0=0.0, threshold: Sequence[float] = SCORE_THRESHOLD[1], friction: float = 0.0,
                   friction_3d: float = 0.0) -> Dict[str, Any]:
    """The metric dict of one (object, gripper) with build_metric's keys (dynamics/predicted.py, sim_test_mj.py:209-218) from
    squeeze_map's rows over the start orientations: start (n, 2), closed / settled (n, 3), flags (n,), host arrays.  One-step keys from
    one closing, classes with ``threshold`` in radians and metres as sim_test_mj.py:198-200 (+ 1); ``final_*`` from the settled pose;
    degrees and centimetres.  With friction > 0 (and only then) the dict also holds ``'squeeze_friction'``: mu and ``'squeeze_jammed'``: the
    number of starts that settled on a jammed cell (flag 16).  With friction_3d > 0 (3-D fingers' rule, and only then) it holds
    ``'squeeze_friction_3d'`` and ``'squeeze_jammed'`` likewise."""
    st, cl, se = (np.asarray(a, dtype=np.float64) for a in (start, closed, settled))
    fl = np.asarray(flags).reshape(-1)
    thr = np.asarray(threshold, dtype=np.float64).reshape(3)
    d = np.stack([fold(cl[:, 0] - st[:, 0], 2.0 * np.pi), cl[:, 1] - st[:, 1], cl[:, 2] - y0], axis=1)
    cls = np.where(d > thr, 2, np.where(d < -thr, 0, 1)).astype(np.int64)
    zeros = np.zeros(len(d))
    out = {'delta_theta': d[:, 0] * DEG, 'delta_pos': np.stack([d[:, 1] * CM, d[:, 2] * CM, zeros], axis=1),
           'profile': cls[:, 0], 'profile_x': cls[:, 1], 'profile_y': cls[:, 2],
           'final_theta': se[:, 0] * DEG, 'final_delta_theta': fold(se[:, 0] - st[:, 0], 2.0 * np.pi) * DEG,
           'final_pos': np.stack([se[:, 1] * CM, se[:, 2] * CM, zeros], axis=1),
           'simulated': SIMULATED, 'squeeze_loose': int(np.count_nonzero(fl & 1)), 'squeeze_cut': int(np.count_nonzero(fl & 4))}
    if float(friction) > 0.0:
        out.update({'squeeze_friction': float(friction), 'squeeze_jammed': int(np.count_nonzero(fl & 16))})
    if float(friction_3d) > 0.0:
        out.update({'squeeze_friction_3d': float(friction_3d), 'squeeze_jammed': int(np.count_nonzero(fl & 16))})
    return out


def start_orientations(num_rot: int, ori_range: Sequence[float]) -> np.ndarray:
    """starts (num_rot, 3): the simulators' start poses, (linspace(ori_range) + 1) * pi at x0 = y0 = 0."""
    theta0 = (np.linspace(ori_range[0], ori_range[1], int(num_rot)) + 1.0) * np.pi
    return np.stack([theta0, np.zeros_like(theta0), np.zeros_like(theta0)], axis=1)


def simulator_lists(out: Dict[str, Any], threshold: Sequence[float], friction: float = 0.0, friction_3d: float = 0.0):
    """A map's outputs -> the simulators' eight lists, one entry per pair: ``squeeze_metric`` in the metrics' slot, None (no videos: [])
    in the others - nothing is rendered."""
    start, closed, settled, flags = (out[k].cpu().numpy() for k in ("start", "closed", "settled", "flags"))
    metrics = [squeeze_metric(start[p], closed[p], settled[p], flags[p], 0.0, threshold, friction, friction_3d) for p in range(len(flags))]
    none: List[Any] = [None] * len(flags)
    return list(none), metrics, list(none), list(none), list(none), list(none), [[] for _ in none], list(none)


class _Simulator:
    """What the two simulators share: the model's config with ``closing_steps`` / ``window`` laid over it, checked on the host."""

    def configure(self, closing_steps: Optional[int], window: Optional[int], config: Dict[str, Any]) -> None:
        self.config = dict(config)
        if closing_steps is not None:
            self.config["closing_steps"] = int(closing_steps)
        if window is not None:
            self.config["window"] = int(window)
        from .. import engine
        c = engine.squeeze_config(**self.config)
        if c.closing_steps < 0 or c.window < 1:
            raise ValueError(f"{type(self).__name__}: closing_steps = {c.closing_steps} (need >= 0), window = {c.window} (need >= 1)")


class SqueezeSimulator(_Simulator):
    """``sim_test_batch`` (dynamics/sim_test_mj.py:249) answered by the squeeze model: ``simulator(samples (n, L, 1), object_ids,
    save_dir, num_cpus=, num_rot=, ori_range=, render=, render_last=)`` -> ``(gripper_imgs, metrics, profiles, profiles_x, profiles_y,
    finals, videos, save_gripper_dirs)``, object-major, gripper-minor, like ``PredictedSimulator``.

    Per (object, gripper) the metric is ``squeeze_metric`` over ``num_rot`` start orientations (linspace(ori_range) + 1) * pi at
    x0 = y0 = 0.  It carries ``'simulated': 'squeeze'``, ``'squeeze_loose'`` and ``'squeeze_cut'`` and never ``'predicted'``: these are
    this model's results, not MuJoCo measurements and not the dynamics model's opinion.  Nothing is rendered: the plot slots are None.
    2-D only.  The call draws no random number and touches none of the sampling path's handles, so the sampled designs are the same
    with the simulator on or off.  ``friction``: the Coulomb coefficient mu (0: frictionless); with mu > 0 the metrics also carry
    ``'squeeze_friction'`` and ``'squeeze_jammed'``."""

    def __init__(self, diffusion, closing_steps: Optional[int] = None, window: Optional[int] = None, friction: float = 0.0, **config):
        if getattr(diffusion, "mode", "point") == 'point_3d':
            raise ValueError("SqueezeSimulator: the squeeze model is 2-D only")
        self.friction = check_friction(friction, "SqueezeSimulator")
        self.diffusion = diffusion
        self.configure(closing_steps, window, config)

    def __call__(self, samples, object_ids, save_dir: Optional[str] = None, num_cpus: int = 32, num_rot: int = 360,
                 ori_range: Sequence[float] = (-1.0, 1.0), render: bool = True, render_last: bool = False):
        import torch
        d = self.diffusion
        if d.object_vertices is None:
            raise ValueError("SqueezeSimulator: the Diffusion holds no objects (object_vertices)")
        x = torch.as_tensor(np.asarray(samples), dtype=torch.float32)
        n = x.shape[0]
        known = d._object_ids()
        oidx = [known.index(o) for o in object_ids]
        bank = torch.as_tensor(d.object_vertices).detach().cpu().double()[oidx] * OBJECT_HALF_BOX_2D
        out = squeeze_map(x.reshape(n, -1), bank, start_orientations(num_rot, ori_range), friction=self.friction, **self.config)
        return simulator_lists(out, SCORE_THRESHOLD[1], self.friction)


# ---------------------------------------------------------------------------------------------------------------- 3-D: a sliced squeeze
# where the two jaw faces stand at jaw travel 0 in the 3-D scene: the left jaw's body at y = -0.23 (assets/finger_3d.py:126), its mesh the
# decoded surface y = yl(x, z) and a copy shifted by `width` in y (:38-57, called with width = 0.1 by sim/sim_3d.py:78-84) - the copy is
# the face that looks at the object, L = yl - 0.23 + width; the right jaw's body at y = +0.23 (:135), its decoded surface itself looking
# at the object, U = yr + 0.23
LOWER_OFFSET_3D, UPPER_OFFSET_3D, FINGER_WIDTH_3D = -0.23, 0.23, 0.1
NO_MESHES_3D = "the run's objects have no meshes (objects.npy or synthetic clouds): the sliced squeeze needs <object_dir>/<name>/model.obj"
FRICTION_2D_ONLY = ("friction is 2-D only: the contact normals of 3-D fingers have a z component that the sliced, per-plane model does not "
                    "see")


def finger_surfaces_3d(samples, sample_size: int = 25, width: float = FINGER_WIDTH_3D, scale: Optional[float] = None, offset: Optional[float] = None):
    """(B, 42[, 1]) control values -> (gx (mu,), gz (mv,), surfaces (B, 2, mv, mu) float64 on the device), mu = mv = sample_size:
    L_j[i] = yl(gx_i, gz_j) - 0.23 + width and U_j[i] = yr(gx_i, gz_j) + 0.23 over dgdm_finger_decode_3d's u-major grid, whose x depends
    on the u index only (cubic, clamped knots: NOT uniform) and whose z on the v index only.  gx / gz: host float64, read off the first
    finger.  scale / offset default to the sampler's units; 1, 0 takes metres."""
    import torch
    from .. import engine
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.as_tensor(samples).to(dev)
    n = int(sample_size)
    pts = engine.finger_decode_3d(s, n, **_decode_units(scale, offset)).double().reshape(s.shape[0], 2, n, n, 3)      # [B][finger][u][v][xyz]
    y = pts[..., 1].transpose(2, 3)                                                           # [B][finger][v][u]
    surfaces = torch.stack([y[:, 0] + LOWER_OFFSET_3D + float(width), y[:, 1] + UPPER_OFFSET_3D], dim=1).contiguous()
    return pts[0, 0, :, 0, 0].cpu().numpy().copy(), pts[0, 0, 0, :, 2].cpu().numpy().copy(), surfaces


def squeeze_map_3d(samples, meshes, starts, pairs=None, sample_size: int = 25, width: float = FINGER_WIDTH_3D, scale: Optional[float] = None,
                   offset: Optional[float] = None, tables: bool = False, workspace_bytes: Optional[int] = None, friction=None,
                   friction_3d: float = 0.0, **config) -> Dict[str, Any]:
    """squeeze_map for 3-D fingers: samples (B, 42[, 1]) designs, meshes a sequence of (vertices (nv, 3) in metres, triangles (nt, 3)) in
    the scene's frame (standing on z = 0), starts (N, 3) = (theta0 rad, x0 m, y0 m) shared by all pairs.  The meshes are sliced on the
    finger grid's levels (engine.squeeze_slice) and squeezed level by level (engine.squeeze_tables_3d); what lies between two levels is
    not seen.  Output keys as squeeze_map, plus segments / offsets.  The 2-D ``friction`` argument is refused (FRICTION_2D_ONLY).
    friction_3d: the Coulomb coefficient of the 3-D antipodal jamming rule (include/dgdm_hip.h "squeeze simulator, 3-D fingers, with
    Coulomb friction"; 0: frictionless, today's outputs bit for bit); with friction_3d > 0 flags also carries 8 / 16 (start / settled
    cell jammed), tables adds jam and contact, and the outputs hold the slicer's normals."""
    from .. import engine
    if friction is not None:
        raise ValueError(f"squeeze_map_3d: {FRICTION_2D_ONLY}")
    fmu = check_friction(friction_3d, "squeeze_map_3d: friction_3d")
    gx, gz, sf = finger_surfaces_3d(samples, sample_size, width, scale, offset)
    sl = engine.squeeze_slice(meshes, gz, normals=fmu > 0.0)
    pr = all_pairs(sf.shape[0], len(sl["offsets"])) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    extra = dict(friction_3d=fmu, gz=gz, normals=sl["normals"]) if fmu > 0.0 else {}
    out = engine.squeeze_tables_3d(sf, gx, sl["segments"], sl["offsets"], pr, starts, tables=tables, workspace_bytes=workspace_bytes, **extra, **config)
    add_poses(out, pr, **config)
    out.update(segments=sl["segments"], offsets=sl["offsets"])
    if fmu > 0.0:
        out["normals"] = sl["normals"]
    return out


class SqueezeSimulator3D(_Simulator):
    """``sim_test_batch_3d`` (dynamics/sim_test_mj_3d.py:229) answered by the sliced squeeze: ``simulator(samples (n, 42, 1), object_names,
    save_dir, num_cpus=, num_rot=, ori_range=, render=, render_last=)`` -> the same eight lists as ``SqueezeSimulator``, object-major,
    gripper-minor.  An object name is read from ``<object_mesh_dir>/<name>/model.obj`` (engine.read_obj) as it stands, in metres; a run
    whose objects have no meshes (objects.npy, synthetic clouds) is refused with a ValueError - a point cloud has no cross-section.
    Metrics: ``squeeze_metric`` with the 3-D thresholds SCORE_THRESHOLD[0], marked ``'simulated': 'squeeze'`` and never ``'predicted'``.
    The 2-D ``friction`` argument is refused (FRICTION_2D_ONLY).  ``friction_3d``: the Coulomb coefficient of the 3-D antipodal jamming
    rule (squeeze_map_3d; 0: frictionless); with friction_3d > 0, and only then, the metrics also carry ``'squeeze_friction_3d'`` and
    ``'squeeze_jammed'``.  This project's own model, untuned; nothing is claimed about MuJoCo."""

    def __init__(self, diffusion, object_mesh_dir: Optional[str] = None, closing_steps: Optional[int] = None, window: Optional[int] = None,
                 sample_size: int = 25, width: float = FINGER_WIDTH_3D, friction=None, friction_3d: float = 0.0, **config):
        if friction is not None:
            raise ValueError(f"SqueezeSimulator3D: {FRICTION_2D_ONLY}")
        self.friction_3d = check_friction(friction_3d, "SqueezeSimulator3D: friction_3d")
        if getattr(diffusion, "mode", "point_3d") != 'point_3d':
            raise ValueError("SqueezeSimulator3D: the sliced squeeze is for 3-D fingers (mode 'point_3d'); SqueezeSimulator is the 2-D one")
        self.diffusion = diffusion
        self.object_mesh_dir = object_mesh_dir if object_mesh_dir is not None else getattr(diffusion, "object_mesh_dir", None)
        if not self.object_mesh_dir:
            raise ValueError(f"SqueezeSimulator3D: {NO_MESHES_3D}")
        self.sample_size, self.width = int(sample_size), float(width)
        self.configure(closing_steps, window, config)
        self._meshes: Dict[str, Any] = {}

    def mesh(self, name):
        import os
        from .. import engine
        from ..dynamics.utils import MESH_FILE
        if name not in self._meshes:
            path = os.path.join(self.object_mesh_dir, str(name), MESH_FILE)
            if not os.path.isfile(path):
                raise ValueError(f"SqueezeSimulator3D: object '{name}' has no mesh at {path}")
            self._meshes[name] = engine.read_obj(path)
        return self._meshes[name]

    def __call__(self, samples, object_names, save_dir: Optional[str] = None, num_cpus: int = 32, num_rot: int = 360,
                 ori_range: Sequence[float] = (-1.0, 1.0), render: bool = True, render_last: bool = False):
        import torch
        x = torch.as_tensor(np.asarray(samples), dtype=torch.float32)
        n = x.shape[0]
        meshes = [self.mesh(o) for o in object_names]
        out = squeeze_map_3d(x.reshape(n, -1), meshes, start_orientations(num_rot, ori_range), sample_size=self.sample_size, width=self.width,
                             friction_3d=self.friction_3d, **self.config)
        return simulator_lists(out, SCORE_THRESHOLD[0], friction_3d=self.friction_3d)
