"""Scores of finger designs PREDICTED by the dynamics model, in the shapes the validation harness takes from a simulator.

The reference ranks its samples with MuJoCo roll-outs (dynamics/sim_test_mj*.py), which this package does not ship.  The dynamics
model that guides the chains predicts, for every (finger, object, orientation, position), the normalised motion the simulator
would measure after one interaction; ``engine.Guidance.score`` evaluates it forward-only on the whole grid.  This module turns
those numbers into

* ``predicted_objective``: the score dict of one finger from the grid tally (class histogram + sums), and
* ``PredictedSimulator``: a callable with the ``sim_test_batch`` / ``sim_test_batch_3d`` signature for
  ``Diffusion(simulator=...)``, so the unguided / guided / multi-object tables are filled without a simulator.

Units.  ``std`` and ``threshold`` are ``DynamicsDataset``'s (dynamics/dataloader.py:11-16, ``SCORE_STD`` / ``SCORE_THRESHOLD``):
radians for the rotation, metres for the two shifts; the model's outputs are scores divided by ``std``, and the class rule
compares them with ``threshold / std``.  The dicts built here are in the units of the simulator's ``metrics`` dict
(sim_test_mj.py:209-218): degrees (x 180 / pi) and centimetres (x 100).

Roll-outs.  The simulator closes the gripper 40 times per start orientation (dynamics/sim_test_mj.py:161-185, sim_test_mj_3d.py:
154-176) and reports the motion after the first closing and the settled pose after the last.  ``PredictedSimulator(...,
rollout_interactions=K)`` does the same with the model in the simulator's place (``engine.Guidance.rollout``): the one-step keys from the
first interaction, the ``final_*`` keys from the pose after the K-th.  With ``K = 0`` one interaction stands for both.

Goals.  ``goal_objective(metric, goal)`` scores a roll-out's settled poses against a chosen pose (``sampler.Goal``): how many start
orientations end within 3 / 5 / 10 degrees of it, the mean angle and position error.

These are the dynamics model's opinion, not simulator measurements; every metric dict carries ``'predicted': True``.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .dataloader import POS_NORM
from .metrics import _ROT, _SHIFT, GOAL_BASIN_DEG

DEG = 180.0 / np.pi       # radians -> degrees (sim_test_mj.py:210)
CM = 100.0                # metres -> centimetres (:211)


def classes(logits: np.ndarray, threshold_std: Sequence[float]) -> np.ndarray:
    """2 above the threshold, 0 below its negative, 1 between, per output (generator/diffusion.py:532, sim_test_mj.py:198-200 + 1)."""
    thr = np.asarray(threshold_std, dtype=np.float32)
    l = np.asarray(logits, dtype=np.float32)
    return np.where(l > thr, 2, np.where(l < -thr, 0, 1)).astype(np.int64)


def predicted_objective(counts, sums, n_cells: int, std: Sequence[float], opt_obj: str) -> Dict[str, Any]:
    """Scores of one finger on one object for ``opt_obj`` from the tally ``Guidance.score`` returns for it: ``counts`` (3, 3, 3),
    the joint histogram of the classes of (rotation, shift x, shift y) over the finger's ``n_cells`` grid cells, and ``sums`` (4,) =
    sum d0, sum |d0|, sum d1, sum d2 of the normalised outputs.  Key names and dtypes as ``metric2objective`` (dynamics/metrics.py:
    67-234) gives them for a metric whose profiles are the grid's classes and whose motions are the un-normalised outputs, with the
    one-step convention for the ``final_*`` keys (final motion = predicted motion).  ``std``: the dataset's (rad, m, m); the means
    come out in degrees and centimetres like the simulator's.  'convergence' is scored on final angles per orientation, which a
    histogram does not hold: use ``build_metric`` + ``metric2objective`` for it."""
    c = np.asarray(counts).reshape(3, 3, 3).astype(np.int64)
    s = np.asarray(sums, dtype=np.float64).reshape(4)
    n = int(n_cells)
    if int(c.sum()) != n:
        raise ValueError(f"predicted_objective: the histogram holds {int(c.sum())} cells, n_cells says {n}")
    std = np.asarray(std, dtype=np.float64).reshape(3)
    rate = lambda k: np.float32(k) / np.float32(n)                                          # noqa: E731  (np.mean(..., dtype=float32))
    rot_n = c.sum(axis=(1, 2))                                                              # cells per rotation class
    shift_n = {'x': c.sum(axis=(0, 2)), 'y': c.sum(axis=(0, 1))}
    d_theta, d_theta_abs = s[0] / n * std[0] * DEG, s[1] / n * std[0] * DEG
    d_pos = {'x': s[2] / n * std[1] * CM, 'y': s[3] / n * std[2] * CM}

    def rot_part(rot):
        return {f'num_{rot}_classes': np.int16(rot_n[_ROT[rot]]), 'delta_theta': d_theta, 'final_delta_theta': d_theta}

    def shift_part(shift):
        ax, _, cls = _SHIFT[shift]
        return {f'num_{shift}_classes': np.int16(shift_n[ax][cls]), f'delta_pos_{ax}': d_pos[ax], f'final_pos_{ax}': d_pos[ax]}

    if opt_obj == 'rotate':
        return {'success_rate': rate(rot_n[0] + rot_n[2]), 'num_zero_classes': np.int16(rot_n[1]), 'delta_theta_abs': d_theta_abs,
                'final_delta_theta_abs': d_theta_abs}
    if opt_obj == 'convergence':
        raise ValueError("predicted_objective: 'convergence' needs the final angle per orientation (build_metric + metric2objective)")
    head, _, tail = opt_obj.partition('_')
    if head == 'rotate' and tail in _ROT:
        return {'success_rate': rate(rot_n[_ROT[tail]]), **rot_part(tail)}
    if head == 'shift' and tail in _SHIFT:
        ax, _, cls = _SHIFT[tail]
        return {'success_rate': rate(shift_n[ax][cls]), **shift_part(tail)}
    if head in _ROT and tail in _SHIFT:
        ax, _, cls = _SHIFT[tail]
        joint = c[_ROT[head]].sum(axis=1 if ax == 'x' else 0)[cls]
        rot, sh = rot_part(head), shift_part(tail)
        return {'success_rate': rate(joint), f'num_{head}_{tail}_classes': rot[f'num_{head}_classes'] + sh[f'num_{tail}_classes'], **rot, **sh}
    raise ValueError('opt obj not supported')


def build_metric(logits, threshold_std: Sequence[float], std: Sequence[float], ori_range: Sequence[float] = (-1.0, 1.0),
                 final_pose=None, left=None, rollout_interactions: Optional[int] = None) -> Dict[str, Any]:
    """The ``metric`` dict ``metric2objective`` consumes (sim_test_mj.py:209-218) for one (object, gripper) from the model's
    normalised outputs ``logits`` (num_rot, 3) at the centre position over ``num_rot`` orientations of ``ori_range``: profiles from
    the classes, motions un-normalised with ``std`` (degrees, centimetres).  Without ``final_pose`` the one interaction stands for
    the settled pose too: ``final_theta`` = initial angle + predicted rotation, ``final_delta_theta`` = ``delta_theta``,
    ``final_pos`` = ``delta_pos``.  With ``final_pose`` (num_rot, 3) = (ori, pos_x, pos_y) after a roll-out of K interactions in the
    model's normalised inputs and ``left`` (num_rot,) (``Guidance.rollout``): ``final_theta`` = (ori + 1) x 180 degrees,
    ``final_delta_theta`` = the signed difference to the initial angle, folded once into [-180, 180] (``continuous_signed_delta``,
    dynamics/utils.py:6-12, in degrees), ``final_pos`` = pos x 0.03 m in centimetres; ``'rollout_interactions'`` = K, which the
    pose does not tell and the caller therefore states (required with ``final_pose``), ``'rollout_left_range'`` counts the orientations whose position left the range the model was trained
    on (``left >= 0``): past it the model extrapolates."""
    l = np.asarray(logits, dtype=np.float32).reshape(-1, 3)
    std = np.asarray(std, dtype=np.float64).reshape(3)
    cls = classes(l, threshold_std)
    delta_theta = l[:, 0].astype(np.float64) * std[0] * DEG
    delta_pos = np.stack([l[:, 1].astype(np.float64) * std[1] * CM, l[:, 2].astype(np.float64) * std[2] * CM, np.zeros(len(l))], axis=1)
    initial = (np.linspace(ori_range[0], ori_range[1], len(l)) + 1.0) * 180.0              # z_rots of sim_test_mj.py:142, in degrees
    metric = {'delta_theta': delta_theta, 'delta_pos': delta_pos, 'profile': cls[:, 0], 'profile_x': cls[:, 1], 'profile_y': cls[:, 2],
              'final_theta': initial + delta_theta, 'final_delta_theta': delta_theta.copy(), 'final_pos': delta_pos.copy(), 'predicted': True}
    if final_pose is None and left is None:
        return metric
    if final_pose is None or left is None:
        raise ValueError("build_metric: final_pose and left come together (Guidance.rollout returns both)")
    if rollout_interactions is None or int(rollout_interactions) < 1:
        raise ValueError("build_metric: a settled pose needs rollout_interactions = K >= 1, the number of interactions that made it")
    fp = np.asarray(final_pose, dtype=np.float64).reshape(-1, 3)
    lf = np.asarray(left).reshape(-1)
    if len(fp) != len(l) or len(lf) != len(l):
        raise ValueError(f"build_metric: {len(l)} orientations, final_pose holds {len(fp)} and left {len(lf)}")
    # (`initial` is float64 linspace, the device's start grid float32: a row that never moves shows ~1e-6 degrees, not 0 - far below
    #  the 3 / 5 / 10 degree thresholds the finals are scored with)
    final_theta = (fp[:, 0] + 1.0) * 180.0
    delta = final_theta - initial
    delta = np.where(delta > 180.0, delta - 360.0, np.where(delta < -180.0, delta + 360.0, delta))
    metric['final_theta'] = final_theta
    metric['final_delta_theta'] = delta
    metric['final_pos'] = np.stack([fp[:, 1] * POS_NORM * CM, fp[:, 2] * POS_NORM * CM, np.zeros(len(l))], axis=1)
    metric['rollout_interactions'] = int(rollout_interactions)
    metric['rollout_left_range'] = int(np.count_nonzero(lf >= 0))
    return metric


def goal_objective(metric: Dict[str, Any], goal) -> Dict[str, Any]:
    """Scores of one (object, gripper) for a ``Goal`` (dgdm_amd/goal.py) from the settled poses of a predicted roll-out: ``metric``
    is ``build_metric``'s with ``final_pose`` (it must carry ``'rollout_interactions'``: one interaction settles nothing), read through
    ``final_theta`` (num_rot,) in degrees and ``final_pos`` (num_rot, 3) in centimetres.
      goal_basin_{3,5,10}deg  start orientations whose final angle is within that many degrees of the goal angle, the difference wrapped
                              into [-180, 180] (np.int16, 0 .. num_rot)
      goal_error_deg          mean absolute wrapped angle error (float64, 0 .. 180)
      goal_pos_error_cm       mean distance of the final position from the goal position (float64)
      predicted               True
    A per-finger Goal is not scored (the metric does not say which finger it belongs to).  Like every score built on roll-outs, these
    are the dynamics model's opinion of its own iterates, not measurements."""
    if metric.get('predicted', False) and 'rollout_interactions' not in metric:
        raise ValueError("goal_objective: the metric holds no settled pose (PredictedSimulator(rollout_interactions=K >= 1) / build_metric(final_pose=...))")
    if getattr(goal, "fingers", None) is not None:
        raise ValueError("goal_objective: a per-finger Goal cannot be scored from one metric dict")
    theta = np.asarray(metric['final_theta'], dtype=np.float64).reshape(-1)
    pos = np.asarray(metric['final_pos'], dtype=np.float64).reshape(len(theta), -1)
    err = np.abs((theta - goal.theta_deg + 180.0) % 360.0 - 180.0)
    goal_cm = np.array([goal.pos[0], goal.pos[1]], dtype=np.float64) * POS_NORM * CM
    out: Dict[str, Any] = {f'goal_basin_{d}deg': np.sum(err <= d, dtype=np.int16) for d in GOAL_BASIN_DEG}
    out['goal_error_deg'] = float(np.mean(err))
    out['goal_pos_error_cm'] = float(np.mean(np.hypot(pos[:, 0] - goal_cm[0], pos[:, 1] - goal_cm[1])))
    out['predicted'] = True
    return out


def center_index(num_pos: int) -> int:
    """Index of the position 0 in linspace(-1, 1, num_pos); an even num_pos has none."""
    if num_pos % 2 == 0:
        raise ValueError(f"PredictedSimulator: num_pos = {num_pos} is even, so the position grid linspace(-1, 1, {num_pos}) has no centre cell "
                         "(pos = 0); use an odd num_pos")
    return num_pos // 2


def center_rows(logits, batch: int, grid_size: int, num_pos: int):
    """logits (n, R, 3) on the cond_fn grid (row = cell * B + finger, cell = (g * P + px) * P + py), tensor or array -> (n, B, G, 3):
    the rows at the centre position px = py = P // 2, where pos = (0, 0)."""
    c = center_index(num_pos)
    v = logits.reshape(logits.shape[0], grid_size, num_pos, num_pos, batch, 3)[:, :, c, c]
    return v.permute(0, 2, 1, 3) if hasattr(v, "permute") else v.transpose(0, 2, 1, 3)


class PredictedSimulator:
    """``sim_test_batch`` / ``sim_test_batch_3d`` (dynamics/sim_test_mj.py:249, sim_test_mj_3d.py:229) answered by the dynamics model
    of a ``Diffusion``: ``simulator(samples (n, L, 1), object_ids, save_dir, num_cpus=, num_rot=, ori_range=, render=, render_last=)``
    -> ``(gripper_imgs, metrics, profiles, profiles_x, profiles_y, finals, videos, save_gripper_dirs)``, object-major, gripper-minor.

    Per (object, gripper) the ``metric`` dict is ``build_metric`` of the centre-position cells of ``Guidance.score``'s logits over
    ``num_rot`` orientations of ``ori_range`` at timestep 0, with ``Diffusion.threshold_std`` / ``Diffusion.std`` (the dataset's units,
    see the module docstring).  Nothing is rendered: the plot slots are None, the video slots empty lists.

    The handles are the simulator's own (nothing the sampling path keeps is touched), and the 3-D FPS start draws come from a
    private ``sampler.TorchRng`` seeded from ``Diffusion.seed`` - never from the global CPU generator - so the sampled designs are
    bit-identical with scoring on, off or rolled out.

    ``rollout_interactions = K > 0``: every key comes from one ``Guidance.rollout`` call of K interactions on the same handle - the
    one-step keys from its first interaction's logits, the ``final_*`` keys from the pose after the last (``build_metric`` with
    ``final_pose`` / ``left``), and ``'rollout_interactions': K``.  ``0``: one ``Guidance.score`` call, one interaction for both.

    ``render_grippers=True`` (``--predicted_render``), in 3-D mode, with a ``save_dir`` and with ``diffusion.object_mesh_dir`` naming
    the directory of the objects' ``<name>/model.obj`` files: every gripper is drawn once (``sim/render_mesh.py render_grippers``) and
    written as ``<save_dir>/<object_idx>_<gripper_idx>_gripper.png`` for every pair; slot 0 holds those paths (sim_test_mj_3d.py:
    99-101).  With ``rollout_interactions > 0`` and ``render_last=True`` also, for each ``v < num_rot // 36``, the object alone at the
    pose the roll-out settled to from start orientation ``36 v``, with the 100-point contour of its start orientation drawn over it in
    (38, 80, 115), as ``<save_dir>/<object_idx>_<gripper_idx>/<v>.png``; the videos slot holds those lists (the reference's
    ``render_last`` branch, :218-225).  The jaws are not drawn in these frames: the model predicts the object's motion and no jaw
    position.  With synthetic objects (no mesh files) or in 2-D mode one line goes to stderr and the slots stay None.  The metrics and
    the FPS draws are the same with the flag on or off."""

    def __init__(self, diffusion, rollout_interactions: int = 0, render_grippers: bool = False):
        if int(rollout_interactions) < 0:
            raise ValueError(f"PredictedSimulator: rollout_interactions = {rollout_interactions} is negative")
        self.diffusion = diffusion
        self.rollout_interactions = int(rollout_interactions)
        self.render_grippers = bool(render_grippers)
        self._render_refused = False
        self._meshes: Dict[Any, Any] = {}
        self._handles: Dict[Any, Any] = {}
        self._rng = None

    def _guidance(self, batch: int, num_rot: int, ori_range, objects):
        import torch
        from .. import engine
        d = self.diffusion
        key = (batch, num_rot, float(ori_range[0]), float(ori_range[1]), tuple(objects.shape))
        g = self._handles.get(key)
        dyn = d._dyn().handle()
        if g is None or g.dyn is not dyn:
            g = engine.Guidance(dyn, batch, num_rot, d.num_pos, ori_range, objects.shape[0], d.noise_scheduler.config.num_train_timesteps,
                                objects.shape[1], d.sub_batch_size if d.mode == 'point_3d' else 0, max_objects=objects.shape[0],
                                contraction_dtype=d.contraction_dtype)
            g._bank = None
            self._handles[key] = g
        if g._bank is None or not torch.equal(g._bank, objects):
            g.set_objects(objects.to(d.device))
            g._bank = objects.clone()
        return g

    def _mesh_dir(self) -> Optional[str]:
        """Where the pictures' object meshes are, or None (said once on stderr) when this run has nothing to draw them from."""
        import sys
        d = self.diffusion
        root = getattr(d, "object_mesh_dir", None)
        why = None
        if d.mode != 'point_3d':
            why = "2-D fingers have no 3-D scene to draw"
        elif not root:
            why = "the run's objects do not come from mesh files"
        if why and not self._render_refused:
            self._render_refused = True
            print(f"[dgdm_amd] --predicted_render: {why} - nothing is rendered", file=sys.stderr)
        return None if why else root

    def _object_mesh(self, root: str, name):
        import os
        from .. import engine
        from .utils import MESH_FILE
        if name not in self._meshes:
            self._meshes[name] = engine.read_obj(os.path.join(root, str(name), MESH_FILE))
        return self._meshes[name]

    def _gripper_pictures(self, x, n_objects: int, save_dir: str) -> List[str]:
        """One picture per gripper, written once per (object, gripper) under the reference's name; the paths, object-major."""
        import os
        from .. import engine
        from ..sim import render_mesh as rm
        d = self.diffusion
        os.makedirs(save_dir, exist_ok=True)
        imgs = rm.render_grippers(engine.finger_mesh_3d(x.to(d.device)), engine.finger_mesh_faces(engine.MESH_3D, 25)).cpu().numpy()
        return [rm.write_png(os.path.join(save_dir, '%d_%d_gripper.png' % (i, b)), imgs[b]) for i in range(n_objects) for b in range(len(imgs))]

    def _settled_pictures(self, root: str, object_ids, final, num_rot: int, ori_range, save_dir: str) -> List[List[str]]:
        """final (objects, grippers, num_rot, 3): the settled (ori, pos_x, pos_y) in the model's normalised inputs."""
        import os
        from ..sim import render_mesh as rm
        nc, n = final.shape[:2]
        starts = np.arange(int(num_rot) // 36) * 36
        start_ori = np.linspace(ori_range[0], ori_range[1], int(num_rot))[starts]
        out: List[List[str]] = []
        for i in range(nc):
            verts, tris = self._object_mesh(root, object_ids[i])
            lists: List[List[str]] = [[] for _ in range(n)]
            if len(starts):
                contours = rm.object_silhouettes(verts, tris, (start_ori + 1.0) * np.pi).cpu().numpy()
                pose = final[i][:, starts].reshape(-1, 3)                                        # gripper-major, then v
                pos = np.stack([pose[:, 1] * POS_NORM, pose[:, 2] * POS_NORM, np.zeros(len(pose))], axis=1)
                frames = rm.object_views(verts, tris, (pose[:, 0] + 1.0) * np.pi, pos, rgb=rm.SETTLED_RGB).cpu().numpy()
                for b in range(n):
                    os.makedirs(os.path.join(save_dir, '%d_%d' % (i, b)), exist_ok=True)
                    for v in range(len(starts)):
                        frame = rm.draw_polyline(frames[b * len(starts) + v].copy(), contours[v], rm.OVERLAY_COLOUR)
                        lists[b].append(rm.write_png(os.path.join(save_dir, '%d_%d' % (i, b), '%d.png' % v), frame))
            out.extend(lists)
        return out

    def __call__(self, samples, object_ids, save_dir: Optional[str] = None, num_cpus: int = 32, num_rot: int = 360,
                 ori_range: Sequence[float] = (-1.0, 1.0), render: bool = True, render_last: bool = False):
        import torch
        from .. import sampler
        d = self.diffusion
        if not self.rollout_interactions:
            center_index(d.num_pos)            # the grid's centre cells; a roll-out starts at pos = 0 whatever the grid
        x = torch.as_tensor(np.asarray(samples), dtype=torch.float32)
        n = x.shape[0]
        x = x.reshape(n, -1)
        bank = torch.as_tensor(d.object_vertices).detach().cpu().float()
        known = d._object_ids()
        oidx = [known.index(o) for o in object_ids]
        g = self._guidance(n, int(num_rot), ori_range, bank)
        nc = len(oidx)
        starts = None
        K = self.rollout_interactions
        if d.mode == 'point_3d':
            if self._rng is None:
                self._rng = sampler.TorchRng(seed=int(d.seed))
            starts = self._rng.fps_starts(g.cfg.num_object_points, g.cfg.sub_batch_size, g.sweep_rows if K else g.rows, n_calls=max(K, 1) * nc)
        thr = [float(v) for v in d.threshold_std]
        std = [float(v) for v in d.std]
        total = nc * n
        none: List[Any] = [None] * total
        gripper_imgs, videos = list(none), [[] for _ in range(total)]
        mesh_dir = self._mesh_dir() if self.render_grippers and save_dir else None
        if mesh_dir:
            gripper_imgs = self._gripper_pictures(x, nc, save_dir)
        if K:
            xc = x.to(d.device)[None].expand(nc, n, x.shape[1]).contiguous()
            final, first, left = g.rollout(xc, oidx, std, K, starts=starts)
            # rows r = g * B + b  ->  (object, gripper, orientation)
            by = lambda t: t.reshape(nc, int(num_rot), n, *t.shape[2:]).transpose(1, 2).cpu().numpy()          # noqa: E731
            final, first, left = by(final), by(first), by(left)
            metrics = []
            for i in range(nc):
                for b in range(n):
                    metrics.append(build_metric(first[i, b], thr, std, ori_range, final_pose=final[i, b], left=left[i, b], rollout_interactions=K))
            if mesh_dir and render_last:
                videos = self._settled_pictures(mesh_dir, object_ids, final, int(num_rot), ori_range, save_dir)
            return gripper_imgs, metrics, list(none), list(none), list(none), list(none), videos, list(none)
        _, _, logits = g.score(x.to(d.device)[None].expand(nc, n, x.shape[1]).contiguous(), oidx, thr, timestep=0, starts=starts, want_logits=True)
        rows = center_rows(logits, n, int(num_rot), d.num_pos).cpu().numpy()                 # (object, gripper, orientation, 3)
        metrics = [build_metric(rows[i, b], thr, std, ori_range) for i in range(nc) for b in range(n)]
        return gripper_imgs, metrics, list(none), list(none), list(none), list(none), videos, list(none)
