"""Entry point behind ``python generator/train.py --mode=test ...`` (reference: generator/train.py:38-166).

Keeps the reference's flags (dynamics/parser.py) and construction order: synthetic finger set from ``RandomState(idx)``
(:43-58), U-Net + DDIM scheduler (:80-83), frozen dynamics model loaded from ``--checkpoint_path`` (:84-92), normalised
object point sets (:93-124), ``Diffusion`` (:129), then - in test mode - one pass of ``validation_step`` per batch of
fingers, which is what Lightning's ``trainer.validate`` does (:152-156).  ``--mode=train`` (the flags of
``generator/train_diffusion_{2d,3d}.sh``) is ``trainer.fit`` (:158-162): epochs over the shuffled 90 % split, one
``training_step`` + ``on_train_batch_end`` per batch on the GPU (csrc/unet_train.hip), the cosine schedule stepped per epoch,
``validation_step`` on the held-out 10 % every ``--val_step`` epochs, a Lightning-shaped checkpoint per epoch (the last ten and
``last.ckpt``, as the ModelCheckpoint of :137-146 keeps them).

Not the reference's: ``--edit_from FILE.npy`` (with ``--pin``, ``--edit_band_mm``, ``--edit_steps``; dgdm_amd/edit.py) makes the guided
chains of the test-mode sweep edit the file's designs - batch b its rows [b B, (b + 1) B) - instead of starting from noise.
``--mode=label --label_out rows.npy`` labels all dataset fingers with the dynamics model's predictions (dgdm_amd/label.py; no eps-net is
built) and writes the rows ``--global_cond`` takes, the raw rows and their statistics; ``--mode=test --cond_stats rows.json --cond_target
NAME=VALUE,...`` samples every batch under the target row those statistics make of raw units.  ``--label_source squeeze`` makes the same
files from the squeeze simulator instead (sim/squeeze.py; 2-D, no dynamics model, no checkpoint), and the target's report is then that
simulator's too.

Assets the image does not have are substituted, loudly:
* no checkpoint files  -> deterministic random-init weights (dgdm_amd.synth).
Objects come from ``--object_dir``: ``objects.npy`` ([n, vertices, 2|3], metres) when present; otherwise, as in the reference,
* 2-D: ``--object_dir`` is the Icons-50 ``.npy`` file itself (a pickled dict whose ``'image'`` holds (N, 3, H, W) icons): the
  contours of the eight test ids are extracted on the GPU without cv2 (assets/icon_process.py, csrc/contour.hip);
* 3-D: ``<object_dir>/<name>/model.obj`` of the six test objects, sampled on the GPU (dynamics/utils.py, csrc/mesh.hip).
Only when that input is missing or unreadable are synthetic objects with the same normalisation used, and the stderr line names the
missing file or meshes.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from .. import synth
from ..assets import icon_process
from ..dynamics import utils as object_utils
from ..dynamics.parser import parse
from ..dynamics.profile_forward_2d import ProfileForward2DModel
from ..dynamics.profile_forward_3d import ProfileForward3DModel
from ..scheduler import DDIMScheduler
from .dataloader import GripperDataset
from .diffusion import Diffusion
from .diffusion_utils import ConditionalUnet1D

OBJECT_IDS = [10000, 2009, 2114, 2082, 1041, 2048, 1045, 1019]     # Icons-50 test ids, generator/train.py:36
ICON_POINTS = 100                                                   # extract_contours' default num_points (generator/train.py:120)
OBJECT_NAMES_3D = ["3D_Dollhouse_Swing", "BABY_CAR", "Ecoforms_Plant_Container_B4_Har", "Threshold_Bamboo_Ceramic_Soap_Dish",
                   "Squirt_Strain_Fruit_Basket",
                   "Office_Depot_Canon_CLI_8CMY_Remanufactured_Ink_Cartridges_Color_Cyan_Magenta_Yellow_3_count"]   # assets/object_names_test.txt


def finger_control_points(num_fingers: int, fingers_3d: bool) -> np.ndarray:
    """generator/train.py:43-58 and assets/finger_3d.py:82-88: per finger idx, RandomState(idx) draws the y of the left then
    the right control points; x (and z) are fixed grids.  Shape (n, 14, 2) or (n, 42, 3)."""
    out = []
    for idx in range(num_fingers):
        rs = np.random.RandomState(idx)
        if fingers_3d:
            yl, yr = rs.uniform(-0.1, 0, size=21), rs.uniform(-0.1, 0, size=21)
            xg, zg = np.meshgrid(np.linspace(-0.12, 0.12, 7), np.linspace(0, 0.12, 3))
            side = lambda y: np.stack([xg.T.reshape(-1), y, zg.T.reshape(-1)], axis=-1)      # noqa: E731
            out.append(np.concatenate((side(yl), side(yr)), axis=0))
        else:
            x = np.linspace(-0.12, 0.12, 7)
            yl, yr = rs.uniform(-0.045, 0.015, size=7), rs.uniform(-0.045, 0.015, size=7)
            out.append(np.concatenate((np.stack([x, yl], axis=-1), np.stack([x, yr], axis=-1)), axis=0))
    return np.stack(out, axis=0)


def load_global_cond(path, num_fingers: int) -> np.ndarray:
    """--global_cond FILE.npy: float32 [num_fingers][gc] with 1 <= gc <= 256 and finite values, row i for finger i.  ValueError otherwise."""
    try:
        c = np.load(path, allow_pickle=False)
    except Exception as e:
        raise ValueError(f"--global_cond: cannot read '{path}' as a .npy array ({type(e).__name__}: {e})")
    if c.ndim != 2:
        raise ValueError(f"--global_cond: '{path}' has shape {c.shape}, expected [num_fingers][gc] (rank 2)")
    if c.shape[0] != num_fingers:
        raise ValueError(f"--global_cond: '{path}' has {c.shape[0]} rows, expected one per finger of the dataset (--num_fingers={num_fingers})")
    if not 1 <= c.shape[1] <= 256:
        raise ValueError(f"--global_cond: '{path}' has gc = {c.shape[1]}, outside 1..256")
    if c.dtype.kind not in "fiu":
        raise ValueError(f"--global_cond: '{path}' holds {c.dtype}, expected float32")
    c = np.ascontiguousarray(c, dtype=np.float32)
    if not np.isfinite(c).all():
        raise ValueError(f"--global_cond: '{path}' holds non-finite values (row {int(np.argwhere(~np.isfinite(c))[0][0])})")
    return c


def check_cond_flags(args) -> None:
    """--cfg_weight / --cond_drop_prob: finite weight, probability in [0, 1); without --global_cond they must be left at their defaults."""
    w, p = float(args.cfg_weight), float(args.cond_drop_prob)
    if not np.isfinite(w):
        raise ValueError(f"--cfg_weight={args.cfg_weight}: not a finite number")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"--cond_drop_prob={args.cond_drop_prob}: a probability in [0, 1)")
    if args.global_cond is None and getattr(args, "cond_target", None) is None and (w != 1.0 or p != 0.0):
        raise ValueError("--cfg_weight / --cond_drop_prob need --global_cond: an unconditional eps-net has nothing to mix or drop")


def check_label_flags(args):
    """--mode=label and --cond_stats / --cond_target, checked before anything is built: returns (LabelStats, requested target by column)
    of a targeted test run, else (None, None).  ValueError for every combination that cannot run."""
    from .. import dist as ddist
    from .. import label as lb
    target, stats_path = getattr(args, "cond_target", None), getattr(args, "cond_stats", None)
    source = getattr(args, "label_source", None) or 'model'
    if (getattr(args, "label_settled", False) or getattr(args, "label_squeeze_cells", None) is not None) and \
            not (args.mode == 'label' and source in ('squeeze', 'squeeze_3d')):
        raise ValueError("--label_settled / --label_squeeze_cells need --mode=label --label_source squeeze")
    if source != 'model' and args.mode != 'label':
        raise ValueError("--label_source needs --mode=label")
    if args.mode == 'label':
        if not args.label_out:
            raise ValueError("--mode=label needs --label_out FILE.npy")
        if source not in lb.SOURCES:
            raise ValueError(f"--label_source={source}: 'model', 'squeeze' or 'squeeze_3d'")
        if source == 'squeeze':
            if args.fingers_3d:
                raise ValueError("--label_source squeeze is 2-D only: a sliced squeeze evaluation per finger of a --fingers_3d dataset is out of "
                                 "scope, not supported")
            if int(args.label_rollout) != 0:
                raise ValueError("--label_rollout is the dynamics model's roll-out: with --label_source squeeze the settled columns are --label_settled")
            label_squeeze_config(args)          # --label_squeeze_cells / --squeeze_*: refused here
        elif source == 'squeeze_3d':
            if not args.fingers_3d:
                raise ValueError("--label_source squeeze_3d needs --fingers_3d: it is the sliced squeeze of 3-D fingers (--label_source squeeze is "
                                 "the 2-D one)")
            if int(args.label_rollout) != 0:
                raise ValueError("--label_rollout is the dynamics model's roll-out: with --label_source squeeze_3d the settled columns are "
                                 "--label_settled")
            label_squeeze_config(args)          # --label_squeeze_cells / --squeeze_*: refused here (--squeeze_friction: squeeze_friction_from_args)
        elif not args.classifier_guidance:
            raise ValueError("--mode=label needs --classifier_guidance and its flags: the labels are the dynamics model's predictions "
                             "(--label_source squeeze needs neither)")
        if args.label_layout not in lb.LAYOUTS:
            raise ValueError(f"--label_layout={args.label_layout}: 'mean' or 'per_object'")
        if int(args.label_rollout) < 0:
            raise ValueError(f"--label_rollout={args.label_rollout}: the number of interactions cannot be negative")
        if target is not None or stats_path is not None or args.global_cond is not None:
            raise ValueError("--mode=label writes condition rows; --global_cond / --cond_stats / --cond_target read them (--mode=train / test)")
        if max(ddist.world_rank()[0], int(os.environ.get("WORLD_SIZE", "1"))) > 1:      # torchrun, joined or not yet
            raise ValueError("--mode=label runs in one process: sharded labelling is not supported")
        return None, None
    if args.label_out:
        raise ValueError("--label_out needs --mode=label")
    if target is None and stats_path is None:
        return None, None
    if target is not None and stats_path is None:
        raise ValueError("--cond_target needs --cond_stats FILE.json: a target in raw units is standardised with the labelling run's statistics")
    if target is None:
        raise ValueError("--cond_stats needs --cond_target: the statistics only turn a target into a condition row")
    if args.mode != 'test':
        raise ValueError("--cond_target samples under a target row in --mode=test")
    if args.global_cond is not None:
        raise ValueError("--cond_target and --global_cond both set the condition rows of --mode=test: give one")
    stats = lb.LabelStats.load(stats_path)
    requested = stats.requested(lb.parse_target(target))         # an unknown column raises here
    if stats.source == 'squeeze':               # the report labels the samples on the recipe's own grid, whatever this run's is
        if args.fingers_3d:
            raise ValueError("--cond_stats: the rows were labelled by the squeeze simulator, which is 2-D only (--fingers_3d)")
    elif stats.source == 'squeeze_3d':          # likewise, by the sliced squeeze on the run's mesh files
        if not args.fingers_3d:
            raise ValueError("--cond_stats: the rows were labelled by the sliced squeeze of 3-D fingers: the run needs --fingers_3d")
    elif args.classifier_guidance:
        r = stats.recipe
        if r.get("G") != args.grid_size or r.get("P") != args.num_pos:
            raise ValueError(f"--cond_stats: the rows were labelled on a {r.get('G')} x {r.get('P')}^2 grid, this run's is {args.grid_size} x {args.num_pos}^2")
    return stats, requested


def label_squeeze_config(args):
    """--label_source squeeze [--label_squeeze_cells T,X --squeeze_closing_steps K --squeeze_window R --squeeze_friction MU] ->
    (squeeze_config, friction).  ValueError for cells that are not two integers T >= 1, X >= 2, K < 0, R < 1, a bad MU.  Host code."""
    from ..sim.squeeze import check_friction, steps_from_args
    config = {}
    cells = getattr(args, "label_squeeze_cells", None)
    if cells is not None:
        try:
            t, x = (int(v) for v in str(cells).split(","))
        except ValueError:
            raise ValueError(f"--label_squeeze_cells {cells!r}: two integers T,X expected") from None
        if t < 1 or x < 2:
            raise ValueError(f"--label_squeeze_cells {cells!r}: need T >= 1 and X >= 2")
        config.update(theta_cells=t, x_cells=x)
    config.update(steps_from_args(args))
    mu = getattr(args, "squeeze_friction", None)
    return config, 0.0 if mu is None else check_friction(mu, "--squeeze_friction")


def _save_squeeze_labels(args, raw, counts, recipe, object_ids, by: str):
    """What the two squeeze sources do with their raw rows alike: the statistics, label_dataset's three files, and the line that says how
    many tally starts were loose or cut.  `by`: who made the rows, for that line.  Returns (stats, raw)."""
    from .. import label as lb
    layout, settled, M = args.label_layout, bool(recipe["settled"]), len(object_ids)
    stats = lb.LabelStats(lb.column_names(layout, object_ids, int(settled)), layout, object_ids, recipe).fit(raw)
    stem = args.label_out[:-4] if args.label_out.endswith(".npy") else args.label_out
    if os.path.dirname(stem):
        os.makedirs(os.path.dirname(stem), exist_ok=True)
    np.save(stem + ".npy", stats.apply(raw))
    np.save(stem + "_raw.npy", raw)
    stats.save(stem + ".json")
    flat = [c for c, k in zip(stats.columns, stats.constant) if k]
    n_starts = raw.shape[0] * M * args.grid_size * args.num_pos ** 2
    print(f"[dgdm_amd] labelled {raw.shape[0]} fingers x {raw.shape[1]} columns by {by}"
          f"{', settled' if settled else ''}) -> {stem}.npy, {stem}_raw.npy, {stem}.json; of {n_starts} tally starts {int(counts[:, 0].sum())} were loose "
          f"at the start, {int(counts[:, 1].sum())} ended loose, {int(counts[:, 2].sum())} were cut by the table's x range"
          + (f"; constant columns (standardised to 0): {', '.join(flat)}" if flat else ""), flush=True)
    return stats, raw


def label_dataset_squeeze(args, dataset, objects, object_ids):
    """--mode=label --label_source squeeze: every dataset finger labelled by the squeeze simulator (label.label_fingers_squeeze) on the
    run's pose grid with the 2-D dataset's raw threshold and std; the same three files as label_dataset.  No dynamics model, no
    checkpoint.  The squeeze model's opinion: frictionless unless --squeeze_friction; its steps, window, friction and the thresholds
    are untuned for squeeze deltas; nothing is claimed about MuJoCo.  Returns (stats, raw)."""
    from .. import engine
    from .. import label as lb
    from ..dynamics.dataloader import SCORE_STD, SCORE_THRESHOLD
    from ..sim.squeeze import OBJECT_HALF_BOX_2D, SIMULATED
    config, mu = label_squeeze_config(args)
    M, layout, settled = objects.shape[0], args.label_layout, bool(args.label_settled)
    lb.cond_dim(layout, M, int(settled))
    thr, std = [float(v) for v in SCORE_THRESHOLD[1]], [float(v) for v in SCORE_STD[1]]
    fingers = np.stack([dataset[i] for i in range(len(dataset))])
    bank = torch.as_tensor(objects).detach().cpu().double() * OBJECT_HALF_BOX_2D       # the bank SqueezeSimulator builds
    rows, counts = lb.label_fingers_squeeze(torch.from_numpy(fingers), bank, list(range(M)), args.grid_size, args.num_pos, (-1.0, 1.0), thr, std,
                                            settled=settled, layout=layout, friction=mu, **config)
    raw, counts = rows.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
    full = {k: getattr(engine.squeeze_config(**config), k) for k in engine.SQUEEZE_DEFAULTS}
    recipe = {"G": args.grid_size, "P": args.num_pos, "ori_range": [-1.0, 1.0], "score_std": std, "source": SIMULATED, "squeeze_config": full,
              "friction": mu, "settled": settled, "threshold": thr}
    return _save_squeeze_labels(args, raw, counts, recipe, object_ids, f"the squeeze simulator ({layout}, {M} objects, friction {mu:g}")


def label_dataset_squeeze_3d(args, dataset, object_ids, mesh_dir):
    """--mode=label --label_source squeeze_3d: every finger of a --fingers_3d dataset labelled by the sliced squeeze
    (label.label_fingers_squeeze_3d) on the run's pose grid against <mesh_dir>/<name>/model.obj, with the 3-D dataset's raw threshold and
    std (SCORE_THRESHOLD[0] / SCORE_STD[0]); label_dataset's three files.  No dynamics model, no eps-net, no checkpoint.  The sliced
    squeeze's opinion: this project's model, not MuJoCo's; blind between two levels of the finger grid; frictionless; steps, window and
    thresholds untuned for squeeze deltas.  Returns (stats, raw)."""
    from .. import engine
    from .. import label as lb
    from ..dynamics.dataloader import SCORE_STD, SCORE_THRESHOLD
    from ..sim.squeeze import FINGER_WIDTH_3D, SIMULATED_3D
    config, _ = label_squeeze_config(args)
    M, layout, settled = len(object_ids), args.label_layout, bool(args.label_settled)
    lb.cond_dim(layout, M, int(settled))
    thr, std = [float(v) for v in SCORE_THRESHOLD[0]], [float(v) for v in SCORE_STD[0]]
    fingers = np.stack([dataset[i] for i in range(len(dataset))])
    meshes = [engine.read_obj(os.path.join(mesh_dir, str(n), object_utils.MESH_FILE)) for n in object_ids]
    sample_size, width = 25, FINGER_WIDTH_3D
    rows, counts = lb.label_fingers_squeeze_3d(torch.from_numpy(fingers), meshes, list(range(M)), args.grid_size, args.num_pos, (-1.0, 1.0), thr, std,
                                               settled=settled, layout=layout, sample_size=sample_size, width=width, **config)
    raw, counts = rows.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
    full = {k: getattr(engine.squeeze_config(**config), k) for k in engine.SQUEEZE_DEFAULTS}
    recipe = {"G": args.grid_size, "P": args.num_pos, "ori_range": [-1.0, 1.0], "score_std": std, "source": SIMULATED_3D, "squeeze_config": full,
              "sample_size": sample_size, "width": width, "settled": settled, "threshold": thr}
    return _save_squeeze_labels(args, raw, counts, recipe, object_ids, f"the sliced squeeze of 3-D fingers ({layout}, {M} meshes")


def _threshold_std(fingers_3d: bool):
    """(threshold / std in float32 as Diffusion forms it, std) of the dynamics dataset (dynamics/dataloader.py)."""
    from ..dynamics.dataloader import SCORE_STD, SCORE_THRESHOLD
    i = 0 if fingers_3d else 1
    thr, std = torch.tensor(SCORE_THRESHOLD[i].tolist()), torch.tensor(SCORE_STD[i].tolist())
    return [float(v) for v in thr / std], [float(v) for v in std]


def label_dataset(args, dataset, classifier, objects, object_ids, dev):
    """--mode=label: every dataset finger labelled at t = 0 with the dataset's threshold / std (as PredictedSimulator scores), the rows
    standardised and written: <label_out> (what --global_cond takes), <stem>_raw.npy, <stem>.json (LabelStats).  Returns (stats, raw)."""
    from .. import engine
    from .. import label as lb
    M, K, layout = objects.shape[0], int(args.label_rollout), args.label_layout
    lb.cond_dim(layout, M, K)                                   # more than 256 columns: ValueError before the handle is built
    thr, std = _threshold_std(args.fingers_3d)
    fingers = np.stack([dataset[i] for i in range(len(dataset))])
    g = engine.Guidance(classifier.handle(), args.batch_size, args.grid_size, args.num_pos, (-1.0, 1.0), M, args.num_train_timesteps,
                        objects.shape[1], args.sub_bs if args.fingers_3d else 0, max_objects=M)
    g.set_objects(objects.to(dev))
    raw = lb.label_fingers(g, torch.from_numpy(fingers), list(range(M)), thr, std=std, rollout=K, layout=layout, timestep=0, seed=int(args.seed),
                           chunk_batches=64).cpu().numpy()
    recipe = {"G": args.grid_size, "P": args.num_pos, "ori_range": [-1.0, 1.0], "threshold_std": thr, "score_std": std, "K": K, "timestep": 0,
              "seed": int(args.seed), "contraction_dtype": g.contraction_dtype}
    stats = lb.LabelStats(lb.column_names(layout, object_ids, K), layout, object_ids, recipe).fit(raw)
    stem = args.label_out[:-4] if args.label_out.endswith(".npy") else args.label_out
    if os.path.dirname(stem):
        os.makedirs(os.path.dirname(stem), exist_ok=True)
    np.save(stem + ".npy", stats.apply(raw))
    np.save(stem + "_raw.npy", raw)
    stats.save(stem + ".json")
    flat = [c for c, k in zip(stats.columns, stats.constant) if k]
    print(f"[dgdm_amd] labelled {raw.shape[0]} fingers x {raw.shape[1]} columns ({layout}, {M} objects, K = {K}) -> {stem}.npy, {stem}_raw.npy, {stem}.json"
          + (f"; constant columns (standardised to 0): {', '.join(flat)}" if flat else ""), flush=True)
    return stats, raw


def _load_or_synth(path, spec, seed, what):
    if path and os.path.exists(path):
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd)
        return {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    print(f"[dgdm_amd] {what}: '{path}' not found - using deterministic random-init weights (seed {seed})", file=sys.stderr)
    return synth.synth_state_dict(spec, seed)


def _objects(args, fingers_3d: bool):
    f = os.path.join(args.object_dir or "", "objects.npy")
    nv = args.object_max_num_vertices
    lo, hi = (torch.tensor([-0.1, -0.1, 0.0]), torch.tensor([0.1, 0.1, 0.12])) if fingers_3d else (torch.tensor([-0.05] * 2), torch.tensor([0.05] * 2))
    if os.path.isfile(f):
        raw = torch.from_numpy(np.load(f)).float()
        return (raw - lo) / (hi - lo) * 2.0 - 1.0, list(range(raw.shape[0]))            # generator/train.py:94-124
    if fingers_3d:
        # the reference's own inputs: <object_dir>/<name>/model.obj of the six test objects, sampled as sample_pts_from_mesh does (:100-109)
        missing = [n for n in OBJECT_NAMES_3D if not os.path.isfile(os.path.join(args.object_dir or "", n, object_utils.MESH_FILE))]
        if not missing:
            raw = torch.from_numpy(object_utils.sample_object_clouds(args.object_dir, OBJECT_NAMES_3D, nv)).float()
            return (raw - lo) / (hi - lo) * 2.0 - 1.0, list(OBJECT_NAMES_3D)
        print(f"[dgdm_amd] no objects.npy and no {object_utils.MESH_FILE} under --object_dir for {', '.join(missing)} - using synthetic objects",
              file=sys.stderr)
    else:
        path = args.object_dir or ""
        images, why = _icon_images(path)
        if images is not None:
            return _icon_objects(images, nv), list(OBJECT_IDS)
        print(f"[dgdm_amd] no objects.npy under --object_dir and no Icons-50 file at '{path}' ({why}) - using synthetic objects",
              file=sys.stderr)
    if fingers_3d:
        return torch.stack([synth.synth_object_3d(i, nv) for i in range(len(OBJECT_NAMES_3D))]), list(OBJECT_NAMES_3D)
    return torch.stack([synth.synth_object_2d(i, nv) for i in range(len(OBJECT_IDS))]), list(OBJECT_IDS)


def _object_mesh_dir(args):
    """The directory whose <name>/model.obj files _objects sampled the run's 3-D objects from, or None (2-D, objects.npy, synthetic)."""
    d = args.object_dir or ""
    if not args.fingers_3d or os.path.isfile(os.path.join(d, "objects.npy")):
        return None
    return d if all(os.path.isfile(os.path.join(d, n, object_utils.MESH_FILE)) for n in OBJECT_NAMES_3D) else None


def _icon_images(path):
    """(the 'image' array of the Icons-50 file at path, None) or (None, why not)."""
    if not os.path.isfile(path):
        return None, "no such file"
    try:
        images = np.load(path, allow_pickle=True).item()["image"]
    except Exception as e:          # not a .npy, not a pickled dict, no 'image': the file is not Icons-50
        return None, f"unreadable: {type(e).__name__}: {e}"
    return images, None


def _icon_objects(images, nv: int) -> torch.Tensor:
    """generator/train.py:111-124: the rescaled 100-point contours of the test icons (all in one device call), float32, normalised to
    [-1, 1] with the reference's statements."""
    if nv != ICON_POINTS:
        raise ValueError(f"--object_max_num_vertices={nv}, but the icon contours have {ICON_POINTS} points (extract_contours' default, "
                         f"generator/train.py:120): pass --object_max_num_vertices={ICON_POINTS}")
    icons = np.asarray(images)[OBJECT_IDS].transpose((0, 2, 3, 1))
    contours = icon_process.extract_contours_batch(icons, ICON_POINTS, rescale=True)
    object_pts_max_x, object_pts_min_x, object_pts_max_y, object_pts_min_y = 0.05, -0.05, 0.05, -0.05
    object_vertices = torch.stack([torch.from_numpy(c).float() for c in contours], dim=0)
    object_vertices[..., 0] = (object_vertices[..., 0] - object_pts_min_x) / (object_pts_max_x - object_pts_min_x) * 2.0 - 1.0
    object_vertices[..., 1] = (object_vertices[..., 1] - object_pts_min_y) / (object_pts_max_y - object_pts_min_y) * 2.0 - 1.0
    return object_vertices


def _object_exporter(args):
    """--save_objects: export(model_root, name) for Diffusion.object_exporter, or None (with one line on stderr) when the run's objects are
    not icons.  A model root named after one object id (the per-object chains) gets that object, any other (allobj, unguided) all eight;
    an icon whose contour cannot be meshed is named on stderr and left out."""
    images, why = (None, "3-D objects are scanned meshes, already files") if args.fingers_3d else _icon_images(args.object_dir or "")
    if images is None:
        print(f"[dgdm_amd] --save_objects: no Icons-50 file at '{args.object_dir or ''}' ({why}) - nothing to export", file=sys.stderr)
        return None
    icons = np.ascontiguousarray(np.asarray(images)[OBJECT_IDS].transpose((0, 2, 3, 1)))

    def export(model_root, name):
        pick = [i for i, idx in enumerate(OBJECT_IDS) if str(idx) == name] or list(range(len(OBJECT_IDS)))
        refused = icon_process.save_icon_objects(icons[pick], model_root, [OBJECT_IDS[i] for i in pick], num_points=ICON_POINTS, skip_invalid=True)
        if refused:
            print(f"[dgdm_amd] --save_objects: {model_root}: the contours of objects {refused} cannot be meshed - left out", file=sys.stderr)
    return export


def _classifier(args, L: int, dev):
    """The frozen dynamics model of --classifier_guidance (generator/train.py:84-92) and the run's objects: (model, objects, object ids)."""
    if args.fingers_3d:
        classifier = ProfileForward3DModel(output_ch=3, params_ch=L)
        spec = synth.dyn3d_spec(L)
    else:
        classifier = ProfileForward2DModel(output_ch=3, params_ch=L, object_ch=2 * args.object_max_num_vertices)
        spec = synth.dyn2d_spec(L, 2 * args.object_max_num_vertices)
    classifier.load_state_dict(_load_or_synth(args.checkpoint_path, spec, 22 + int(args.fingers_3d), "dynamics checkpoint"))
    classifier.eval().requires_grad_(False).to(dev)
    objects, object_ids = _objects(args, args.fingers_3d)
    return classifier, objects, object_ids


def fit(model: Diffusion, pts: np.ndarray, args, bounds, dev) -> Diffusion:
    """``trainer.fit(diffusion_model, train_loader, val_loader)`` (generator/train.py:44-45, 66-67, 147-162) without Lightning: the
    loop its ``LightningTrainer(max_epochs=num_epochs, check_val_every_n_epoch=val_step)`` runs.  Under torchrun every rank takes the
    slice ``indices[rank::world]`` of the epoch's permutation (DistributedSampler) and the gradients are averaged (DDP)."""
    from torch.utils.data import DataLoader
    from .. import dist as ddist
    n = pts.shape[0]
    train_ids, val_ids = list(range(int(n * 0.9))), list(range(int(n * 0.9), n))
    cond = getattr(model, "global_cond_rows", None)             # --global_cond: row i belongs to finger i
    sub = lambda ids: None if cond is None else cond[ids]        # noqa: E731
    train_set, val_set = GripperDataset(pts[train_ids], *bounds, cond=sub(train_ids)), GripperDataset(pts[val_ids], *bounds, cond=sub(val_ids))
    world, rank = ddist.world_rank()
    if not hasattr(model, "lr_scheduler"):      # a resumed model (load_checkpoint) carries its schedule position
        model.configure_optimizers()
    model.to(dev)
    if world > 1:
        # Lightning wraps the module in DistributedDataParallel, whose constructor broadcasts rank 0's parameters and buffers (generator/
        # train.py:147-162 with strategy 'ddp'): without it every rank would start from its own random eps-net and the averaged gradients
        # would be taken at different weights.  A resumed model (same checkpoint file on every rank) already agrees and keeps its handle.
        if getattr(model, "_unet_trainer", None) is None:
            with torch.no_grad():
                for t in list(model.noise_pred_net.parameters()) + list(model.noise_pred_net.buffers()):
                    t.copy_(ddist.broadcast_from_rank0(t.detach().clone()))
        # the noise / timestep draws of get_stats come from the device generator: a different stream per rank, as DDP workers have
        torch.cuda.manual_seed((int(torch.initial_seed()) + 7919 * rank) & 0x7FFFFFFFFFFFFFFF)
    ckdir = os.path.join(args.save_dir, "checkpoints") if args.save_dir else None
    if ckdir and rank == 0:
        os.makedirs(ckdir, exist_ok=True)
    step, log = int(getattr(model, "global_step", 0)), []
    # save_top_k = 10 also counts the epoch files a resumed run finds in place
    kept = sorted(os.path.join(ckdir, f) for f in os.listdir(ckdir) if f.startswith("epoch=") and f.endswith(".ckpt")) if ckdir and os.path.isdir(ckdir) else []
    val_loader = DataLoader(val_set, batch_size=args.batch_size, shuffle=False, num_workers=0, drop_last=False)

    def validate(limit=None):
        # Every rank walks the WHOLE validation set, batch by batch, and that is deliberate: validation_step's guided chains are sharded
        # over the ranks inside each batch (objectives / objects over ranks, results all-gathered: diffusion.py guided_* ->
        # dist.guided_chains_sharded), so all ranks must enter the same batches.  A DistributedSampler on top (the reference's Lightning
        # default) would hand the ranks different batches under those collectives.
        model.eval()
        out = []
        with torch.no_grad():
            for bi, batch in enumerate(val_loader):
                if limit is not None and bi >= limit:
                    break
                out.append(model.validation_step(batch, bi)["stats"])
        model.train()
        return out
    if len(val_set):
        validate(limit=2)                      # Lightning's sanity check (num_sanity_val_steps = 2) before the first epoch
    for epoch in range(model.lr_scheduler.last_epoch, args.num_epochs):
        model.current_epoch = epoch
        if world == 1:
            loader = DataLoader(train_set, batch_size=args.batch_size, shuffle=True, num_workers=0, drop_last=False)
        else:                                   # DistributedSampler(shuffle=True, seed=0): randperm from Generator(seed + epoch), padded, strided
            gen = torch.Generator()
            gen.manual_seed(epoch)
            idx = torch.randperm(len(train_set), generator=gen).tolist()
            total = -(-len(idx) // world) * world
            idx = (idx + idx[:total - len(idx)])[rank:total:world]
            loader = DataLoader(torch.utils.data.Subset(train_set, idx), batch_size=args.batch_size, shuffle=False, num_workers=0, drop_last=False)
        losses = []
        for bi, batch in enumerate(loader):
            losses.append(float(model.training_step(batch, bi)))
            model.on_train_batch_end(None, batch, bi)
            step += 1
        model.lr_scheduler.step()
        rec = {"epoch": epoch, "train/loss": float(np.mean(losses)), "lr": model.lr_scheduler.get_last_lr()[0], "ema_decay": model.ema.decay}
        if (epoch + 1) % max(1, args.val_step) == 0 and len(val_set):
            vs = validate()
            rec.update({k: float(np.mean([v[k] for v in vs])) for k in vs[0]})
        log.append(rec)
        if rank == 0:
            print("[dgdm_amd] " + ", ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in rec.items()), flush=True)
            if ckdir:
                ck = model.checkpoint(epoch=epoch + 1, global_step=step)
                f = os.path.join(ckdir, "epoch=%04d.ckpt" % epoch)
                torch.save(ck, f)
                torch.save(ck, os.path.join(ckdir, "last.ckpt"))
                if f in kept:                  # a run resumed from an older checkpoint re-saves epochs that are already on the list
                    kept.remove(f)
                kept.append(f)
                while len(kept) > 10:          # save_top_k = 10, monitor = 'epoch', mode = 'max'
                    old = kept.pop(0)
                    if os.path.exists(old):
                        os.remove(old)
    model.sync_model()
    model.train_log = log
    if world > 1:
        # every rank took the same Adam steps on the same averaged gradients from the same start: the replicas must be bit-identical
        flat = torch.cat([p.detach().reshape(-1).double() for p in model.noise_pred_net.parameters()])
        sums = ddist.all_gather_rows(torch.stack([flat.sum(), flat.abs().sum(), (flat * torch.arange(1, flat.numel() + 1, device=flat.device, dtype=flat.dtype)).sum()]))
        if not bool((sums == sums[0]).all()):
            raise RuntimeError(f"data-parallel replicas of the eps-net diverged: per-rank parameter checksums {sums.tolist()}")
        if rank == 0:
            print(f"[dgdm_amd] {world} ranks hold identical eps-net parameters (checksum {float(sums[0][1]):.9g})", flush=True)
    return model


def _labels_by_squeeze(args) -> bool:
    """--mode=label --label_source squeeze / squeeze_3d: a user of the --squeeze_* flags (squeeze_3d: but for --squeeze_friction)."""
    return getattr(args, "mode", "test") == 'label' and (getattr(args, "label_source", None) or 'model') in ('squeeze', 'squeeze_3d')


def squeeze_friction_from_args(args):
    """--squeeze_friction MU -> mu, or None without the flag.  ValueError: a negative or non-finite mu, --squeeze_sim_3d (friction is 2-D
    only), no squeeze user (--squeeze_sim or --resample_potential squeeze).  Host-side checks only."""
    mu = getattr(args, "squeeze_friction", None)
    if mu is None:
        return None
    from ..sim.squeeze import FRICTION_2D_ONLY, check_friction
    mu = check_friction(mu, "--squeeze_friction")
    if getattr(args, "squeeze_sim_3d", False):
        raise ValueError(f"--squeeze_friction with --squeeze_sim_3d: {FRICTION_2D_ONLY}")
    if getattr(args, "mode", "test") == 'label' and getattr(args, "label_source", None) == 'squeeze_3d':
        raise ValueError(f"--squeeze_friction with --label_source squeeze_3d: {FRICTION_2D_ONLY}")
    if (getattr(args, "resample_potential", None) or 'model') == 'squeeze_3d':
        raise ValueError(f"--squeeze_friction with --resample_potential squeeze_3d: {FRICTION_2D_ONLY}")
    if not getattr(args, "squeeze_sim", False) and (getattr(args, "resample_potential", None) or 'model') != 'squeeze' and not _labels_by_squeeze(args):
        raise ValueError("--squeeze_friction needs --squeeze_sim or --resample_potential squeeze (or --mode=label --label_source squeeze)")
    return mu


def squeeze_sim_config(args, flag: str):
    """What --squeeze_sim and --squeeze_sim_3d (`flag`) refuse alike, then the config keys of --squeeze_closing_steps / --squeeze_window."""
    if getattr(args, "predicted_sim", False):
        raise ValueError(f"{flag} and --predicted_sim both fill the objective tables: choose one")
    if getattr(args, "mode", "test") != 'test':
        raise ValueError(f"{flag} scores the samples of --mode=test")
    if getattr(args, "goal_pose", None):
        raise ValueError(f"{flag} with --goal_pose: goal scores (dynamics/predicted.py goal_objective) are marked as the dynamics model's "
                         "predictions, which squeeze results are not - not supported")
    if not getattr(args, "classifier_guidance", False):
        raise ValueError(f"{flag} needs --classifier_guidance: the run's objects come with it")
    from ..sim.squeeze import steps_from_args
    return steps_from_args(args)


def squeeze_from_args(args):
    """--squeeze_sim [--squeeze_closing_steps K --squeeze_window R --squeeze_friction MU] -> SqueezeSimulator's keywords, or None without
    the flag.  Host-side checks only."""
    k, r = getattr(args, "squeeze_closing_steps", None), getattr(args, "squeeze_window", None)
    mu = squeeze_friction_from_args(args)
    if not getattr(args, "squeeze_sim", False):
        if (k is not None or r is not None) and not getattr(args, "squeeze_sim_3d", False) and \
                (getattr(args, "resample_potential", None) or 'model') not in ('squeeze', 'squeeze_3d') and not _labels_by_squeeze(args):
            raise ValueError("--squeeze_closing_steps / --squeeze_window need --squeeze_sim (or, with --fingers_3d, --squeeze_sim_3d), or "
                             "--resample_potential squeeze / squeeze_3d")
        return None
    if getattr(args, "squeeze_sim_3d", False):
        raise ValueError("--squeeze_sim and --squeeze_sim_3d: choose one (--squeeze_sim is 2-D only, --squeeze_sim_3d is for --fingers_3d)")
    if getattr(args, "fingers_3d", False):
        raise ValueError("--squeeze_sim is 2-D only: the squeeze model has no 3-D fingers (--fingers_3d); --squeeze_sim_3d is the sliced form "
                         "for them")
    config = squeeze_sim_config(args, "--squeeze_sim")
    return config if mu is None else dict(config, friction=mu)


def squeeze_friction_3d_from_args(args):
    """--squeeze_friction_3d MU -> mu, or None without the flag.  ValueError: a negative or non-finite mu, no --squeeze_sim_3d (the labels
    and the resampling potential of 3-D fingers have no friction).  Host-side checks only."""
    mu = getattr(args, "squeeze_friction_3d", None)
    if mu is None:
        return None
    from ..sim.squeeze import check_friction
    mu = check_friction(mu, "--squeeze_friction_3d")
    if not getattr(args, "squeeze_sim_3d", False):
        raise ValueError("--squeeze_friction_3d needs --squeeze_sim_3d: it is the friction of the sliced squeeze's scores (--squeeze_friction is "
                         "the 2-D one; --label_source squeeze_3d and --resample_potential squeeze_3d are frictionless)")
    return mu


def squeeze_3d_from_args(args):
    """--squeeze_sim_3d [--squeeze_closing_steps K --squeeze_window R --squeeze_friction_3d MU] -> SqueezeSimulator3D's keywords, or None
    without the flag.  Host-side checks only; that the run's objects are mesh files is checked where they are known (train)."""
    mu = squeeze_friction_3d_from_args(args)
    if not getattr(args, "squeeze_sim_3d", False):
        return None
    squeeze_friction_from_args(args)        # --squeeze_friction: refused, that rule is 2-D only
    if not getattr(args, "fingers_3d", False):
        raise ValueError("--squeeze_sim_3d needs --fingers_3d: it is the squeeze model for 3-D fingers (--squeeze_sim is the 2-D one)")
    config = squeeze_sim_config(args, "--squeeze_sim_3d")
    return config if mu is None else dict(config, friction_3d=mu)


def train(args):
    dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else int(os.environ.get("LOCAL_RANK", "0")))
    pts = finger_control_points(args.num_fingers, args.fingers_3d)
    max_y, min_y = (0.0, -0.1) if args.fingers_3d else (0.015, -0.045)
    check_cond_flags(args)
    squeeze_from_args(args)                 # --squeeze_sim: refused here, before anything is built
    if squeeze_3d_from_args(args) is not None and _object_mesh_dir(args) is None:      # --squeeze_sim_3d: likewise
        raise ValueError("--squeeze_sim_3d needs the run's objects as mesh files (<object_dir>/<name>/model.obj): objects.npy and synthetic "
                         "clouds have no cross-sections")
    cond_stats, cond_requested = check_label_flags(args)    # --mode=label, --cond_stats / --cond_target: refused here, before anything is built
    label_3d = args.mode == 'label' and getattr(args, "label_source", None) == 'squeeze_3d'
    if (label_3d or (cond_stats is not None and cond_stats.source == 'squeeze_3d')) and _object_mesh_dir(args) is None:
        from ..sim.squeeze import NO_MESHES_3D
        raise ValueError(f"{'--label_source squeeze_3d' if label_3d else '--cond_stats'}: {NO_MESHES_3D}")
    from ..edit import plan_from_args
    edit_plan = plan_from_args(args)        # --edit_from / --pin / --edit_band_mm / --edit_steps: read and checked before anything is built
    if edit_plan is not None and (args.mode != 'test' or not args.classifier_guidance):
        raise ValueError("--edit_from edits designs in the guided chains of --mode=test and needs --classifier_guidance")
    from ..resample import resample_from_args
    resample = resample_from_args(args)     # --resample_every / --resample_beta / --resample_ess: refused here unless --classifier_guidance and --eta > 0
    if (getattr(args, "resample_potential", None) or 'model') == 'squeeze_3d' and _object_mesh_dir(args) is None:
        from ..sim.squeeze import NO_MESHES_3D
        raise ValueError(f"--resample_potential squeeze_3d: {NO_MESHES_3D}")
    cond = load_global_cond(args.global_cond, args.num_fingers) if args.global_cond is not None else None
    gc = 0 if cond is None else cond.shape[1]
    if cond_stats is not None:
        gc = cond_stats.dim                 # --cond_target: the eps-net is as wide as the labelling run's rows
    dataset = GripperDataset(pts, 0.12, -0.12, max_y, min_y, cond=cond)
    L = args.ctrlpts_dim
    if args.mode == 'label' and (getattr(args, "label_source", None) or 'model') == 'squeeze':      # no eps-net, no dynamics model: objects alone
        objects, object_ids = _objects(args, False)
        return label_dataset_squeeze(args, dataset, objects, object_ids)
    if label_3d:                            # likewise: the mesh files alone
        return label_dataset_squeeze_3d(args, dataset, list(OBJECT_NAMES_3D), _object_mesh_dir(args))
    if args.mode == 'label':                # no eps-net: the dynamics model and the objects of --classifier_guidance alone
        classifier, objects, object_ids = _classifier(args, L, dev)
        return label_dataset(args, dataset, classifier, objects, object_ids, dev)
    unet = ConditionalUnet1D(input_dim=1, global_cond_dim=gc, down_dims=[128, 256], diffusion_step_embed_dim=32)
    mode = 'point_3d' if args.fingers_3d else 'point'
    scheduler = DDIMScheduler(num_train_timesteps=args.num_train_timesteps, beta_schedule='squaredcos_cap_v2', clip_sample=True,
                              prediction_type='epsilon')
    classifier, objects, object_ids = None, None, None
    if args.classifier_guidance:
        classifier, objects, object_ids = _classifier(args, L, dev)
    elif cond_stats is not None and cond_stats.source == 'squeeze':
        objects, object_ids = _objects(args, False)     # the squeeze report's objects: the object flags without a dynamics model, for this only
    elif cond_stats is not None and cond_stats.source == 'squeeze_3d':
        objects, object_ids = _objects(args, True)      # the names the report reads <object_dir>/<name>/model.obj by
    if cond_stats is not None and objects is not None and objects.shape[0] != len(cond_stats.object_ids):
        raise ValueError(f"--cond_stats: the rows were labelled against {len(cond_stats.object_ids)} objects, this run has {objects.shape[0]}")
    model = Diffusion(noise_pred_net=unet, noise_scheduler=scheduler, num_inference_steps=args.num_inference_steps, mode=mode, input_dim=1,
                      num_points=L, learning_rate=args.learning_rate, lr_warmup_steps=args.lr_warmup_steps, ema_power=args.ema_power,
                      class_cond=args.classifier_guidance, classifier_model=classifier, grid_size=args.grid_size, num_pos=args.num_pos,
                      object_vertices=objects, object_ids=object_ids, num_cpus=args.num_cpus, pts_x_dim=args.ctrlpts_x_dim,
                      pts_z_dim=args.ctrlpts_z_dim, sub_batch_size=args.sub_bs, render_video=args.render_video, seed=args.seed,
                      eta=float(getattr(args, "eta", 0.0) or 0.0), noise_seed=getattr(args, "noise_seed", None))
    if not args.classifier_guidance and objects is not None:
        model.object_vertices, model.object_ids = objects, object_ids      # Diffusion keeps them only with class_cond: the squeeze report reads them
    model.shared_step_noise = bool(getattr(args, "shared_step_noise", False))
    model.save_meshes = bool(getattr(args, "save_meshes", False))
    model.edit_plan = edit_plan
    from ..resample import squeeze_potential_from_args
    potential = squeeze_potential_from_args(args)       # --resample_potential squeeze: the fingers weighed by the squeeze model
    if resample is not None and potential is not None and args.resample_potential == 'squeeze_3d':
        from ..resample import with_squeeze_3d
        from ..sim.squeeze import SqueezeSimulator3D
        reader = SqueezeSimulator3D(model, object_mesh_dir=_object_mesh_dir(args))     # the mesh files --squeeze_sim_3d reads, in the handle's order
        resample = with_squeeze_3d(resample, [reader.mesh(n) for n in OBJECT_NAMES_3D], **potential)
    elif resample is not None and potential is not None:
        from ..resample import with_squeeze
        from ..sim.squeeze import OBJECT_HALF_BOX_2D
        bank = torch.as_tensor(objects).detach().cpu().double() * OBJECT_HALF_BOX_2D      # the bank SqueezeSimulator builds, in the handle's order
        resample = with_squeeze(resample, bank.numpy(), **potential)
    model.resample = resample
    model.cfg_weight, model.cond_drop_prob, model.global_cond_rows = float(args.cfg_weight), float(args.cond_drop_prob), cond
    if getattr(args, "save_objects", False):
        model.object_exporter = _object_exporter(args)
    rollout = int(getattr(args, "predicted_rollout", 0) or 0)
    if rollout and not getattr(args, "predicted_sim", False):
        raise ValueError(f"--predicted_rollout={rollout} needs --predicted_sim: it sets how many interactions the predicted simulator iterates")
    if rollout < 0:
        raise ValueError(f"--predicted_rollout={rollout}: the number of interactions cannot be negative")
    render = bool(getattr(args, "predicted_render", False))
    if render and not getattr(args, "predicted_sim", False):
        raise ValueError("--predicted_render needs --predicted_sim: the pictures are drawn by the predicted simulator")
    if getattr(args, "predicted_sim", False) and args.classifier_guidance and model.simulator is None:
        from ..dynamics.predicted import PredictedSimulator      # opt-in: the tables scored by the dynamics model instead of roll-outs
        model.object_mesh_dir = _object_mesh_dir(args) if render else None      # where --predicted_render finds <name>/model.obj
        model.simulator = PredictedSimulator(model, rollout_interactions=rollout, render_grippers=render)
    squeeze = squeeze_from_args(args)       # --squeeze_sim: refused with --fingers_3d, --predicted_sim, outside --mode=test
    if squeeze is not None and model.simulator is None:
        from ..sim.squeeze import SqueezeSimulator               # opt-in: the tables scored by the squeeze model (its own idealisation)
        model.simulator = SqueezeSimulator(model, **squeeze)
    squeeze3 = squeeze_3d_from_args(args)   # --squeeze_sim_3d: the sliced form for --fingers_3d, on the run's mesh files
    if squeeze3 is not None and model.simulator is None:
        from ..sim.squeeze import SqueezeSimulator3D
        model.simulator = SqueezeSimulator3D(model, object_mesh_dir=_object_mesh_dir(args), **squeeze3)
    if cond_stats is not None and cond_stats.source == 'squeeze_3d':
        model.object_mesh_dir = _object_mesh_dir(args)  # where the --cond_target report finds <name>/model.obj
    from ..goal import goal_from_args
    model.goal = goal_from_args(args)       # --goal_pose: the sweep adds a goal objective after the reference's (Diffusion._objective_sweep)
    if model.goal is not None and getattr(args, "predicted_sim", False) and not rollout:
        raise ValueError("--goal_pose with --predicted_sim needs --predicted_rollout K >= 1: a goal is scored on the pose the roll-out settles to")
    if args.mode != 'test':                 # generator/train.py:158-162
        if args.diffusion_checkpoint_path is not None:
            print('loading diffusion checkpoint from', args.diffusion_checkpoint_path)
            model.to(dev)
            model.load_checkpoint(torch.load(args.diffusion_checkpoint_path, map_location="cpu", weights_only=False))
        model.save_dir = args.save_dir or None
        return fit(model, pts, args, (0.12, -0.12, max_y, min_y), dev), []
    ck = _load_or_synth(args.diffusion_checkpoint_path, [("ema_nets.noise_pred_net." + k, s) for k, s in synth.unet_spec(global_cond_dim=gc)], 11,
                        "diffusion checkpoint")
    res = model.load_state_dict(ck)
    lost = [k for k in res.missing_keys if k.startswith("ema_nets.noise_pred_net.")]
    if lost or res.unexpected_keys:
        raise KeyError(f"diffusion checkpoint does not match ConditionalUnet1D: missing {lost[:5]}{'...' if len(lost) > 5 else ''}, "
                       f"unexpected {list(res.unexpected_keys)[:5]}")
    model.eval().to(dev)
    model.save_dir = args.save_dir or None
    if model.save_dir:
        os.makedirs(model.save_dir, exist_ok=True)
    results = []
    n_batches = len(dataset) // args.batch_size                       # DataLoader(drop_last=True), :69
    target_row = None
    if cond_stats is not None:              # --cond_target: one row in the labelling run's standardised units, broadcast to every batch
        model.cond_target = (cond_stats, cond_requested)
        target_row = torch.from_numpy(cond_stats.target(cond_requested))[None].expand(args.batch_size, -1).contiguous()
    with torch.no_grad():
        for bi in range(n_batches):
            ids = range(bi * args.batch_size, (bi + 1) * args.batch_size)
            if target_row is not None:
                batch = (torch.from_numpy(np.stack([dataset[i] for i in ids])), target_row)
            elif cond is None:
                batch = torch.from_numpy(np.stack([dataset[i] for i in ids]))
            else:
                batch = (torch.from_numpy(np.stack([dataset[i][0] for i in ids])), torch.from_numpy(cond[list(ids)]))
            res = model.validation_step(batch, bi)
            if int(os.environ.get("RANK", "0")) == 0:
                print(f"[dgdm_amd] batch {bi}: " + ", ".join(f"{k}={v:.5f}" for k, v in res["stats"].items()))
            results.append(res)
    return model, results


def main(argv=None):
    """Single process: one GPU.  Under torchrun (`torchrun --nproc-per-node N generator/train.py ...`): one rank per GPU, the
    guided chains sharded over the ranks (dgdm_amd/dist.py) where the reference wraps the classifier in nn.DataParallel (:86,88)."""
    from .. import _lib
    from .. import dist as ddist
    world, rank, local = ddist.init_from_env()
    _lib.device_init(local)
    try:
        train(parse(argv))
    finally:
        if world > 1:
            import torch.distributed as td
            td.destroy_process_group()


if __name__ == "__main__":
    main()
