"""Condition rows of the eps-net made by the dynamics model: what it predicts every finger of a set does, as ``global_cond`` rows.

``label_fingers`` runs ``engine.Guidance.label`` (and, with ``rollout=K``, ``label_settled``) over all fingers and returns the raw rows;
``label_fingers_squeeze`` makes the same columns from the squeeze simulator's closings instead, with no dynamics model (source 'squeeze'),
``label_fingers_squeeze_3d`` from the sliced squeeze of 3-D fingers on object meshes (source 'squeeze_3d');
``LabelStats`` remembers how a dataset's rows were standardised, so that a request in plain units - "clockwise on 90 % of the grid" -
becomes a condition row at sampling time (``LabelStats.target``).  The columns are those of include/dgdm_hip.h.

Model labels are the dynamics model's opinion, not simulator measurements, and in 3-D they depend on the FPS start seed like every
``cond_fn`` call.  Squeeze labels are the squeeze model's (sim/squeeze.py): this project's own idealisation, not MuJoCo's.
"""
from __future__ import annotations

import json
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np

TALLY_COLUMNS = ["frac_clockwise", "frac_counterclockwise", "frac_up", "frac_down", "frac_left", "frac_right",
                 "mean_rot", "mean_abs_rot", "mean_shift_x", "mean_shift_y"]
SETTLED_COLUMNS = ["settle_concentration", "settle_cos", "settle_sin", "settle_offset", "left_range"]
LAYOUTS = ("mean", "per_object")
MAX_COND_DIM = 256                 # the eps-net's global_cond_dim limit
# what a labelling run records beside the statistics (score_std: the dataset's (rad, m, m); K: roll-out interactions)
RECIPE_KEYS = ("G", "P", "ori_range", "threshold_std", "score_std", "K", "timestep", "seed", "contraction_dtype")
# who made the rows: the dynamics model (the key is absent from its files) or the squeeze simulator, whose files also record its recipe
# (threshold: the raw (rad, m, m) of squeeze_metric's classes; settled: the 5 settled columns were made)
# 'squeeze_3d': the sliced squeeze of 3-D fingers, which has no friction and records the finger grid it sliced on instead
SOURCES = ("model", "squeeze", "squeeze_3d")
SQUEEZE_RECIPE_KEYS = ("source", "squeeze_config", "friction", "settled", "threshold")
SQUEEZE_3D_RECIPE_KEYS = ("source", "squeeze_config", "sample_size", "width", "settled", "threshold")
SOURCE_RECIPE_KEYS = {"model": (), "squeeze": SQUEEZE_RECIPE_KEYS, "squeeze_3d": SQUEEZE_3D_RECIPE_KEYS}

_ROT_COLUMN = {"clockwise": "frac_clockwise", "counterclockwise": "frac_counterclockwise"}
_SHIFT_COLUMN = {"up": "frac_up", "down": "frac_down", "left": "frac_left", "right": "frac_right"}
# the 14 directional objective names -> the one or two fraction columns they ask for
ALIASES: Dict[str, List[str]] = {}
for _r, _rc in _ROT_COLUMN.items():
    ALIASES[f"rotate_{_r}"] = [_rc]
    for _s, _sc in _SHIFT_COLUMN.items():
        ALIASES[f"{_r}_{_s}"] = [_rc, _sc]
for _s, _sc in _SHIFT_COLUMN.items():
    ALIASES[f"shift_{_s}"] = [_sc]
_REFUSED = {"rotate": "'rotate' has no single column: name the two rotation fractions, frac_clockwise and frac_counterclockwise",
            "convergence": "'convergence' is not a tally column: use settle_concentration (label with --label_rollout K)"}


def block_columns(rollout: int) -> List[str]:
    return TALLY_COLUMNS + (SETTLED_COLUMNS if int(rollout) > 0 else [])


def column_names(layout: str, object_ids: Sequence[Any], rollout: int = 0) -> List[str]:
    """The row's column names: 'mean' the 10 (+5) names, 'per_object' ``<name>@<object id>`` object after object."""
    if layout not in LAYOUTS:
        raise ValueError(f"label layout {layout!r} not supported ({' or '.join(LAYOUTS)})")
    cols = block_columns(rollout)
    if layout == "mean":
        return list(cols)
    return [f"{c}@{o}" for o in object_ids for c in cols]


def cond_dim(layout: str, n_objects: int, rollout: int = 0) -> int:
    """Width of a row; ValueError for an unknown layout or more columns than the eps-net takes."""
    if layout not in LAYOUTS:
        raise ValueError(f"label layout {layout!r} not supported ({' or '.join(LAYOUTS)})")
    gc = len(block_columns(rollout)) * (1 if layout == "mean" else int(n_objects))
    if gc > MAX_COND_DIM:
        raise ValueError(f"label rows of {gc} columns ({n_objects} objects, layout {layout!r}): the eps-net takes at most {MAX_COND_DIM}")
    return gc


def label_fingers(guidance, fingers, objects: Sequence[int], threshold_std: Sequence[float], std: Optional[Sequence[float]] = None,
                  rollout: int = 0, layout: str = "mean", timestep: int = 0, seed: int = 0, chunk_batches: Optional[int] = None):
    """Raw rows (N, gc) float32 on the device for fingers (N, L[, 1]) in sampler units: gc = 10 (+5 with rollout = K > 0) for 'mean',
    M times that for 'per_object' (per object the tally block, then the settled block).  objects: indices into the handle's bank.
    3-D: the FPS start draws come from ``sampler.TorchRng(seed)``, batch after batch (a batch's tally draws, then its roll-out's);
    chunk_batches bounds how many batches' draws are held at once and does not change the rows.  A non-finite settled state raises
    ValueError naming the finger."""
    import torch
    from . import sampler
    K, M = int(rollout), len(objects)
    if K < 0:
        raise ValueError(f"label_fingers: rollout = {rollout} is negative")
    if K and std is None:
        raise ValueError("label_fingers: rollout needs std, the dataset's (rad, m, m)")
    gc = cond_dim(layout, M, K)
    x = torch.as_tensor(fingers).detach().to(device=torch.device("cuda", torch.cuda.current_device()), dtype=torch.float32)
    x = x.reshape(x.shape[0], -1).contiguous()
    N, B = x.shape[0], guidance.cfg.batch
    if N < 1:
        raise ValueError("label_fingers: no fingers")
    nb = -(-N // B)
    per = len(block_columns(K))
    rows = torch.empty((N, gc), dtype=torch.float32, device=x.device)
    three_d = guidance.dyn.kind == 3
    rng = sampler.TorchRng(seed=int(seed)) if three_d else None
    chunk = nb if not chunk_batches or not three_d else max(1, int(chunk_batches))
    for k0 in range(0, nb, chunk):
        k1 = min(nb, k0 + chunk)
        f0, f1 = k0 * B, min(N, k1 * B)
        st_t = st_s = None
        if three_d:
            pts, sub = guidance.cfg.num_object_points, guidance.cfg.sub_batch_size
            st_t = np.empty((k1 - k0, M, guidance.starts_per_call), dtype=np.int64)
            st_s = np.empty((k1 - k0, K, M, 2 * guidance.sweep_rows), dtype=np.int64) if K else None
            for k in range(k1 - k0):
                rng.fps_starts(pts, sub, guidance.rows, n_calls=M, out=st_t[k])
                if K:
                    rng.fps_starts(pts, sub, guidance.sweep_rows, n_calls=K * M, out=st_s[k].reshape(K * M, -1))
        # the last chunk's padding repeats finger N - 1 of the WHOLE set, which is also the chunk's last finger
        part = rows[f0:f1]
        guidance.label(x[f0:f1], objects, threshold_std, timestep=timestep, starts=st_t, layout=layout, out=part, column_offset=0, object_stride=per)
        if K:
            guidance.label_settled(x[f0:f1], objects, std, K, starts=st_s, layout=layout, out=part, column_offset=10, object_stride=per)
    if K:
        bad = torch.isnan(rows).any(dim=1)
        if bool(bad.any()):
            raise ValueError(f"label_fingers: the roll-out of finger {int(torch.nonzero(bad)[0])} reached a non-finite state (its settled columns are NaN)")
    return rows


def label_fingers_squeeze(fingers, contours, objects: Sequence[int], grid_size: int, num_pos: int, ori_range: Sequence[float],
                          threshold: Sequence[float], score_std: Sequence[float], settled: bool = False, layout: str = "mean", friction: float = 0.0,
                          num_points: int = 200, **squeeze_config):
    """The same rows made by the squeeze simulator instead of the dynamics model (engine.squeeze_label; include/dgdm_hip.h
    "squeeze-simulator labels", DESIGN.md 4.1b "source: squeeze"): no model, no checkpoint, no random draw.  fingers (N, L[, 1]) in sampler
    units; contours (O, nv, 2) float64 polygons in metres; objects: indices into contours.  The tally starts are the pose grid's cells
    (resample.start_grid(G, P, ori_range)), one closing each; with settled=True the G start orientations (sim.squeeze.start_orientations)
    follow, each run until it settles, and the rows carry the 5 settled columns.  threshold: raw (rad, m, m), squeeze_metric's classes;
    score_std: the dataset's (rad, m, m).  -> (rows (N, gc) float32 on the device, counts (N, 3) int32 on the device: per finger the
    tally (object, start)s that were loose at the start, ended loose, and were cut by the table's x range).  The fingers are decoded and
    run in chunks of as many as one workspace holds, so only one chunk's surfaces exist at a time; the chunking does not change the rows.
    The simulator's opinion: frictionless unless friction > 0, its steps, window, friction and these thresholds untuned for squeeze
    deltas; nothing is claimed about MuJoCo.  NaN settled columns raise ValueError naming the finger."""
    import ctypes as C
    import torch
    from . import engine
    from .resample import start_grid
    from .sim import squeeze as sq
    M = len(objects)
    gc = cond_dim(layout, M, 1 if settled else 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(fingers).detach().to(device=dev, dtype=torch.float32)
    x = x.reshape(x.shape[0], -1).contiguous()
    N = x.shape[0]
    if N < 1:
        raise ValueError("label_fingers_squeeze: no fingers")
    if M < 1:
        raise ValueError("label_fingers_squeeze: no objects")
    mu = sq.check_friction(friction, "label_fingers_squeeze")
    tally = start_grid(grid_size, num_pos, ori_range)
    starts = np.concatenate([tally, sq.start_orientations(grid_size, ori_range)]) if settled else tally
    cfg = engine.squeeze_config(**squeeze_config)
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
    bank, st, rot = f64(torch.as_tensor(contours).detach().cpu().numpy()), f64(starts), f64(engine.squeeze_rotation_table(cfg.theta_cells))
    sizer = lambda n: int(engine.lib().dgdm_squeeze_label_workspace_bytes(C.byref(cfg), n, M, int(mu > 0.0)))      # noqa: E731
    one = sizer(1)
    if one < 0:
        engine._check_value(one)
    chunk = max(1, min(N, engine.SQUEEZE_WORKSPACE_BYTES // one, 65535 // M))
    rows = torch.empty((N, gc), dtype=torch.float32, device=dev)
    counts = torch.empty((N, 3), dtype=torch.int32, device=dev)
    per = len(block_columns(1 if settled else 0))
    for f0 in range(0, N, chunk):
        f1 = min(N, f0 + chunk)
        sf = sq.finger_surfaces(x[f0:f1], int(num_points))
        _, cnt = engine.squeeze_label(sf, bank, objects, st, len(tally), threshold, score_std, layout=layout, friction=mu, rot=rot, out=rows[f0:f1],
                                      object_stride=per, workspace_bytes=sizer(f1 - f0), **squeeze_config)
        counts[f0:f1] = cnt
    if settled:
        bad = torch.isnan(rows).any(dim=1)
        if bool(bad.any()):
            raise ValueError(f"label_fingers_squeeze: finger {int(torch.nonzero(bad)[0])} settled on a non-finite pose (its settled columns are NaN)")
    return rows, counts


def label_fingers_squeeze_3d(fingers, meshes, objects: Sequence[int], grid_size: int, num_pos: int, ori_range: Sequence[float],
                             threshold: Sequence[float], score_std: Sequence[float], settled: bool = False, layout: str = "mean",
                             sample_size: int = 25, width: Optional[float] = None, **squeeze_config):
    """label_fingers_squeeze for 3-D fingers (engine.squeeze_label_3d; include/dgdm_hip.h "squeeze-simulator labels, 3-D fingers",
    DESIGN.md 4.1b "source: squeeze_3d"): fingers (N, 42[, 1]) in sampler units; meshes a sequence of (vertices (nv, 3) in metres,
    triangles (nt, 3)) standing on z = 0; objects: indices into meshes.  The starts, threshold, score_std, settled, layout and the
    returned (rows, counts) are label_fingers_squeeze's.  The meshes are sliced once, on the levels gz of the first chunk's decode (the
    finger grid's z depends on the v index only, so every chunk has the same); the fingers are decoded chunk by chunk
    (sim.squeeze.finger_surfaces_3d with sample_size and width).  The sliced squeeze's opinion: blind between two levels, frictionless,
    its steps, window and these thresholds untuned; nothing is claimed about MuJoCo.  NaN settled columns raise ValueError naming the
    finger."""
    import ctypes as C
    import torch
    from . import engine
    from .resample import start_grid
    from .sim import squeeze as sq
    M, n = len(objects), int(sample_size)
    gc = cond_dim(layout, M, 1 if settled else 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(fingers).detach().to(device=dev, dtype=torch.float32)
    x = x.reshape(x.shape[0], -1).contiguous()
    N = x.shape[0]
    if N < 1:
        raise ValueError("label_fingers_squeeze_3d: no fingers")
    if M < 1:
        raise ValueError("label_fingers_squeeze_3d: no objects")
    meshes = list(meshes)
    w = sq.FINGER_WIDTH_3D if width is None else float(width)
    tally = start_grid(grid_size, num_pos, ori_range)
    starts = np.concatenate([tally, sq.start_orientations(grid_size, ori_range)]) if settled else tally
    cfg = engine.squeeze_config(**squeeze_config)
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
    st, rot = f64(starts), f64(engine.squeeze_rotation_table(cfg.theta_cells))
    sizer = lambda k: int(engine.lib().dgdm_squeeze_label_3d_workspace_bytes(C.byref(cfg), k, M, n, n, max(len(meshes), 1)))      # noqa: E731
    one = sizer(1)
    if one < 0:
        engine._check_value(one)
    chunk = max(1, min(N, engine.SQUEEZE_WORKSPACE_BYTES // one, 65535 // M))
    rows = torch.empty((N, gc), dtype=torch.float32, device=dev)
    counts = torch.empty((N, 3), dtype=torch.int32, device=dev)
    per = len(block_columns(1 if settled else 0))
    sl = None
    for f0 in range(0, N, chunk):
        f1 = min(N, f0 + chunk)
        gx, gz, sf = sq.finger_surfaces_3d(x[f0:f1], n, w)
        if sl is None:
            sl = engine.squeeze_slice(meshes, gz)
        _, cnt = engine.squeeze_label_3d(sf, gx, sl["segments"], sl["offsets"], objects, st, len(tally), threshold, score_std, layout=layout, rot=rot,
                                         out=rows[f0:f1], object_stride=per, workspace_bytes=sizer(f1 - f0), **squeeze_config)
        counts[f0:f1] = cnt
    if settled:
        bad = torch.isnan(rows).any(dim=1)
        if bool(bad.any()):
            raise ValueError(f"label_fingers_squeeze_3d: finger {int(torch.nonzero(bad)[0])} settled on a non-finite pose (its settled columns are NaN)")
    return rows, counts


def parse_target(text: str) -> Dict[str, float]:
    """``"frac_clockwise=0.9,frac_up=0.7"`` -> {'frac_clockwise': 0.9, 'frac_up': 0.7}; ValueError on anything else."""
    out: Dict[str, float] = {}
    for item in str(text).split(","):
        name, eq, val = item.partition("=")
        name = name.strip()
        try:
            v = float(val)
        except ValueError:
            v = float("nan")
        if not eq or not name or not np.isfinite(v):
            raise ValueError(f"--cond_target: '{item.strip()}' is not NAME=NUMBER")
        if name in out:
            raise ValueError(f"--cond_target: '{name}' is set twice")
        out[name] = v
    return out


class LabelStats:
    """How a dataset's raw label rows were standardised, and the recipe that made them.  ``fit(raw)`` -> per-column mean and std in
    numpy float64 (a column of std 0 is flagged in ``constant`` and standardises to 0); ``apply(raw)`` -> float32 ``(v - mean) / std``;
    ``target({...})`` -> one row for sampling; ``save`` / ``load``: a JSON file."""

    def __init__(self, columns: Sequence[str], layout: str = "mean", object_ids: Sequence[Any] = (), recipe: Optional[Mapping[str, Any]] = None):
        if layout not in LAYOUTS:
            raise ValueError(f"label layout {layout!r} not supported ({' or '.join(LAYOUTS)})")
        self.columns = [str(c) for c in columns]
        self.layout = layout
        self.object_ids = list(object_ids)
        self.recipe: Dict[str, Any] = dict(recipe or {})
        n = len(self.columns)
        self.mean, self.std = np.zeros(n), np.ones(n)
        self.min, self.max = np.zeros(n), np.zeros(n)

    @property
    def dim(self) -> int:
        return len(self.columns)

    @property
    def source(self) -> str:
        """'model' (also when the recipe does not say), 'squeeze' or 'squeeze_3d'."""
        return self.recipe.get("source") or "model"

    @property
    def constant(self) -> np.ndarray:
        return self.std == 0.0

    def fit(self, raw) -> "LabelStats":
        r = np.asarray(raw, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != self.dim or r.shape[0] < 1:
            raise ValueError(f"LabelStats.fit: rows of shape {r.shape} for {self.dim} columns")
        if not np.isfinite(r).all():
            raise ValueError(f"LabelStats.fit: non-finite value in row {int(np.argwhere(~np.isfinite(r))[0][0])}")
        self.mean, self.std = r.mean(axis=0), r.std(axis=0)
        self.min, self.max = r.min(axis=0), r.max(axis=0)
        return self

    def _standardise(self, r: np.ndarray) -> np.ndarray:
        safe = np.where(self.constant, 1.0, self.std)
        return np.where(self.constant, 0.0, (r - self.mean) / safe)

    def apply(self, raw) -> np.ndarray:
        r = np.asarray(raw, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != self.dim:
            raise ValueError(f"LabelStats.apply: rows of shape {r.shape} for {self.dim} columns")
        return self._standardise(r).astype(np.float32)

    def resolve(self, name: str) -> List[int]:
        """The column indices a target name sets: a column, a bare name (every object's column in 'per_object'), an objective alias."""
        if name in _REFUSED:
            raise ValueError(f"cond target: {_REFUSED[name]}")
        if name in self.columns:
            return [self.columns.index(name)]
        bare, at, obj = name.partition("@")
        names = ALIASES.get(bare, [bare])
        idx = [i for n in names for i, c in enumerate(self.columns) if c == (f"{n}@{obj}" if at else n) or (not at and c.startswith(n + "@"))]
        if not idx or any(n not in TALLY_COLUMNS + SETTLED_COLUMNS for n in names):
            raise ValueError(f"cond target: unknown column '{name}' (columns: {', '.join(self.columns[:15])}{', ...' if self.dim > 15 else ''}; "
                             f"objective aliases: {', '.join(sorted(ALIASES))})")
        return idx

    def requested(self, target: Mapping[str, float]) -> Dict[str, float]:
        """The target by column name, in raw units, aliases and bare names resolved."""
        out: Dict[str, float] = {}
        for name, v in target.items():
            for i in self.resolve(str(name)):
                out[self.columns[i]] = float(v)
        return out

    def target(self, target: Mapping[str, float]) -> np.ndarray:
        """One float32 row (dim,): the named columns standardised from raw units, every other column 0 - the dataset mean."""
        raw = self.mean.copy()
        for c, v in self.requested(target).items():
            raw[self.columns.index(c)] = v
        return self._standardise(raw[None])[0].astype(np.float32)

    def to_dict(self) -> Dict[str, Any]:
        return {"columns": self.columns, "mean": self.mean.tolist(), "std": self.std.tolist(), "min": self.min.tolist(), "max": self.max.tolist(),
                "layout": self.layout, "object_ids": [o.item() if isinstance(o, np.generic) else o for o in self.object_ids],
                **{k: self.recipe.get(k) for k in RECIPE_KEYS},
                **({"predicted": True} if self.source == "model" else
                   {**{k: self.recipe.get(k) for k in SOURCE_RECIPE_KEYS.get(self.source, SQUEEZE_RECIPE_KEYS)}, "simulated": "squeeze"})}

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=1)

    @classmethod
    def load(cls, path: str) -> "LabelStats":
        try:
            with open(path) as f:
                d = json.load(f)
            source = d.get("source") or "model"
            if source not in SOURCES:
                raise ValueError(f"label source {source!r} (need one of {', '.join(SOURCES)})")
            s = cls(d["columns"], d["layout"], d["object_ids"],
                    {k: d.get(k) for k in RECIPE_KEYS + SOURCE_RECIPE_KEYS[source]})
            s.mean, s.std = np.asarray(d["mean"], dtype=np.float64), np.asarray(d["std"], dtype=np.float64)
            s.min, s.max = np.asarray(d["min"], dtype=np.float64), np.asarray(d["max"], dtype=np.float64)
        except (OSError, KeyError, TypeError, ValueError) as e:
            raise ValueError(f"--cond_stats: cannot read '{path}' as label statistics ({type(e).__name__}: {e})")
        if not (len(s.mean) == len(s.std) == len(s.min) == len(s.max) == s.dim) or not 1 <= s.dim <= MAX_COND_DIM:
            raise ValueError(f"--cond_stats: '{path}' holds {s.dim} columns and statistics of {len(s.mean)}, {len(s.std)}, {len(s.min)}, {len(s.max)} entries")
        return s
