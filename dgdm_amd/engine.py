"""Python handles over the C-ABI objects of libdgdm_hip.so.

PyTorch supplies device memory and the stream; every computation is a HIP kernel behind
``include/dgdm_hip.h``.  These classes are what the reference-shaped modules in
``dgdm_amd.generator`` / ``dgdm_amd.dynamics`` delegate to.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, lib, stream_ptr


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(dtype=torch.float32).contiguous()


def check_global_cond(global_cond: Optional[torch.Tensor], gc: int, rows: int, what: str = "global_cond") -> Optional[torch.Tensor]:
    """The condition rows of `rows` samples for an eps-net of global_cond_dim `gc`: (rows, gc) or None when gc == 0 and none is given.
    Host-side validation only (no library call, no launch); raises ValueError for a missing condition, a wrong width or row count."""
    if gc == 0:
        if global_cond is not None:
            raise ValueError(f"{what}: this eps-net has global_cond_dim 0 and takes no condition")
        return None
    if global_cond is None:
        raise ValueError(f"{what}: this eps-net has global_cond_dim {gc} and needs a condition of shape ({rows}, {gc})")
    if global_cond.dim() != 2 or global_cond.shape[1] != gc:
        raise ValueError(f"{what}: expected width {gc} (shape ({rows}, {gc})), got shape {tuple(global_cond.shape)}")
    if global_cond.shape[0] != rows:
        raise ValueError(f"{what}: expected {rows} rows (one per sample), got {global_cond.shape[0]}")
    return global_cond


def chain_cond_layout(global_cond: Optional[torch.Tensor], gc: int, n_chains: int, batch: int):
    """The chain runner's view of a condition: (B, gc) shared by all chains -> (tensor, 0); (n_chains, B, gc) -> (tensor, B * gc).
    Host-side validation only; raises ValueError."""
    if gc == 0 or global_cond is None:
        check_global_cond(global_cond, gc, batch)
        return None, 0
    if global_cond.dim() == 2:
        return check_global_cond(global_cond, gc, batch), 0
    if global_cond.dim() != 3 or tuple(global_cond.shape) != (n_chains, batch, gc):
        raise ValueError(f"global_cond: expected ({batch}, {gc}) or ({n_chains}, {batch}, {gc}), got shape {tuple(global_cond.shape)}")
    return global_cond, batch * gc


def cfg_mix(eps_c: torch.Tensor, eps_u: torch.Tensor, w: float) -> torch.Tensor:
    """Classifier-free guidance mix eps_u + w (eps_c - eps_u), three separately rounded float32 operations (dgdm_cfg_mix)."""
    ec, eu = _f32(eps_c), _f32(eps_u)
    if ec.shape != eu.shape:
        raise ValueError(f"cfg_mix: shapes differ ({tuple(ec.shape)} and {tuple(eu.shape)})")
    out = torch.empty_like(ec)
    check(lib().dgdm_cfg_mix(dptr(ec), dptr(eu), float(w), dptr(out), ec.numel(), stream_ptr()))
    return out


class Unet1d:
    """``ConditionalUnet1D`` weights packed on the device (generator/diffusion_utils.py:123-285)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], down_dims: Sequence[int] = (128, 256), step_embed_dim: int = 32,
                 kernel_size: int = 5, n_groups: int = 8, contraction_dtype: str = "f32"):
        packed = _lib.PackedStateDict(state_dict)
        dd = (C.c_int32 * len(down_dims))(*down_dims)
        h = C.c_void_p()
        check(lib().dgdm_unet1d_create(C.byref(h), packed.array, packed.n, dd, len(down_dims), step_embed_dim, kernel_size, n_groups))
        self._h = h
        self.global_cond_dim = int(lib().dgdm_unet1d_global_cond_dim(h))
        self.set_contraction_dtype(contraction_dtype)

    def set_contraction_dtype(self, dtype: str) -> None:
        """Arithmetic of the multi-channel convolutions: 'f32' (default, the parity path: float32-grade, every product as three f16 MFMA
        products on exactly scaled two-way split operands, csrc/unet.hip conv_mfma_f16x3; 'f32_f16x3' names the same form), 'f32_mfma' (the float32 MFMA chain of rounds 1-3) or 'bf16' (operands ROUNDED to bf16)."""
        codes = {"f32": 0, "bf16": 1, "f32_mfma": 2, "f32_f16x3": 3}
        if dtype not in codes:
            raise ValueError(f"contraction dtype {dtype!r} not supported")
        check(lib().dgdm_unet1d_set_contraction_dtype(self._h, codes[dtype]))
        self.contraction_dtype = dtype

    def effective_form(self, batch: int, num_points: int):
        """(arithmetic, batched) a forward of `batch` samples of `num_points` control points actually runs: arithmetic is 'f32_f16x3',
        'f32_mfma' (also what 'f32' falls back to where the split form's slabs do not fit the LDS: L = 44, 46) or 'bf16'; batched says
        whether the layer-by-layer form for large batches is used (same bits as the per-sample kernel)."""
        code = int(lib().dgdm_unet1d_effective_form(self._h, int(batch), int(num_points)))
        if code < 0:
            raise ValueError("bad batch / num_points")
        return {1: "bf16", 2: "f32_mfma", 3: "f32_f16x3"}[code & 15], bool(code & 16)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # module globals are None during interpreter shutdown
            lib().dgdm_unet1d_destroy(self._h)
            self._h = None

    def forward(self, sample: torch.Tensor, timestep: torch.Tensor, global_cond: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sample (B, L, 1) float32 cuda, timestep (B,) integer, global_cond (B, global_cond_dim) or None -> eps (B, L, 1)."""
        assert sample.dim() == 3 and sample.shape[-1] == 1, "input_dim must be 1 (generator/train.py:76)"
        c = check_global_cond(global_cond, self.global_cond_dim, sample.shape[0])
        x = _f32(sample)
        B, L, _ = x.shape
        t = timestep.to(device=x.device, dtype=torch.int32).expand(B).contiguous()
        out = torch.empty_like(x)
        if c is None:
            check(lib().dgdm_unet1d_forward(self._h, dptr(x), dptr(t), dptr(out), B, L, stream_ptr()))
        else:
            c = _f32(c).to(x.device)
            check(lib().dgdm_unet1d_forward_cond(self._h, dptr(x), dptr(t), dptr(c), dptr(out), B, L, stream_ptr()))
        return out

    def forward_cfg(self, sample: torch.Tensor, timestep: torch.Tensor, global_cond: Optional[torch.Tensor] = None, cfg_weight: float = 1.0) -> torch.Tensor:
        """eps under classifier-free guidance, as dgdm_guided_chains_run_cond forms it: weight 1 (or no condition) -> the conditional
        eps, 0 -> the eps of the all-zero condition, otherwise ONE forward of 2B samples [condition rows | zero rows] and the mix."""
        w = float(cfg_weight)
        if self.global_cond_dim == 0 or w == 1.0:
            return self.forward(sample, timestep, global_cond)
        c = check_global_cond(global_cond, self.global_cond_dim, sample.shape[0])
        if w == 0.0:
            return self.forward(sample, timestep, torch.zeros_like(c))
        B = sample.shape[0]
        t = timestep.to(device=sample.device).expand(B)
        both = self.forward(torch.cat((sample, sample)), torch.cat((t, t)), torch.cat((c, torch.zeros_like(c))))
        return cfg_mix(both[:B], both[B:], w)


class UnetTrainer:
    """Training state of the eps-net on the device (csrc/unet_train.hip): parameters, gradients, Adam moments and the EMA copy, with
    one call per ``Diffusion.get_stats`` + backward + ``torch.optim.Adam`` step (generator/diffusion.py:126-177, 711-724)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_points: int, down_dims: Sequence[int] = (128, 256), step_embed_dim: int = 32,
                 kernel_size: int = 5, n_groups: int = 8, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        self._keys = {k: tuple(v.shape) for k, v in state_dict.items()}
        packed = _lib.PackedStateDict(state_dict)
        dd = (C.c_int32 * len(down_dims))(*down_dims)
        h = C.c_void_p()
        check(lib().dgdm_unet_trainer_create(C.byref(h), packed.array, packed.n, num_points, dd, len(down_dims), step_embed_dim, kernel_size, n_groups,
                                             betas[0], betas[1], eps, weight_decay))
        self._h, self.num_points = h, num_points
        self.global_cond_dim = int(lib().dgdm_unet_trainer_global_cond_dim(h))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib().dgdm_unet_trainer_destroy(self._h)
            self._h = None

    def _args(self, x0, noise, sqrt_abar, sqrt_1m_abar, timesteps):
        dev = torch.device("cuda", torch.cuda.current_device())
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
        x0, noise = f(x0).reshape(x0.shape[0], -1), f(noise).reshape(x0.shape[0], -1)
        assert x0.shape[1] == self.num_points and noise.shape == x0.shape
        return x0, noise, f(sqrt_abar), f(sqrt_1m_abar), timesteps.detach().to(device=dev, dtype=torch.int64).contiguous()

    def _cond(self, global_cond, rows: int):
        c = check_global_cond(global_cond, self.global_cond_dim, rows)
        if c is None:
            return None
        return c.detach().to(device=torch.device("cuda", torch.cuda.current_device()), dtype=torch.float32).contiguous()

    def step(self, x0, noise, sqrt_abar, sqrt_1m_abar, timesteps, lr: float, want_pred: bool = False, want_loss: bool = True, global_cond=None):
        """One optimisation step; returns (loss or None, noise_pred (B, L, 1) or None).  global_cond: (B, global_cond_dim) rows."""
        c = self._cond(global_cond, x0.shape[0])
        a = self._args(x0, noise, sqrt_abar, sqrt_1m_abar, timesteps)
        B = a[0].shape[0]
        pred = torch.empty_like(a[0]) if want_pred else None
        loss = C.c_float()
        check(lib().dgdm_unet_trainer_step_cond(self._h, *[dptr(v) for v in a], dptr(c), B, float(lr), dptr(pred), C.byref(loss) if want_loss else None,
                                                stream_ptr()))
        return (float(loss.value) if want_loss else None), (pred.reshape(B, -1, 1) if want_pred else None)

    def forward_backward(self, x0, noise, sqrt_abar, sqrt_1m_abar, timesteps, total_samples: Optional[int] = None, backward: bool = True,
                         want_pred: bool = False, global_cond=None):
        c = self._cond(global_cond, x0.shape[0])
        a = self._args(x0, noise, sqrt_abar, sqrt_1m_abar, timesteps)
        B = a[0].shape[0]
        pred = torch.empty_like(a[0]) if want_pred else None
        loss = C.c_float()
        check(lib().dgdm_unet_trainer_forward_backward_cond(self._h, *[dptr(v) for v in a], dptr(c), B, int(total_samples or B), 1 if backward else 0,
                                                            dptr(pred), C.byref(loss), stream_ptr()))
        return float(loss.value), (pred.reshape(B, -1, 1) if want_pred else None)

    def gradient_count(self) -> int:
        return int(lib().dgdm_unet_trainer_gradient_count(self._h))

    def read_gradients(self) -> torch.Tensor:
        flat = torch.empty(self.gradient_count(), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
        check(lib().dgdm_unet_trainer_gradients(self._h, dptr(flat), flat.numel(), 0, 1.0, stream_ptr()))
        return flat

    def write_gradients(self, flat: torch.Tensor, scale: float = 1.0) -> None:
        check(lib().dgdm_unet_trainer_gradients(self._h, dptr(flat), flat.numel(), 1, float(scale), stream_ptr()))

    def apply(self, lr: float) -> None:
        check(lib().dgdm_unet_trainer_apply(self._h, float(lr), stream_ptr()))

    def ema_step(self, decay: float) -> None:
        check(lib().dgdm_unet_trainer_ema_step(self._h, float(decay), float(1 - decay), stream_ptr()))

    def steps(self) -> int:
        return int(lib().dgdm_unet_trainer_steps(self._h))

    def export(self, which: int = 0) -> Dict[str, torch.Tensor]:
        """which: 0 parameters, 1 gradients, 2 / 3 Adam's exp_avg / exp_avg_sq, 4 the EMA copy (host tensors, the U-Net's own keys)."""
        host = {k: torch.empty(shp, dtype=torch.float32) for k, shp in self._keys.items()}
        packed = _lib.PackedStateDict(host)
        check(lib().dgdm_unet_trainer_export(self._h, which, packed.array, packed.n))
        return {n.decode(): torch.from_numpy(a.copy()).reshape(self._keys[n.decode()]) for n, a in zip(packed.names, packed.keep)}

    def load(self, which: int, state_dict: Dict[str, torch.Tensor], adam_steps: int = -1) -> None:
        packed = _lib.PackedStateDict(state_dict)
        check(lib().dgdm_unet_trainer_import(self._h, which, packed.array, packed.n, adam_steps))


class Dynamics:
    """``ProfileForward2DModel`` (kind 2) / ``ProfileForward3DModel`` (kind 3) on the device."""

    def __init__(self, kind: int, state_dict: Dict[str, torch.Tensor], params_ch: int, object_ch: int = 0):
        packed = _lib.PackedStateDict(state_dict)
        h = C.c_void_p()
        check(lib().dgdm_dynamics_create(C.byref(h), kind, packed.array, packed.n, params_ch, object_ch))
        self._h, self.kind, self.params_ch, self.object_ch = h, kind, params_ch, object_ch

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # module globals are None during interpreter shutdown
            lib().dgdm_dynamics_destroy(self._h)
            self._h = None

    def forward2d(self, x_ctrl, x_ori, x_pos, timesteps, object_vertices) -> torch.Tensor:
        rows = x_ctrl.shape[0]
        a = [_f32(v) for v in (x_ctrl, x_ori, x_pos, timesteps, object_vertices)]
        out = torch.empty((rows, 3), dtype=torch.float32, device=a[0].device)
        check(lib().dgdm_dyn2d_forward(self._h, *[dptr(v) for v in a], dptr(out), rows, stream_ptr()))
        return out

    @staticmethod
    def _starts(s: torch.Tensor) -> np.ndarray:
        return np.ascontiguousarray(s.detach().cpu().numpy().astype(np.int64))

    def pointnet2(self, xyz: torch.Tensor, start_sa1: torch.Tensor, start_sa2: torch.Tensor) -> torch.Tensor:
        """xyz (rows, 3, N) -> (rows, 256)."""
        x = _f32(xyz)
        rows, _, N = x.shape
        s1, s2 = self._starts(start_sa1), self._starts(start_sa2)
        out = torch.empty((rows, 256), dtype=torch.float32, device=x.device)
        check(lib().dgdm_pointnet2_forward(self._h, dptr(x), s1.ctypes.data, s2.ctypes.data, dptr(out), rows, N, stream_ptr()))
        return out

    def forward3d(self, x_ctrl, x_ori, x_pos, timesteps, xyz, start_sa1, start_sa2) -> torch.Tensor:
        rows, _, N = xyz.shape
        a = [_f32(v) for v in (x_ctrl, x_ori, x_pos, timesteps, xyz)]
        s1, s2 = self._starts(start_sa1), self._starts(start_sa2)
        out = torch.empty((rows, 3), dtype=torch.float32, device=a[0].device)
        check(lib().dgdm_dyn3d_forward(self._h, *[dptr(v) for v in a], s1.ctypes.data, s2.ctypes.data, dptr(out), rows, N, stream_ptr()))
        return out


def debug_pointnet_indices(dyn: "Dynamics", cloud: torch.Tensor, perm: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
    """Test hook: the index decisions of the PointNet++ pipeline for one cloud (N, 3) - FPS sequences from every start index,
    sa1's 32-neighbour lists, sa2's first-64 lists for the candidate order `perm` (default: index order), crowded flags."""
    x = _f32(cloud)
    N = x.shape[0]
    pm = (torch.arange(N) if perm is None else perm).to(device=x.device, dtype=torch.int32).contiguous()
    mk = lambda *shape: torch.empty(shape, dtype=torch.int32, device=x.device)       # noqa: E731
    out = dict(fps512=mk(N, 512), fps128=mk(N, 128), fps128_flags=mk(N), ball1=mk(N, 32), ball2=mk(N, 64), ball2_count=mk(N), crowded=mk(N))
    check(lib().dgdm_debug_pointnet_indices(dyn._h, dptr(x), N, dptr(pm), pm.numel(), *[dptr(v) for v in out.values()], stream_ptr()))
    return {k: v.cpu().numpy() for k, v in out.items()}


def make_objective(name: Optional[str], object_index: int = 0, row_field: bool = False, lin: Sequence[float] = (0.0, 0.0, 0.0),
                   quad: Sequence[float] = (0.0, 0.0, 0.0)) -> _lib.Objective:
    """The objective of a reference name - or, with row_field=True (name None), a row-field objective (include/dgdm_hip.h
    DGDM_OBJ_ROWFIELD): d objective / d delta_j of row r = lin[j] + 2 quad[j] delta_j + field[r][j], the field being the one given to
    Guidance.set_row_field at the chain's index of the launch."""
    o = _lib.Objective()
    o.object = object_index
    if row_field:
        if name is not None:
            raise ValueError("a row-field objective has no reference name (pass name=None)")
        for j in range(3):
            o.lin[j], o.quad[j] = float(lin[j]), float(quad[j])
        o.use_rowcoef = _lib.OBJ_ROWFIELD
        return o
    check(lib().dgdm_objective_from_name(name.encode(), C.byref(o)))
    return o


class Guidance:
    """State of ``Diffusion.cond_fn`` for up to ``max_chains`` chains (generator/diffusion.py:473-504)."""

    def __init__(self, dyn: Dynamics, batch: int, grid_size: int, num_pos: int, ori_range: Sequence[float], max_chains: int,
                 num_train_timesteps: int, num_object_points: int, sub_batch_size: int = 0, max_objects: int = 8,
                 contraction_dtype: str = "f32"):
        cfg = _lib.GuidanceConfig(batch, grid_size, num_pos, float(ori_range[0]), float(ori_range[1]), max_chains,
                                  num_train_timesteps, sub_batch_size, num_object_points, max_objects)
        h = C.c_void_p()
        check(lib().dgdm_guidance_create(C.byref(h), dyn._h, C.byref(cfg)))
        self._h, self.dyn, self.cfg = h, dyn, cfg
        self.rows = int(lib().dgdm_guidance_rows(h))
        self.starts_per_call = int(lib().dgdm_guidance_starts_per_call(h))
        self.sweep_rows = batch * grid_size
        self.n_objects = 0
        self._row_field: Optional[torch.Tensor] = None      # set_row_field keeps the tensor the library points at
        self.set_contraction_dtype(contraction_dtype)

    def set_contraction_dtype(self, dtype: str) -> None:
        """Arithmetic of the trunk of cond_fn: 'f32' (default, = 'f32_f16x3': float32 operands as two exactly scaled f16 pieces, three f16
        MFMAs per product, float32 accumulation - float32-grade, csrc/trunk_f16l.hip), 'f32_mfma' (the k-ordered float32 MFMA chain,
        csrc/trunk.hip) or 'bf16' (operands ROUNDED to bf16, float32 accumulation)."""
        codes = {"f32": 0, "bf16": 1, "f32_mfma": 2, "f32_f16x3": 3}
        if dtype not in codes:
            raise ValueError(f"contraction dtype {dtype!r} not supported")
        check(lib().dgdm_guidance_set_contraction_dtype(self._h, codes[dtype]))
        self.contraction_dtype = dtype

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:      # module globals are None during interpreter shutdown
            lib().dgdm_guidance_destroy(self._h)
            self._h = None

    def set_objects(self, objects: torch.Tensor, wait: bool = False) -> None:
        """2-D: (n, V, 2); 3-D: (n, N, 3).  The table build (3-D) is enqueued on the handle's build streams and the call returns: like
        every other call of the handle it is ordered by the stream - the coordinates are copied into the handle's pool by a device
        copy on the current stream before anything else reads them (so `objects` is only needed by that enqueued copy, the contract
        of any asynchronous call; torch's allocator keeps a freed block for work on the same stream), the build streams start behind
        everything already enqueued on the current stream (chains still reading the previous tables included), and every call of the
        handle that reads the tables makes its stream wait for the build.  Other work that follows on the current stream does NOT
        wait: the first step's eps-net and per-finger tables run beside the build.  The host is free to convert and sort the next
        chains' FPS draws while the tables are being built (`dgdm_guided_chains_run` waits for the build's read-back only when it
        needs it).  `wait=True` blocks until the tables exist (the build streams are not the current stream: it waits for the
        device)."""
        o = _f32(objects)
        check(lib().dgdm_guidance_set_objects(self._h, dptr(o), o.shape[0], stream_ptr()))
        self._objects_ref = o                            # `o` may be a temporary: it is read by the copy still in flight
        if wait:
            torch.cuda.synchronize()
        self.n_objects = o.shape[0]

    def debug_fps_path(self, mode):
        """Test hook: where a reference row's PointNet++ embedding comes from.  0 / False: default ((chain, s1)-group gather kernel
        until the objects have served more than 5 cond_fn calls, then the per-object embedding table and no gather at all); 5: the
        next set_objects builds the embedding tables right away; 3: always the group gather kernel; 2: per-row table kernel;
        1 / True: every row runs its own FPS(128); 4: like 0, and the next set_objects builds the crowded centres' features with
        global gathers.  All must agree bit for bit.  Returns which objects are admissible for the table path."""
        ok = (C.c_int32 * max(1, self.n_objects))()
        check(lib().dgdm_guidance_debug_fps_path(self._h, int(mode), ok))
        return [bool(v) for v in ok][:self.n_objects]

    def debug_partials(self, n_chains: int) -> torch.Tensor:
        """Test hook: per-tile partial sums of d objective / d z1 of the last grad() call -> (n_chains, B, tiles_per_finger, W1)."""
        tp, w = C.c_int32(), C.c_int32()
        check(lib().dgdm_guidance_debug_partials(self._h, n_chains, None, C.byref(tp), C.byref(w), stream_ptr()))
        out = torch.empty((n_chains, self.cfg.batch, tp.value, w.value), dtype=torch.float32, device="cuda")
        check(lib().dgdm_guidance_debug_partials(self._h, n_chains, dptr(out), None, None, stream_ptr()))
        return out

    def rowcoef(self, centers: torch.Tensor) -> np.ndarray:
        """'convergence' row coefficients of one chain (deltas_to_objective :445-452 applied per cond_fn call)."""
        c = np.ascontiguousarray(centers.detach().cpu().numpy().astype(np.int64))
        out = np.empty(self.rows, dtype=np.float32)
        sub = self.cfg.sub_batch_size if self.dyn.kind == 3 else 0
        check(lib().dgdm_convergence_rowcoef(c.ctypes.data, len(c), self.cfg.grid_size, self.cfg.num_pos, self.rows, sub, out.ctypes.data))
        return out

    def goal_field(self, goals: torch.Tensor, specs: Sequence[_lib.GoalSpec]) -> torch.Tensor:
        """The row field of goal poses (include/dgdm_hip.h, dgdm_guidance_goal_field): goals (n, B, 3) = (ori, pos_x, pos_y) per chain
        and finger in the model's normalised inputs, specs one _lib.GoalSpec per chain -> (n, R, 3) float32 on the goals' device.
        A bad window, profile or a non-finite goal raises ValueError."""
        dev = torch.device("cuda", torch.cuda.current_device())
        gl = torch.as_tensor(goals).detach().to(device=dev, dtype=torch.float32).contiguous()
        n = len(specs)
        if gl.shape != (n, self.cfg.batch, 3):
            raise ValueError(f"goal_field: goals of shape {tuple(gl.shape)} for {n} specs (need ({n}, {self.cfg.batch}, 3))")
        arr = (_lib.GoalSpec * n)(*specs)
        out = torch.empty((n, self.rows, 3), dtype=torch.float32, device=dev)
        _check_value(lib().dgdm_guidance_goal_field(self._h, dptr(gl), arr, n, dptr(out), stream_ptr()))
        return out

    def set_row_field(self, field: Optional[torch.Tensor]) -> None:
        """field (n, R, 3) float32 on the device: the per-row seed of the chains whose objective is a row-field objective, chain i of a
        grad() / guided_chains_run launch reading field[i]; None clears it.  The library keeps the POINTER: the tensor is referenced
        here until it is replaced or cleared (and must not be modified while launches that read it are in flight)."""
        if field is None:
            check(lib().dgdm_guidance_set_row_field(self._h, None, 0, stream_ptr()))
            self._row_field = None
            return
        if not (field.is_cuda and field.dtype == torch.float32 and field.is_contiguous() and field.dim() == 3 and
                tuple(field.shape[1:]) == (self.rows, 3)):
            raise ValueError(f"set_row_field: a contiguous float32 device tensor (n, {self.rows}, 3) expected, got {tuple(field.shape)} {field.dtype}")
        check(lib().dgdm_guidance_set_row_field(self._h, dptr(field), field.shape[0], stream_ptr()))
        self._row_field = field

    def grad(self, x: torch.Tensor, timestep: int, objectives: Sequence[_lib.Objective], rowcoef: Optional[torch.Tensor] = None,
             starts: Optional[np.ndarray] = None) -> torch.Tensor:
        """x (n_chains, B, L) -> d sum(objective)/dx (n_chains, B, L)."""
        x = _f32(x)
        nc = x.shape[0]
        assert nc == len(objectives)
        arr = (_lib.Objective * nc)(*objectives)
        out = torch.empty_like(x)
        rc_ptr = dptr(rowcoef) if rowcoef is not None else None
        if self.dyn.kind == 2:
            check(lib().dgdm_dyn2d_guidance_grad(self._h, dptr(x), int(timestep), arr, rc_ptr, nc, dptr(out), stream_ptr()))
        else:
            assert starts is not None and starts.dtype == np.int64 and starts.size == nc * self.starts_per_call
            starts = np.ascontiguousarray(starts)
            check(lib().dgdm_dyn3d_guidance_grad(self._h, dptr(x), int(timestep), arr, rc_ptr, starts.ctypes.data, nc, dptr(out), stream_ptr()))
        return out

    def score(self, x: torch.Tensor, object_of_chain: Sequence[int], threshold_std: Sequence[float], timestep: int = 0,
              starts: Optional[np.ndarray] = None, want_logits: bool = False):
        """Forward-only scoring of x (n_chains, B, L) on the cond_fn grid (generator/diffusion.py:473-504, forward half; classes of
        :506-532): (counts (n, B, 3, 3, 3) int32 - the joint histogram of the classes of (d0, d1, d2) over the finger's G P^2 cells -,
        sums (n, B, 4) float32 = sum d0, sum |d0|, sum d1, sum d2[, logits (n, R, 3), row = cell * B + finger]).  threshold_std:
        threshold / std, the model's normalised units.  3-D: starts as grad() takes them.  'bf16' handles raise DgdmError."""
        x = _f32(x)
        nc, B = x.shape[0], self.cfg.batch
        oc = (C.c_int32 * nc)(*[int(o) for o in object_of_chain])
        thr = (C.c_float * 3)(*[float(v) for v in threshold_std])
        counts = torch.empty((nc, B, 3, 3, 3), dtype=torch.int32, device=x.device)
        sums = torch.empty((nc, B, 4), dtype=torch.float32, device=x.device)
        logits = torch.empty((nc, self.rows, 3), dtype=torch.float32, device=x.device) if want_logits else None
        sp = None
        if self.dyn.kind == 3:
            assert starts is not None and starts.dtype == np.int64 and starts.size == nc * self.starts_per_call
            starts = np.ascontiguousarray(starts)
            sp = starts.ctypes.data
        check(lib().dgdm_guidance_score(self._h, dptr(x), int(timestep), oc, sp, thr, nc, dptr(logits), dptr(counts), dptr(sums), stream_ptr()))
        return (counts, sums, logits) if want_logits else (counts, sums)

    def objective_values(self, logits: torch.Tensor, objectives: Sequence[_lib.Objective], rowcoef: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The objectives' VALUES per finger (include/dgdm_hip.h, dgdm_guidance_objective_values): logits (n_chains, R, 3) float32 as
        score(want_logits=True) returns them, objectives / rowcoef as grad() takes them (the row field is the handle's) ->
        (n_chains, B) float64, the objective of chain i summed over finger b's grid cells.  A row-field chain without a field raises
        DgdmError before anything is launched."""
        nc = len(objectives)
        if not (logits.is_cuda and logits.dtype == torch.float32 and tuple(logits.shape) == (nc, self.rows, 3)):
            raise ValueError(f"objective_values: float32 device logits ({nc}, {self.rows}, 3) expected, got {tuple(logits.shape)} {logits.dtype}")
        lg = logits.contiguous()
        arr = (_lib.Objective * nc)(*objectives)
        rc = _f32(rowcoef) if rowcoef is not None else None
        if rc is not None and rc.numel() != nc * self.rows:
            raise ValueError(f"objective_values: rowcoef of {rc.numel()} entries for {nc} chains of {self.rows} rows")
        out = torch.empty((nc, self.cfg.batch), dtype=torch.float64, device=lg.device)
        check(lib().dgdm_guidance_objective_values(self._h, dptr(lg), arr, dptr(rc), nc, dptr(out), stream_ptr()))
        return out

    def sweep(self, x: torch.Tensor, object_of_chain: Sequence[int], starts: Optional[np.ndarray] = None) -> torch.Tensor:
        """Orientation sweep of get_convergence_centers (:506-531): logits (n_chains, B*G, 3), row = g*B + b."""
        x = _f32(x)
        nc = x.shape[0]
        oc = (C.c_int32 * nc)(*object_of_chain)
        out = torch.empty((nc, self.sweep_rows, 3), dtype=torch.float32, device=x.device)
        sp = None
        if self.dyn.kind == 3:
            assert starts is not None and starts.dtype == np.int64 and starts.size == nc * 2 * self.sweep_rows
            starts = np.ascontiguousarray(starts)
            sp = starts.ctypes.data
        check(lib().dgdm_guidance_orientation_sweep(self._h, dptr(x), oc, sp, nc, dptr(out), stream_ptr()))
        return out

    def rollout(self, x: torch.Tensor, object_of_chain: Sequence[int], std: Sequence[float], n_interactions: int,
                starts: Optional[np.ndarray] = None, want_trajectory: bool = False):
        """The dynamics model iterated on its own output from the sweep's poses (include/dgdm_hip.h, dgdm_guidance_rollout; in place
        of the simulator's 40 gripper closings per start orientation, dynamics/sim_test_mj.py:161-185): x (n_chains, B, L) ->
        (final (n, B*G, 3) float64 = (ori, pos_x, pos_y) after the last interaction in the model's normalised inputs, first_logits
        (n, B*G, 3) float32 of interaction 0, left (n, B*G) int32 = the first interaction after which |pos| > 1 or -1[, traj_pose
        (K + 1, n, B*G, 3) float64 with slot 0 = the start, traj_logits (K, n, B*G, 3) float32]); row = g*B + b.  std: the dataset's
        (rad, m, m) the model's outputs are normalised by.  3-D: starts = K consecutive classifier calls' draws, (K, n_chains,
        2*B*G) int64 in the sweep's layout.  'bf16' and 'f32_mfma' handles raise DgdmError."""
        from .dynamics.dataloader import POS_NORM
        x = _f32(x)
        nc, K, R = x.shape[0], int(n_interactions), self.sweep_rows
        oc = (C.c_int32 * nc)(*[int(o) for o in object_of_chain])
        scale = (C.c_double * 3)(float(std[0]) / np.pi, float(std[1]) / POS_NORM, float(std[2]) / POS_NORM)
        dev = x.device
        final = torch.empty((nc, R, 3), dtype=torch.float64, device=dev)
        first = torch.empty((nc, R, 3), dtype=torch.float32, device=dev)
        left = torch.empty((nc, R), dtype=torch.int32, device=dev)
        tp = torch.empty((max(K, 0) + 1, nc, R, 3), dtype=torch.float64, device=dev) if want_trajectory else None
        tl = torch.empty((max(K, 0), nc, R, 3), dtype=torch.float32, device=dev) if want_trajectory else None
        sp = None
        if self.dyn.kind == 3:
            assert starts is not None and starts.dtype == np.int64 and starts.size == max(K, 0) * nc * 2 * R
            starts = np.ascontiguousarray(starts)
            sp = starts.ctypes.data
        check(lib().dgdm_guidance_rollout(self._h, dptr(x), oc, sp, scale, K, nc, dptr(final), dptr(first), dptr(left), dptr(tp), dptr(tl), stream_ptr()))
        return (final, first, left, tp, tl) if want_trajectory else (final, first, left)

    LABEL_LAYOUTS = {"mean": 0, "per_object": 1}

    def _label_args(self, fingers, objects, layout, out, cols, column_offset, object_stride):
        """Shared front of label() / label_settled(): the fingers (N, L), the object array, the layout code, the rows matrix (a new
        (N, cols or M * cols) one unless `out` is given) and the pointer of its first written float."""
        x = _f32(fingers)
        x = x.reshape(x.shape[0], -1)
        if layout not in self.LABEL_LAYOUTS:
            raise ValueError(f"label layout {layout!r} not supported ('mean' or 'per_object')")
        M = len(objects)
        oc = (C.c_int32 * max(M, 1))(*[int(o) for o in objects])
        if object_stride is None:
            object_stride = cols
        if out is None:
            out = torch.empty((x.shape[0], cols if layout == "mean" else M * cols), dtype=torch.float32, device=x.device)
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.is_contiguous() and out.shape[0] == x.shape[0]):
            raise ValueError(f"label rows: a contiguous float32 device matrix of {x.shape[0]} rows expected, got {tuple(out.shape)} {out.dtype}")
        need = cols if layout == "mean" else (M - 1) * int(object_stride) + cols
        if column_offset < 0 or column_offset + max(need, cols) > out.shape[1]:
            raise ValueError(f"label rows: {need} floats from column {column_offset} do not fit rows of {out.shape[1]}")
        return x, oc, M, self.LABEL_LAYOUTS[layout], out, out.data_ptr() + 4 * int(column_offset), int(out.shape[1]), int(object_stride)

    def label(self, fingers: torch.Tensor, objects: Sequence[int], threshold_std: Sequence[float], timestep: int = 0,
              starts: Optional[np.ndarray] = None, layout: str = "mean", out: Optional[torch.Tensor] = None, column_offset: int = 0,
              object_stride: Optional[int] = None) -> torch.Tensor:
        """The tally columns of every finger (include/dgdm_hip.h, dgdm_guidance_label): fingers (N, L) in sampler units, any N, labelled
        in batches of the handle's B against `objects` -> rows (N, 10) ('mean') or (N, M * 10) ('per_object').  out / column_offset /
        object_stride: write into a wider matrix instead (row stride = its width).  3-D: starts (n_batches, M, starts_per_call) int64."""
        x, oc, M, lay, out, ptr, stride, ostride = self._label_args(fingers, objects, layout, out, 10, column_offset, object_stride)
        thr = (C.c_float * 3)(*[float(v) for v in threshold_std])
        sp = None
        if self.dyn.kind == 3:
            nb = -(-x.shape[0] // self.cfg.batch)
            assert starts is not None and starts.dtype == np.int64 and starts.size == nb * M * self.starts_per_call
            starts = np.ascontiguousarray(starts)
            sp = starts.ctypes.data
        check(lib().dgdm_guidance_label(self._h, dptr(x), x.shape[0], oc, M, int(timestep), thr, sp, lay, ptr, stride, ostride, stream_ptr()))
        return out

    def label_settled(self, fingers: torch.Tensor, objects: Sequence[int], std: Sequence[float], n_interactions: int,
                      starts: Optional[np.ndarray] = None, layout: str = "mean", out: Optional[torch.Tensor] = None, column_offset: int = 0,
                      object_stride: Optional[int] = None) -> torch.Tensor:
        """The settled columns of every finger from roll-outs of n_interactions (dgdm_guidance_label_settled) -> rows (N, 5) or
        (N, M * 5); placement as label().  std as rollout() takes it.  3-D: starts (n_batches, K, M, 2*B*G) int64."""
        from .dynamics.dataloader import POS_NORM
        x, oc, M, lay, out, ptr, stride, ostride = self._label_args(fingers, objects, layout, out, 5, column_offset, object_stride)
        K = int(n_interactions)
        scale = (C.c_double * 3)(float(std[0]) / np.pi, float(std[1]) / POS_NORM, float(std[2]) / POS_NORM)
        sp = None
        if self.dyn.kind == 3:
            nb = -(-x.shape[0] // self.cfg.batch)
            assert starts is not None and starts.dtype == np.int64 and starts.size == nb * max(K, 0) * M * 2 * self.sweep_rows
            starts = np.ascontiguousarray(starts)
            sp = starts.ctypes.data
        check(lib().dgdm_guidance_label_settled(self._h, dptr(x), x.shape[0], oc, M, scale, K, sp, lay, ptr, stride, ostride, stream_ptr()))
        return out

    def debug_rollout_table(self, n_chains: int):
        """Test hook: (layer 1's pose term of the last rollout()'s last interaction as operand tiles (n_chains, B, tiles_per_finger,
        W1 * 32), the sweep's own table in the same layout (tiles_per_finger, W1 * 32))."""
        tpf, w = C.c_int32(), C.c_int32()
        check(lib().dgdm_guidance_debug_rollout_table(self._h, n_chains, None, None, C.byref(tpf), C.byref(w), stream_ptr()))
        a = torch.empty((n_chains, self.cfg.batch, tpf.value, w.value * 32), dtype=torch.float32, device="cuda")
        b = torch.empty((tpf.value, w.value * 32), dtype=torch.float32, device="cuda")
        check(lib().dgdm_guidance_debug_rollout_table(self._h, n_chains, dptr(a), dptr(b), None, None, stream_ptr()))
        return a, b


def _bounds_block(bounds, numel: int, device) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(lo, hi) of an edit as contiguous float32 device tensors and their period; ValueError unless both have the same size and it divides numel."""
    if not isinstance(bounds, (tuple, list)) or len(bounds) != 2 or bounds[0] is None or bounds[1] is None:
        raise ValueError("bounds are a (lo, hi) pair of tensors")
    lo, hi = _f32(bounds[0]).to(device), _f32(bounds[1]).to(device)
    if lo.numel() != hi.numel() or lo.numel() == 0 or numel % lo.numel():
        raise ValueError(f"bounds of {lo.numel()} and {hi.numel()} entries do not tile the {numel} entries of the step")
    return lo, hi, lo.numel()


def _u64(v: int) -> int:
    return int(v) & 0xFFFFFFFFFFFFFFFF


def chain_keys_tensor(keys: Sequence[int], device) -> torch.Tensor:
    """Noise keys (uint64 values; negative ints wrap) as the int64 device tensor whose bits the library reads as uint64."""
    return torch.from_numpy(np.array([_u64(k) for k in keys], dtype=np.uint64).view(np.int64)).to(device)


def step_noise(seed: int, keys: Sequence[int], step_index: int, per_chain: int) -> torch.Tensor:
    """The keyed normals the stochastic step draws (dgdm_ddim_step_noise; the recipe is in include/dgdm_hip.h): (len(keys), per_chain)
    float32, row c = element 0 .. per_chain - 1 of the chain keyed (seed, keys[c]) at step `step_index`."""
    kd = chain_keys_tensor(keys, "cuda")
    out = torch.empty((len(keys), int(per_chain)), dtype=torch.float32, device="cuda")
    check(lib().dgdm_ddim_step_noise(_u64(seed), dptr(kd), len(keys), int(step_index), int(per_chain), dptr(out), stream_ptr()))
    return out


def resample_uniform(seed: int, keys: Sequence[int], step_index: int) -> torch.Tensor:
    """The uniform the resampling step of (seed, keys[c], step_index) draws (dgdm_resample_uniform): (len(keys),) float64 in [0, 1)."""
    kd = chain_keys_tensor(keys, "cuda")
    out = torch.empty((len(keys),), dtype=torch.float64, device="cuda")
    check(lib().dgdm_resample_uniform(_u64(seed), dptr(kd), len(keys), int(step_index), dptr(out), stream_ptr()))
    return out


def chain_resample(x: torch.Tensor, values: torch.Tensor, n_grad: int, beta_per_cell: float, ess_frac: float, seed: int, chain_keys: Sequence[int],
                   step_index: int, logw: torch.Tensor, vprev: torch.Tensor):
    """One weight / effective-sample-size / systematic-resampling step (include/dgdm_hip.h, dgdm_chain_resample): x (n_chains, B, L)
    float32, values (n_grad * n_chains, B) float64 object-major, logw / vprev (n_chains, B) float64 device tensors UPDATED IN PLACE (a
    run's state, zero at its start) -> (x_out (n_chains, B, L), ancestors (n_chains, B) int32, ess (n_chains,) float64,
    did (n_chains,) int32).  Shapes and dtypes are checked here (ValueError); the library refuses B, L, n_grad < 1."""
    if x.dim() != 3 or not x.is_cuda:
        raise ValueError(f"chain_resample: x (n_chains, B, L) on the device expected, got {tuple(x.shape)}")
    x = _f32(x)
    nc, B, L = x.shape
    if len(chain_keys) != nc:
        raise ValueError(f"chain_resample: {len(chain_keys)} chain keys for {nc} chains")
    if not (values.is_cuda and values.dtype == torch.float64 and tuple(values.shape) == (int(n_grad) * nc, B)):
        raise ValueError(f"chain_resample: float64 device values ({int(n_grad) * nc}, {B}) expected, got {tuple(values.shape)} {values.dtype}")
    for name, t in (("logw", logw), ("vprev", vprev)):
        if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (nc, B) and t.is_contiguous()):
            raise ValueError(f"chain_resample: {name} is a contiguous float64 device tensor ({nc}, {B}), got {tuple(t.shape)} {t.dtype}")
    values = values.contiguous()
    kd = chain_keys_tensor(chain_keys, x.device)
    out = torch.empty_like(x)
    anc = torch.empty((nc, B), dtype=torch.int32, device=x.device)
    ess = torch.empty((nc,), dtype=torch.float64, device=x.device)
    did = torch.empty((nc,), dtype=torch.int32, device=x.device)
    check(lib().dgdm_chain_resample(dptr(x), dptr(values), nc, B, L, int(n_grad), float(beta_per_cell), float(ess_frac), _u64(seed), dptr(kd),
                                    int(step_index), dptr(logw), dptr(vprev), dptr(out), dptr(anc), dptr(ess), dptr(did), stream_ptr()))
    return out, anc, ess, did


def ddim_guided_step(x: torch.Tensor, eps: torch.Tensor, grad: Optional[torch.Tensor], n_grad: int, coef: Tuple[float, float, float, float],
                     scale: float, bounds=None, eta_coef: Optional[Tuple[float, float]] = None, seed: int = 0,
                     chain_keys: Optional[Sequence[int]] = None, step_index: int = 0, variance_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad: None or (n_grad, *x.shape) stacked gradients whose mean guides the step.  bounds = (lo, hi): the predicted clean sample is
    clipped to them per entry instead of to [-1, 1] (dgdm_ddim_guided_step_bounded): lo / hi hold one block that repeats over x (e.g.
    (B, L) for x (n_chains, B, L)).

    eta_coef = (sigma, dir) (DDIMScheduler.eta_coefficients): the stochastic step (dgdm_ddim_guided_step_noisy), dir in the place of
    coef[3].  Its noise is `variance_noise` (like x), or the keyed device normal: x holds len(chain_keys) whole chains, chain c keyed
    (seed, chain_keys[c]) at `step_index`.  sigma > 0 with neither: ValueError.  eta_coef None is the eta = 0 step of old."""
    x, eps = _f32(x), _f32(eps)
    out = torch.empty_like(x)
    g = _f32(grad) if grad is not None else None
    args = (dptr(x), dptr(eps), dptr(g), n_grad, dptr(out), x.numel(), *[float(c) for c in coef[:3]])
    if eta_coef is not None:
        sigma, dirc = float(eta_coef[0]), float(eta_coef[1])
        lo = hi = None
        period = 0
        if bounds is not None:
            lo, hi, period = _bounds_block(bounds, x.numel(), x.device)
        z = kd = None
        per_chain = 0
        if sigma != 0.0:
            if variance_noise is not None:
                z = _f32(variance_noise).to(x.device)
                if z.numel() != x.numel():
                    raise ValueError(f"variance_noise of {z.numel()} entries for a step of {x.numel()}")
            elif chain_keys is not None:
                if len(chain_keys) == 0 or x.numel() % len(chain_keys):
                    raise ValueError(f"{len(chain_keys)} chain keys do not divide the {x.numel()} entries of the step into whole chains")
                kd, per_chain = chain_keys_tensor(chain_keys, x.device), x.numel() // len(chain_keys)
            else:
                raise ValueError("a step with sigma > 0 needs variance_noise or chain_keys")
        check(lib().dgdm_ddim_guided_step_noisy(*args, dirc, float(scale), dptr(lo), dptr(hi), period, sigma, dptr(z), _u64(seed), dptr(kd),
                                                int(step_index), per_chain, stream_ptr()))
        return out
    args = args + (float(coef[3]), float(scale))
    if bounds is None:
        check(lib().dgdm_ddim_guided_step(*args, stream_ptr()))
    else:
        lo, hi, period = _bounds_block(bounds, x.numel(), x.device)
        check(lib().dgdm_ddim_guided_step_bounded(*args, dptr(lo), dptr(hi), period, stream_ptr()))
    return out


def ddim_guided_step_bounded(x, eps, grad, n_grad: int, coef, scale: float, bounds) -> torch.Tensor:
    """ddim_guided_step under the name tests and scripts call; here bounds are not optional (None is the ValueError of a malformed pair)."""
    return ddim_guided_step(x, eps, grad, n_grad, coef, scale, () if bounds is None else bounds)


def guided_chains_run(unet: "Unet1d", guid: "Guidance", noise: torch.Tensor, n_chains: int, n_grad: int, objectives: Sequence[_lib.Objective],
                      rowcoef: Optional[torch.Tensor], starts: Optional[np.ndarray], timesteps: Sequence[int],
                      coefs: Sequence[Tuple[float, float, float, float]], scales: Sequence[float], global_cond: Optional[torch.Tensor] = None,
                      cfg_weight: float = 1.0, bounds=None, eta_coef: Optional[Sequence[Tuple[float, float]]] = None, seed: int = 0,
                      chain_keys: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The whole guided denoise loop in one library call (dgdm_guided_chains_run_noisy): noise (B, L) -> (n_chains, B, L).
    eta_coef: None (eta = 0), or one (sigma, dir) per step - chain k's step si then draws the keyed normal of (seed, chain_keys[k]) at
    step_index si; chain_keys None: 0 .. n_chains - 1.
    global_cond: (B, gc) shared by all chains or (n_chains, B, gc); cfg_weight: classifier-free guidance weight (1: the plain conditional run).
    bounds: None, or an edit's (lo, hi), each (B, L), shared by all chains - every step then clips its predicted clean sample to them;
    `noise` is then the edit's start sample and timesteps / coefs the schedule's last steps (dgdm_amd/edit.py)."""
    cond, cond_stride = chain_cond_layout(global_cond, unet.global_cond_dim, n_chains, noise.shape[0])
    x0 = _f32(noise).reshape(noise.shape[0], -1)
    B, L = x0.shape
    if cond is not None:
        cond = _f32(cond).to(x0.device)
    S = len(timesteps)
    assert len(objectives) == n_chains * n_grad and len(scales) == n_chains and len(coefs) == S
    arr = (_lib.Objective * len(objectives))(*objectives)
    ts = (C.c_int32 * S)(*[int(t) for t in timesteps])
    cf = (C.c_float * (4 * S))(*[float(v) for c in coefs for v in c])
    sc = (C.c_float * n_chains)(*[float(v) for v in scales])
    sp = None
    if guid.dyn.kind == 3:
        assert starts is not None and starts.dtype == np.int64 and starts.size == S * n_chains * n_grad * guid.starts_per_call
        starts = np.ascontiguousarray(starts)
        sp = starts.ctypes.data
    lo = hi = None
    if bounds is not None:
        lo, hi, period = _bounds_block(bounds, B * L, x0.device)
        if period != B * L:
            raise ValueError(f"bounds of {period} entries: the chains take one (B, L) = ({B}, {L}) block")
    out = torch.empty((n_chains, B, L), dtype=torch.float32, device=x0.device)
    ec = ck = None
    if eta_coef is not None:
        assert len(eta_coef) == S and (chain_keys is None or len(chain_keys) == n_chains)
        ec = (C.c_float * (2 * S))(*[float(v) for c in eta_coef for v in c])
        if chain_keys is not None:
            ck = (C.c_uint64 * n_chains)(*[_u64(k) for k in chain_keys])
    check(lib().dgdm_guided_chains_run_noisy(unet._h, guid._h, dptr(x0), n_chains, n_grad, arr, dptr(rowcoef) if rowcoef is not None else None, sp,
                                             ts, cf, sc, S, dptr(out), dptr(cond), int(cond_stride), float(cfg_weight), dptr(lo), dptr(hi),
                                             ec, _u64(seed), ck, stream_ptr()))
    return out         # `starts` has been consumed: every step converts it into the handle's pinned staging buffer before it returns


def ddim_add_noise(x0: torch.Tensor, noise: torch.Tensor, sqrt_abar: float, sqrt_1m_abar: float) -> torch.Tensor:
    x0, noise = _f32(x0), _f32(noise)
    out = torch.empty_like(x0)
    check(lib().dgdm_ddim_add_noise(dptr(x0), dptr(noise), dptr(out), x0.numel(), float(sqrt_abar), float(sqrt_1m_abar), stream_ptr()))
    return out


def ddim_pred_x0(x: torch.Tensor, eps: torch.Tensor, coef: Sequence[float]) -> torch.Tensor:
    """The predicted clean sample of a DDIM step on its own (dgdm_ddim_pred_x0): clip((x - coef[1] eps) / coef[0], -1, 1) in the step's
    float32 operations, coef = DDIMScheduler.coefficients(t)[:2] = (sqrt(abar_t), sqrt(1 - abar_t)).  x, eps: float32 device tensors of one
    shape (ValueError otherwise)."""
    for name, t in (("x", x), ("eps", eps)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            raise ValueError(f"ddim_pred_x0: {name} is a float32 device tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if x.shape != eps.shape:
        raise ValueError(f"ddim_pred_x0: x {tuple(x.shape)} and eps {tuple(eps.shape)} differ in shape")
    if len(coef) < 2:
        raise ValueError("ddim_pred_x0: coef holds sqrt(abar_t) and sqrt(1 - abar_t)")
    x, eps = x.contiguous(), eps.contiguous()
    out = torch.empty_like(x)
    check(lib().dgdm_ddim_pred_x0(dptr(x), dptr(eps), dptr(out), x.numel(), float(coef[0]), float(coef[1]), stream_ptr()))
    return out


def finger_decode_2d(samples: torch.Tensor, num_points: int = 200, scale: float = 0.03, offset: float = -0.015) -> torch.Tensor:
    """(B, L, 1) or (B, L) control values -> (B, 2 fingers, num_points, 2) spline points in metres; the defaults map sampler
    units [-1, 1] as dynamics/sim_test_mj.py:257-262 does before assets/finger_sampler.py:39-51."""
    s = _f32(samples).reshape(samples.shape[0], -1)
    out = torch.empty((s.shape[0], 2, num_points, 2), dtype=torch.float32, device=s.device)
    check(lib().dgdm_finger_decode_2d(dptr(s), s.shape[0], s.shape[1], int(num_points), float(scale), float(offset), dptr(out), stream_ptr()))
    return out


def finger_decode_3d(samples: torch.Tensor, sample_size: int = 25, scale: float = 0.05, offset: float = -0.05) -> torch.Tensor:
    """(B, 42, 1) or (B, 42) control values -> (B, 2 fingers, sample_size^2, 3) surface points in metres; the defaults map
    sampler units [-1, 1] as dynamics/sim_test_mj_3d.py:236-237 does before assets/finger_3d.py:60-81."""
    s = _f32(samples).reshape(samples.shape[0], -1)
    out = torch.empty((s.shape[0], 2, sample_size * sample_size, 3), dtype=torch.float32, device=s.device)
    check(lib().dgdm_finger_decode_3d(dptr(s), s.shape[0], s.shape[1], int(sample_size), float(scale), float(offset), dptr(out), stream_ptr()))
    return out


def read_obj(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """Vertex positions (V, 3) float64 and triangles (T, 3) int32, 0-based, of an OBJ file in file order (the reader of
    include/dgdm_hip.h: polygons fan-triangulated, everything but `v` / `f` ignored).  Host code; releases the GIL while it parses."""
    h = C.c_void_p()
    check(lib().dgdm_mesh_read_obj(os.fsencode(path), C.byref(h)))
    try:
        verts = np.empty((lib().dgdm_mesh_num_vertices(h), 3), dtype=np.float64)
        tris = np.empty((lib().dgdm_mesh_num_triangles(h), 3), dtype=np.int32)
        check(lib().dgdm_mesh_copy(h, verts.ctypes.data, tris.ctypes.data))
    finally:
        lib().dgdm_mesh_destroy(h)
    return verts, tris


def concat_meshes(meshes: Sequence[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray, Tuple[np.ndarray, np.ndarray]]:
    """[(verts (V_m, 3), tris (T_m, 3) local to the mesh), ...] -> the batch form of sample_mesh_points."""
    nv = np.array([0] + [len(v) for v, _ in meshes], dtype=np.int64)
    nt = np.array([0] + [len(t) for _, t in meshes], dtype=np.int64)
    verts = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 3) for v, _ in meshes])
    tris = np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1, 3) for _, t in meshes])
    return verts, tris, (np.cumsum(nv), np.cumsum(nt))


def sample_mesh_points(verts, tris, offsets, keys, num_points: int, seed: int = 0) -> torch.Tensor:
    """Surface point clouds of a batch of meshes, (M, num_points, 3) float64 on the current device: open3d's sample_points_uniformly
    (dynamics/utils.py:14-18) under the sampling contract of include/dgdm_hip.h (DESIGN.md "Object clouds from meshes").
    verts (V, 3) float64 and tris (T, 3) int32 (indices local to their mesh) are the meshes concatenated, host or device;
    offsets = (vertex offsets, triangle offsets), each M + 1 int64 starting at 0 (concat_meshes builds all three);
    keys: M uint64 mesh keys (callers use zlib.crc32 of the object name).  Synchronises the stream once."""
    vo = np.ascontiguousarray(offsets[0], dtype=np.int64)
    to = np.ascontiguousarray(offsets[1], dtype=np.int64)
    k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    M = len(to) - 1
    if M < 1 or len(vo) != M + 1 or len(k) != M:
        raise ValueError(f"sample_mesh_points: {len(vo)} vertex offsets, {len(to)} triangle offsets and {len(k)} keys (need M + 1, M + 1, M)")
    dev = torch.device("cuda", torch.cuda.current_device())
    v = torch.as_tensor(verts).to(device=dev, dtype=torch.float64).contiguous()
    t = torch.as_tensor(tris).to(device=dev, dtype=torch.int32).contiguous()
    if v.numel() != 3 * int(vo[-1]) or t.numel() != 3 * int(to[-1]):
        raise ValueError(f"sample_mesh_points: {v.numel() // 3} vertices / {t.numel() // 3} triangles, the offsets say {int(vo[-1])} / {int(to[-1])}")
    ws_bytes = lib().dgdm_mesh_sample_workspace_bytes(to.ctypes.data, M)
    if ws_bytes < 0:
        check(int(ws_bytes))
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    out = torch.empty((M, int(num_points), 3), dtype=torch.float64, device=dev)
    check(lib().dgdm_mesh_sample_points(dptr(v), dptr(t), vo.ctypes.data, to.ctypes.data, M, int(seed) & 0xFFFFFFFFFFFFFFFF, k.ctypes.data,
                                        int(num_points), dptr(out), dptr(ws), int(ws_bytes), stream_ptr()))
    return out


def _check_value(rc: int) -> None:
    """check(), with DGDM_EINVAL (a bad image or argument) raised as ValueError, as numpy / cv2 callers expect."""
    if rc == _lib.EINVAL:
        raise ValueError(lib().dgdm_last_error().decode("utf-8", "replace"))
    check(rc)


# ---------------------------------------------------------------------------------------------------------------- finger meshes
MESH_2D, MESH_3D, PIECE_2D, PIECE_3D = 2, 3, 12, 13       # the kinds of include/dgdm_hip.h "finger meshes"
_faces_dev: Dict[Tuple[int, int, str], torch.Tensor] = {}


def finger_mesh_faces(kind: int, n: int = 0) -> np.ndarray:
    """The triangle table (T, 3) int32, 0-based and outward-oriented, of one finger mesh: kind 2 the extruded 2-D finger of n curve
    points, kind 3 the 3-D finger of n x n surface samples, kinds 12 / 13 one collision piece of either (n unused).  Host code."""
    nv, nt = C.c_int64(), C.c_int64()
    _check_value(lib().dgdm_finger_mesh_counts(int(kind), int(n), C.byref(nv), C.byref(nt)))
    tris = np.empty((nt.value, 3), dtype=np.int32)
    _check_value(lib().dgdm_finger_mesh_faces(int(kind), int(n), tris.ctypes.data))
    return tris


def _faces_on(kind: int, n: int, device: torch.device) -> torch.Tensor:
    key = (int(kind), int(n), str(device))
    if key not in _faces_dev:
        _faces_dev[key] = torch.from_numpy(finger_mesh_faces(kind, n)).to(device)
    return _faces_dev[key]


def finger_mesh_2d(samples: torch.Tensor, num_points: int = 200, width: float = 0.03, height: float = 0.02, scale: float = 0.03,
                   offset: float = -0.015) -> torch.Tensor:
    """(B, L, 1) or (B, L) control values -> (B, 2 fingers, 4 num_points, 3) mesh vertices in metres: the four rings of
    generate_finger_shape (assets/finger_sampler.py:13-21) over finger_decode_2d's curve; faces are finger_mesh_faces(2, num_points).
    The defaults are what prepare_finger passes (dynamics/sim_test_mj.py:90-97)."""
    s = _f32(samples).reshape(samples.shape[0], -1)
    out = torch.empty((s.shape[0], 2, 4 * int(num_points), 3), dtype=torch.float32, device=s.device)
    _check_value(lib().dgdm_finger_mesh_vertices_2d(dptr(s), s.shape[0], s.shape[1], int(num_points), float(scale), float(offset), float(width),
                                                    float(height), dptr(out), stream_ptr()))
    return out


def finger_mesh_3d(samples: torch.Tensor, sample_size: int = 25, width: float = 0.1, scale: float = 0.05, offset: float = -0.05) -> torch.Tensor:
    """(B, 42, 1) or (B, 42) control values -> (B, 2 fingers, 2 sample_size^2, 3) mesh vertices in metres: finger_decode_3d's sheet and
    the sheet + width in y (assets/finger_3d.py:41-44); faces are finger_mesh_faces(3, sample_size).  The defaults are what
    prepare_gripper passes (dynamics/sim_test_mj_3d.py:80-85)."""
    s = _f32(samples).reshape(samples.shape[0], -1)
    out = torch.empty((s.shape[0], 2, 2 * int(sample_size) ** 2, 3), dtype=torch.float32, device=s.device)
    _check_value(lib().dgdm_finger_mesh_vertices_3d(dptr(s), s.shape[0], s.shape[1], int(sample_size), float(scale), float(offset), float(width),
                                                    dptr(out), stream_ptr()))
    return out


def finger_mesh_stats(verts: torch.Tensor, tris, area_eps: float = 0.0) -> torch.Tensor:
    """verts (..., V, 3) float32 on the device, tris (T, 3) int32 shared by every mesh -> (..., 4) float64: signed volume, surface area,
    smallest triangle area, number of triangles with area < area_eps."""
    v = _f32(verts)
    t = torch.as_tensor(tris).to(device=v.device, dtype=torch.int32).contiguous()
    lead = v.shape[:-2]
    out = torch.empty((*lead, 4), dtype=torch.float64, device=v.device)
    _check_value(lib().dgdm_finger_mesh_stats(dptr(v), dptr(t), int(np.prod(lead, dtype=np.int64)), v.shape[-2], t.shape[0], float(area_eps),
                                              dptr(out), stream_ptr()))
    return out


def finger_pieces_2d(verts: torch.Tensor, pieces: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """finger_mesh_2d's vertices (B, 2, 4 n, 3) -> (collision pieces (B, 2, pieces, 8, 3) float32, chord_err (B, 2) float64 metres).
    Piece k is the sheared box between knots k and k + 1 of the curve, faces finger_mesh_faces(12); the default is the reference's
    V-HACD hull cap (dynamics/sim_test_mj.py:69-70)."""
    v = _f32(verts)
    B, n = v.shape[0], v.shape[2] // 4
    out = torch.empty((B, 2, int(pieces), 8, 3), dtype=torch.float32, device=v.device)
    err = torch.empty((B, 2), dtype=torch.float64, device=v.device)
    _check_value(lib().dgdm_finger_pieces_2d(dptr(v), B, n, int(pieces), dptr(out), dptr(err), stream_ptr()))
    return out, err


def finger_pieces_3d(verts: torch.Tensor, pu: int = 8, pv: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
    """finger_mesh_3d's vertices (B, 2, 2 n^2, 3) -> (collision pieces (B, 2, 2 pu pv, 6, 3) float32, chord_err (B, 2) float64 metres).
    Each cell of the (pu + 1) x (pv + 1) knot grid gives two triangular prisms, faces finger_mesh_faces(13); the default 2 * 8 * 2 = 32
    is the reference's V-HACD hull cap (dynamics/sim_test_mj_3d.py:59-60)."""
    v = _f32(verts)
    B = v.shape[0]
    n = int(round((v.shape[2] // 2) ** 0.5))
    if 2 * n * n != v.shape[2]:
        raise ValueError(f"finger_pieces_3d: {v.shape[2]} vertices per finger is not 2 n^2")
    out = torch.empty((B, 2, 2 * int(pu) * int(pv), 6, 3), dtype=torch.float32, device=v.device)
    err = torch.empty((B, 2), dtype=torch.float64, device=v.device)
    _check_value(lib().dgdm_finger_pieces_3d(dptr(v), B, n, int(pu), int(pv), dptr(out), dptr(err), stream_ptr()))
    return out, err


def write_obj(path: str, verts, tris) -> None:
    """Vertices (V, 3), written as float32 with 9 significant digits, and triangles (T, 3), 0-based, as an OBJ file that read_obj returns
    unchanged.  Host code; releases the GIL while it formats and writes."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    _check_value(lib().dgdm_mesh_write_obj(os.fsencode(path), v.ctypes.data, len(v), t.ctypes.data, len(t)))


def resample_contours(points, offsets, num_points: int, rescale: bool = False) -> torch.Tensor:
    """resample_contour (assets/icon_process.py) of a batch of contours, (M, num_points, 2) on the current device: int32, or float64
    c / 128 * 0.1 - 0.05 when rescale.  points (total, 2) integer pixel pairs, host or device; offsets M + 1 int64 starting at 0,
    contour m = rows offsets[m] .. offsets[m + 1] (at least one point each).  Contract: include/dgdm_hip.h, DESIGN.md §4.5b."""
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    M, n = len(off) - 1, int(num_points)
    if M < 1:
        raise ValueError("resample_contours: need at least one contour (offsets of length M + 1)")
    if n < 1:
        raise ValueError(f"resample_contours: num_points {n} (need >= 1)")
    dev = torch.device("cuda", torch.cuda.current_device())
    p = torch.as_tensor(points)
    if p.dtype.is_floating_point or p.dtype.is_complex or p.dtype == torch.bool:
        raise ValueError(f"resample_contours: integer points expected, got {p.dtype}")
    p = p.to(device=dev, dtype=torch.int32).contiguous()
    if p.numel() != 2 * int(off[-1]):
        raise ValueError(f"resample_contours: {p.numel() // 2} points, the offsets say {int(off[-1])}")
    ws_bytes = lib().dgdm_contour_resample_workspace_bytes(off.ctypes.data, M)
    if ws_bytes < 0:
        _check_value(int(ws_bytes))
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    out = torch.empty((M, n, 2), dtype=torch.float64 if rescale else torch.int32, device=dev)
    _check_value(lib().dgdm_contour_resample(dptr(p), off.ctypes.data, M, n, int(bool(rescale)), dptr(out), dptr(ws), int(ws_bytes),
                                             stream_ptr()))
    return out


def icon_raw_contours(images) -> Tuple[torch.Tensor, np.ndarray]:
    """The contour extract_contours keeps for each icon, before resampling: (points (total, 2) int32 on the current device, offsets
    M + 1 int64 on the host), image m's contour = rows offsets[m] .. offsets[m + 1], in cv2's point order.  images (M, H, W, C) uint8,
    host or device, C = 3 (BGR) or 4 (BGRA, alpha ignored).  An image without foreground raises ValueError naming its index.
    Synchronises the stream twice (the counts, the points).  Contract: include/dgdm_hip.h, DESIGN.md §4.5b."""
    im = torch.as_tensor(images)
    if im.dtype != torch.uint8:
        raise ValueError(f"icon_contours: uint8 images expected, got {im.dtype}")
    if im.dim() != 4 or im.shape[3] not in (3, 4) or min(im.shape) < 1:
        raise ValueError(f"icon_contours: images of shape (M, H, W, 3|4) expected, got {tuple(im.shape)}")
    M, H, W, Cn = (int(d) for d in im.shape)
    dev = torch.device("cuda", torch.cuda.current_device())
    im = im.to(device=dev).contiguous()
    ws_bytes = lib().dgdm_icon_workspace_bytes(M)
    if ws_bytes < 0:
        _check_value(int(ws_bytes))
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    counts = np.zeros(M, dtype=np.int64)
    _check_value(lib().dgdm_icon_trace(dptr(im), M, H, W, Cn, dptr(ws), int(ws_bytes), counts.ctypes.data, stream_ptr()))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rs_bytes = lib().dgdm_contour_resample_workspace_bytes(off.ctypes.data, M)
    if rs_bytes < 0:
        _check_value(int(rs_bytes))
    rs = torch.empty(int(rs_bytes), dtype=torch.uint8, device=dev)
    points = torch.empty((int(off[-1]), 2), dtype=torch.int32, device=dev)
    _check_value(lib().dgdm_icon_fetch_contours(dptr(ws), int(ws_bytes), M, off.ctypes.data, dptr(points), dptr(rs), int(rs_bytes), stream_ptr()))
    return points, off


def icon_contours(images, num_points: int = 100, rescale: bool = False) -> torch.Tensor:
    """extract_contours (assets/icon_process.py) of a stack of icons in one batch: (M, num_points, 2) on the current device, int32
    pixel coordinates on the 128 x 128 grid, or float64 c / 128 * 0.1 - 0.05 when rescale.  images as icon_raw_contours takes them.
    Synchronises the stream three times (the counts, the points, the resample)."""
    if int(num_points) < 1:
        raise ValueError(f"icon_contours: num_points {int(num_points)} (need >= 1)")
    points, off = icon_raw_contours(images)
    return resample_contours(points, off, num_points, rescale)


# ---------------------------------------------------------------------------------------------------------------- mesh rendering
RENDER_MAX_SIZE = 2048


def render_meshes(verts, tris, offsets, inst_view, inst_mesh, inst_matrix, inst_id, n_views: int, width: int, height: int, inst_rgb=None,
                  eyes=None, inst_model=None, snapped: bool = False):
    """One batched z-buffer rendering (include/dgdm_hip.h "mesh rendering") -> (ids (n_views, height, width) int32, -1 =
    background; depth float32, +inf there; rgb (n_views, height, width, 3) uint8, white there, or None without inst_rgb / eyes; rejected
    (n_views,) int32: triangles dropped for a vertex behind the eye or off the snapping range), all on the current device.
    verts (V, 3), tris (T, 3) int32 local to their mesh and offsets = (vertex offsets, triangle offsets) are the meshes concatenated
    (concat_meshes), host or device.  Per instance: inst_view, inst_mesh, inst_matrix (n_inst, 4, 4) model -> pixel x, pixel y, depth, w
    (float64 is rounded to float32 once, here), inst_id, inst_rgb (n_inst, 3) in [0, 1].  eyes (n_views, 3): the eye of each view in world
    coordinates; inst_model (n_inst, 4, 4): the instances' model -> world matrices (identity when None), used only to carry each view's eye
    into the instance's model frame on the host, in float64.  snapped=True appends the debug table (instance vertices, 4) int32 of
    X, Y, the bits of zs, kept.  Synchronises the stream once."""
    vo = np.ascontiguousarray(offsets[0], dtype=np.int64).reshape(-1)
    to = np.ascontiguousarray(offsets[1], dtype=np.int64).reshape(-1)
    M = len(vo) - 1
    view = np.ascontiguousarray(inst_view, dtype=np.int32).reshape(-1)
    mesh = np.ascontiguousarray(inst_mesh, dtype=np.int32).reshape(-1)
    ident = np.ascontiguousarray(inst_id, dtype=np.int32).reshape(-1)
    n = len(view)
    mat64 = np.asarray(inst_matrix, dtype=np.float64)
    if M < 1 or len(to) != M + 1 or n < 1 or len(mesh) != n or len(ident) != n or mat64.shape != (n, 4, 4):
        raise ValueError(f"render_meshes: {len(vo)} / {len(to)} offsets (need M + 1 each), {n} views, {len(mesh)} meshes, {len(ident)} ids and "
                         f"matrices of shape {mat64.shape} (need (n_inst, 4, 4))")
    mat = np.ascontiguousarray(mat64, dtype=np.float32)
    want_rgb = inst_rgb is not None and eyes is not None
    if (inst_rgb is None) != (eyes is None):
        raise ValueError("render_meshes: inst_rgb and eyes come together (both for an rgb image, neither without)")
    n_views, width, height = int(n_views), int(width), int(height)
    rgbs = eye_m = None
    if want_rgb:
        rgbs = np.ascontiguousarray(inst_rgb, dtype=np.float32).reshape(-1, 3)
        ew = np.asarray(eyes, dtype=np.float64).reshape(-1, 3)
        if len(rgbs) != n or len(ew) != n_views:
            raise ValueError(f"render_meshes: {len(rgbs)} colours for {n} instances, {len(ew)} eyes for {n_views} views")
        if view.min() < 0 or view.max() >= n_views:
            raise ValueError(f"render_meshes: view indices {int(view.min())} .. {int(view.max())} outside 0 .. {n_views - 1}")
        e = np.concatenate([ew[view], np.ones((n, 1))], axis=1)
        if inst_model is not None:
            mod = np.asarray(inst_model, dtype=np.float64)
            if mod.shape != (n, 4, 4):
                raise ValueError(f"render_meshes: inst_model of shape {mod.shape} (need ({n}, 4, 4))")
            e = np.einsum('nij,nj->ni', np.linalg.inv(mod), e)
        eye_m = np.ascontiguousarray(e[:, :3] / e[:, 3:4], dtype=np.float32)
    dev = torch.device("cuda", torch.cuda.current_device())
    v = torch.as_tensor(verts).to(device=dev, dtype=torch.float32).contiguous()
    t = torch.as_tensor(tris).to(device=dev, dtype=torch.int32).contiguous()
    if v.numel() != 3 * int(vo[-1]) or t.numel() != 3 * int(to[-1]):
        raise ValueError(f"render_meshes: {v.numel() // 3} vertices / {t.numel() // 3} triangles, the offsets say {int(vo[-1])} / {int(to[-1])}")
    ws_bytes = lib().dgdm_render_workspace_bytes(vo.ctypes.data, to.ctypes.data, M, mesh.ctypes.data, n, n_views)
    if ws_bytes < 0:
        _check_value(int(ws_bytes))
    if not (1 <= width <= RENDER_MAX_SIZE and 1 <= height <= RENDER_MAX_SIZE):
        raise ValueError(f"render_meshes: image of {width} x {height} (need 1 .. {RENDER_MAX_SIZE} each)")
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    ids = torch.empty((n_views, height, width), dtype=torch.int32, device=dev)
    depth = torch.empty((n_views, height, width), dtype=torch.float32, device=dev)
    rgb = torch.empty((n_views, height, width, 3), dtype=torch.uint8, device=dev) if want_rgb else None
    rejected = torch.empty((n_views,), dtype=torch.int32, device=dev)
    n_pv = int(sum(vo[m + 1] - vo[m] for m in mesh))
    snap = torch.empty((n_pv, 4), dtype=torch.int32, device=dev) if snapped else None
    _check_value(lib().dgdm_render_meshes(dptr(v), dptr(t), vo.ctypes.data, to.ctypes.data, M, view.ctypes.data, mesh.ctypes.data, mat.ctypes.data,
                                          ident.ctypes.data, rgbs.ctypes.data if want_rgb else None, eye_m.ctypes.data if want_rgb else None, n,
                                          n_views, width, height, dptr(ids), dptr(depth), dptr(rgb), dptr(rejected), dptr(snap), dptr(ws),
                                          int(ws_bytes), stream_ptr()))
    return (ids, depth, rgb, rejected, snap) if snapped else (ids, depth, rgb, rejected)


# ---------------------------------------------------------------------------------------------------------------- integer rings
POLYGON_MAX_POINTS, POLYGON_MAX_COORD = 256, 32767


def _ring_points(points, fn: str) -> torch.Tensor:
    p = torch.as_tensor(points)
    if p.dtype.is_floating_point or p.dtype.is_complex or p.dtype == torch.bool:
        raise ValueError(f"{fn}: integer points expected (extract_contours_batch(..., rescale=False)), got {p.dtype}")
    if p.dim() != 3 or p.shape[2] != 2 or p.shape[0] < 1:
        raise ValueError(f"{fn}: points of shape (batch, n, 2) expected, got {tuple(p.shape)}")
    if p.dtype != torch.int32 and p.numel() and (int(p.min()) < 0 or int(p.max()) > POLYGON_MAX_COORD):
        raise ValueError(f"{fn}: a coordinate outside [0, {POLYGON_MAX_COORD}]")            # before the cast to int32 can wrap it
    return p.to(device=torch.device("cuda", torch.cuda.current_device()), dtype=torch.int32).contiguous()


def polygon_decompose(points, pieces: bool = True) -> Dict[str, torch.Tensor]:
    """Steps 1-4 of the ring contract of include/dgdm_hip.h ("integer rings") for a batch of closed rings in one launch.
    points (batch, n, 2) integer pixel coordinates in [0, 32767], 3 <= n <= 256, host or device.  Device tensors: status (batch,) int32,
    count (batch,) int32, ring (batch, n) int32, area2 (batch,) int64, triangles (batch, n - 2, 3) int32 and, with pieces, piece_count
    (batch,), piece_offsets (batch, n - 1), piece_index (batch, 3 (n - 2)) int32; unused entries are -1.  Synchronises the stream once."""
    p = _ring_points(points, "polygon_decompose")
    B, n = int(p.shape[0]), int(p.shape[1])
    new = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=p.device)      # noqa: E731
    out = {"status": new(B), "count": new(B), "ring": new(B, n), "area2": new(B, dtype=torch.int64), "triangles": new(B, max(n - 2, 0), 3)}
    head = [dptr(p), B, n] + [dptr(out[k]) for k in ("status", "count", "ring", "area2", "triangles")]
    if pieces:
        out.update(piece_count=new(B), piece_offsets=new(B, max(n - 1, 0)), piece_index=new(B, 3 * max(n - 2, 0)))
        _check_value(lib().dgdm_polygon_convex_pieces(*head, dptr(out["piece_count"]), dptr(out["piece_offsets"]), dptr(out["piece_index"]),
                                                      stream_ptr()))
    else:
        _check_value(lib().dgdm_polygon_triangulate(*head, stream_ptr()))
    return out


def polygon_triangulate(points) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(status, count, ring, area2, triangles) of polygon_decompose: the cleaned ring, why it is refused if it is, and its M - 2
    triangles of original indices in clip order."""
    o = polygon_decompose(points, pieces=False)
    return o["status"], o["count"], o["ring"], o["area2"], o["triangles"]


def canonical_pieces(piece_count, piece_offsets, piece_index) -> List[List[Tuple[int, ...]]]:
    """The pieces of polygon_decompose as host tuples in canonical form: each rotated to start at its smallest index, then sorted."""
    pc, po, pi = (torch.as_tensor(t).cpu().numpy() for t in (piece_count, piece_offsets, piece_index))
    out = []
    for b in range(len(pc)):
        faces = []
        for q in range(int(pc[b])):
            f = pi[b, po[b, q]:po[b, q + 1]].tolist()
            k = f.index(min(f))
            faces.append(tuple(f[k:] + f[:k]))
        out.append(sorted(faces))
    return out


def polygon_pieces(points) -> List[List[Tuple[int, ...]]]:
    """The convex pieces (Hertel-Mehlhorn on polygon_triangulate's triangles) of each ring, canonical: a list per ring (empty for a
    refused ring) of tuples of original indices, counter-clockwise in the working order."""
    o = polygon_decompose(points)
    return canonical_pieces(o["piece_count"], o["piece_offsets"], o["piece_index"])


# ---------------------------------------------------------------------------------------------------------------- squeeze simulator
SQUEEZE_DEFAULTS = dict(theta_cells=720, x_cells=241, x_half=0.06, window=2, closing_steps=6, travel_max=0.1, finger_half_len=0.12)
SQUEEZE_WORKSPACE_BYTES = 1 << 30       # default chunking of squeeze_tables: as many pairs as fit 1 GiB (7.6 MB per pair at the defaults)


def squeeze_rotation_table(theta_cells: int) -> np.ndarray:
    """rot (theta_cells, 2) float64 = (cos, sin) of 2 pi a / theta_cells: the table dgdm_squeeze_map takes (host, numpy)."""
    ang = 2.0 * np.pi * np.arange(int(theta_cells), dtype=np.float64) / float(theta_cells)
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1))


def squeeze_config(**kw) -> _lib.SqueezeConfig:
    c = dict(SQUEEZE_DEFAULTS)
    unknown = set(kw) - set(c)
    if unknown:
        raise ValueError(f"squeeze_config: unknown keys {sorted(unknown)}")
    c.update(kw)
    return _lib.SqueezeConfig(int(c["theta_cells"]), int(c["x_cells"]), int(c["window"]), int(c["closing_steps"]), float(c["x_half"]),
                              float(c["travel_max"]), float(c["finger_half_len"]))


def _squeeze_mover():
    """t -> a contiguous float64 tensor on the current device (no copy of one that is there already)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    return lambda t: torch.as_tensor(t).detach().to(device=dev, dtype=torch.float64).contiguous()


def _squeeze_front(who: str, cfg, f64, sizer, pairs, starts, rot, tables: bool, workspace_bytes: Optional[int]):
    """What squeeze_tables and squeeze_tables_3d (`who`) do alike.  f64: _squeeze_mover(); sizer(n): the entry's *_workspace_bytes for
    chunks of n pairs.  -> (out, tail, keep): the output dict; the entries' common trailing arguments, from pairs_host to stream; the
    arrays behind them.  Without workspace_bytes the workspace holds as many pairs as fit SQUEEZE_WORKSPACE_BYTES, at least one, never
    more than the call has."""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P, T, X = len(pr), cfg.theta_cells, cfg.x_cells
    fit = int(sizer(min(max(P, 1), 65535)))         # all pairs in one chunk; negative: a config or sizes the library refuses
    if fit < 0:
        _check_value(fit)
    rt = f64(squeeze_rotation_table(T) if rot is None else rot)
    if rt.shape != (T, 2):
        raise ValueError(f"{who}: rot of shape {tuple(rt.shape)} (need ({T}, 2))")
    st = f64(starts).reshape(-1, 3) if starts is not None else None
    N = 0 if st is None else int(st.shape[0])
    if workspace_bytes is not None:
        ws_bytes = int(workspace_bytes)
    elif fit <= SQUEEZE_WORKSPACE_BYTES:
        ws_bytes = fit
    else:                                           # the library cuts the budget into chunks of as many pairs as fit it
        ws_bytes = max(SQUEEZE_WORKSPACE_BYTES, int(sizer(1)))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=rt.device)
    new = lambda *shape, dtype: torch.empty(shape, dtype=dtype, device=rt.device)                      # noqa: E731
    out = {"cells": new(P, N, 3, dtype=torch.int32), "y": new(P, N, 2, dtype=torch.float64), "flags": new(P, N, dtype=torch.int32)}
    if tables:
        out.update({k: new(P, T, X, dtype=torch.float64) for k in ("S", "touch_l", "touch_r")})
        out["succ"] = new(P, T * X, dtype=torch.int32)
    tail = (pr.ctypes.data, P, dptr(rt), dptr(st), N, dptr(out["cells"]), dptr(out["y"]), dptr(out["flags"]), dptr(out.get("S")),
            dptr(out.get("touch_l")), dptr(out.get("touch_r")), dptr(out.get("succ")), dptr(ws), ws_bytes, stream_ptr())
    return out, tail, (pr, rt, st, ws)


def squeeze_tables(surfaces, objects, pairs, starts=None, rot=None, tables: bool = False, workspace_bytes: Optional[int] = None,
                   friction: float = 0.0, jam: bool = False, contact: bool = False, **config) -> Dict[str, torch.Tensor]:
    """dgdm_squeeze_map (include/dgdm_hip.h "squeeze simulator") on the current device.  surfaces (F, 2, m) float64: the
    lower and upper jaw surface at travel 0; objects (O, nv, 2) float64 polygons; pairs (P, 2) (finger, object), host; starts (N, 3)
    float64 (theta0, x0, y0) shared by all pairs, or None; rot: squeeze_rotation_table(theta_cells) when None; config: the keys of
    SQUEEZE_DEFAULTS.  -> cells (P, N, 3) int32 (start, closed, settled cell = a * x_cells + b), y (P, N, 2) float64, flags (P, N) int32
    and, with tables, S / touch_l / touch_r (P, theta_cells, x_cells) float64 and succ (P, theta_cells * x_cells) int32.  The pairs run in
    chunks of as many as workspace_bytes holds.  Synchronises the stream once.
    friction: the Coulomb coefficient mu of dgdm_squeeze_map_friction ("squeeze simulator with Coulomb friction"); that entry runs when
    friction > 0 or when its tables are asked for - jam (P, theta_cells, x_cells) int32 and contact (P, theta_cells, x_cells, 2) int32
    (the lower and upper contact's code), both also returned with tables=True - and flags then carries 8 / 16 (start / settled cell
    jammed).  Otherwise dgdm_squeeze_map runs, as it always did."""
    from .sim.squeeze import check_friction
    cfg = squeeze_config(**config)
    mu = check_friction(friction, "squeeze_tables")
    with_friction = mu > 0.0 or bool(jam) or bool(contact)
    f64 = _squeeze_mover()
    sf, ob = f64(surfaces), f64(objects)
    if sf.dim() != 3 or sf.shape[1] != 2 or ob.dim() != 3 or ob.shape[2] != 2:
        raise ValueError(f"squeeze_tables: surfaces (F, 2, m) and objects (O, nv, 2) expected, got {tuple(sf.shape)} and {tuple(ob.shape)}")
    sizer = lib().dgdm_squeeze_friction_workspace_bytes if with_friction else lib().dgdm_squeeze_workspace_bytes
    out, tail, keep = _squeeze_front("squeeze_tables", cfg, f64, lambda n: sizer(C.byref(cfg), n), pairs, starts, rot, tables, workspace_bytes)
    shape = (len(keep[0]), cfg.theta_cells, cfg.x_cells)
    if with_friction and (tables or jam):
        out["jam"] = torch.empty(shape, dtype=torch.int32, device=sf.device)
    if with_friction and (tables or contact):
        out["contact"] = torch.empty(shape + (2,), dtype=torch.int32, device=sf.device)
    args = (C.byref(cfg), dptr(sf), int(sf.shape[0]), int(sf.shape[2]), dptr(ob), int(ob.shape[0]), int(ob.shape[1])) + tail
    if with_friction:
        _check_value(lib().dgdm_squeeze_map_friction(*args, mu, dptr(out.get("jam")), dptr(out.get("contact"))))
    else:
        _check_value(lib().dgdm_squeeze_map(*args))
    return out


LABEL_LAYOUTS = {"mean": 0, "per_object": 1}        # DGDM_LABEL_MEAN / DGDM_LABEL_PER_OBJECT


def _squeeze_label_front(who: str, cfg, f64, sf, objects, starts, n_tally, threshold, score_std, pos_norm, layout, rot, out, column_offset,
                         object_stride, counts, workspace_bytes, sizer):
    """What squeeze_label and squeeze_label_3d (`who`) do alike once their own inputs are on the device (sf: the surfaces, fingers
    leading).  sizer(n, M): the entry's *_workspace_bytes for chunks of n fingers of M objects.  -> (out, counts, (objects int32, M, rot,
    starts, n_tally, n_settle), the entries' common arguments from threshold to counts_dev, (workspace, its bytes, what `tail` points to)).  Without
    workspace_bytes the workspace holds as many fingers as fit SQUEEZE_WORKSPACE_BYTES, at least one, never more than the call has."""
    if layout not in LABEL_LAYOUTS:
        raise ValueError(f"{who}: layout {layout!r} not supported ({' or '.join(LABEL_LAYOUTS)})")
    st = f64(starts).reshape(-1, 3)
    oi = np.ascontiguousarray(objects, dtype=np.int32).reshape(-1)
    F, M, nt = int(sf.shape[0]), len(oi), int(n_tally)
    ns = int(st.shape[0]) - nt
    if pos_norm is None:
        from .dynamics.dataloader import POS_NORM
        pos_norm = POS_NORM
    if len(threshold) != 3 or len(score_std) != 3:
        raise ValueError(f"{who}: threshold and score_std hold three entries (theta, x, y)")
    cols = 10 + (5 if ns > 0 else 0)
    per_object = layout == "per_object"
    stride = cols if object_stride is None else int(object_stride)
    width = int(column_offset) + ((M - 1) * stride if per_object else 0) + cols
    if out is None:
        out = torch.empty((F, width), dtype=torch.float32, device=sf.device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == F and out.shape[1] >= width
            and out.stride(1) == 1):
        raise ValueError(f"{who}: out must be a float32 device tensor ({F}, >= {width}) with unit column stride")
    T = cfg.theta_cells
    rt = f64(squeeze_rotation_table(T) if rot is None else rot)
    if rt.shape != (T, 2):
        raise ValueError(f"{who}: rot of shape {tuple(rt.shape)} (need ({T}, 2))")
    fit = int(sizer(min(max(F, 1), max(65535 // max(M, 1), 1)), M))      # all fingers in one chunk; negative: what the library refuses
    if fit < 0:
        _check_value(fit)
    if workspace_bytes is not None:
        ws_bytes = int(workspace_bytes)
    elif fit <= SQUEEZE_WORKSPACE_BYTES:
        ws_bytes = fit
    else:                                           # the library cuts the budget into chunks of as many fingers as fit it
        ws_bytes = max(SQUEEZE_WORKSPACE_BYTES, int(sizer(1, M)))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=sf.device)
    cnt = torch.empty((F, 3), dtype=torch.int32, device=sf.device) if counts else None
    thr = (C.c_double * 3)(*[float(v) for v in threshold])
    std = (C.c_double * 3)(*[float(v) for v in score_std])
    tail = (thr, std, float(pos_norm), LABEL_LAYOUTS[layout], out.data_ptr(), int(out.stride(0)), int(column_offset), stride, dptr(cnt))
    return out, cnt, (oi, M, rt, st, nt, ns), tail, (ws, ws_bytes, thr, std)


def squeeze_label(surfaces, bank, objects: Sequence[int], starts, n_tally: int, threshold: Sequence[float], score_std: Sequence[float],
                  pos_norm: Optional[float] = None, layout: str = "mean", friction: float = 0.0, rot=None, out: Optional[torch.Tensor] = None,
                  column_offset: int = 0, object_stride: Optional[int] = None, counts: bool = True, workspace_bytes: Optional[int] = None,
                  **config) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dgdm_squeeze_label (include/dgdm_hip.h "squeeze-simulator labels", DESIGN.md §4.1b "source: squeeze") on the current device: the
    eps-net's condition rows of every finger from the squeeze simulator, reduced on the device chunk by chunk - no per-start output is
    stored.  surfaces (F, 2, m) float64; bank (O, nv, 2) float64 polygons in metres; objects: M indices into the bank (pair f * M + k is
    finger f on objects[k]); starts (n_tally + n_settle, 3) float64, the first n_tally tallied after one closing, the rest followed until
    they settle (none: the 10 tally columns only); threshold (rad, m, m) and score_std (rad, m, m); pos_norm: metres per unit of position,
    the dataset's POS_NORM by default; friction: the Coulomb coefficient (0: frictionless); config: the keys of SQUEEZE_DEFAULTS.
    -> (rows, counts): rows (F, gc) float32, gc = 10 (+5) for 'mean' and M times that for 'per_object' - or `out` (F, >= width) float32,
    written at column_offset with object blocks object_stride apart, every other float left alone; counts (F, 3) int32 = the finger's
    tally (pair, start)s that were loose at the start, ended loose, and were cut by the x range (None with counts=False).
    The workspace follows squeeze_tables' rule, counted in fingers: as many fingers as fit SQUEEZE_WORKSPACE_BYTES, at least one, never
    more than the call has; workspace_bytes overrides it and does not change a bit of the rows.  Synchronises the stream once."""
    from .sim.squeeze import check_friction
    cfg = squeeze_config(**config)
    mu = check_friction(friction, "squeeze_label")
    f64 = _squeeze_mover()
    sf, ob = f64(surfaces), f64(bank)
    if sf.dim() != 3 or sf.shape[1] != 2 or ob.dim() != 3 or ob.shape[2] != 2:
        raise ValueError(f"squeeze_label: surfaces (F, 2, m) and bank (O, nv, 2) expected, got {tuple(sf.shape)} and {tuple(ob.shape)}")
    out, cnt, head, tail, keep = _squeeze_label_front("squeeze_label", cfg, f64, sf, objects, starts, n_tally, threshold, score_std, pos_norm, layout, rot,
                                                      out, column_offset, object_stride, counts, workspace_bytes,
                                                      lambda n, M: lib().dgdm_squeeze_label_workspace_bytes(C.byref(cfg), n, M, int(mu > 0.0)))
    oi, M, rt, st, nt, ns = head
    _check_value(lib().dgdm_squeeze_label(C.byref(cfg), dptr(sf), int(sf.shape[0]), int(sf.shape[2]), dptr(ob), int(ob.shape[0]), int(ob.shape[1]),
                                          oi.ctypes.data, M, dptr(rt), dptr(st), nt, ns, mu, *tail, dptr(keep[0]), keep[1], stream_ptr()))
    return out, cnt


def squeeze_objective_values(cells: torch.Tensor, y: torch.Tensor, starts: torch.Tensor, batch: int, objectives: Sequence[_lib.Objective],
                             rowcoef: Optional[torch.Tensor] = None, score_std: Optional[Sequence[float]] = None, **config) -> torch.Tensor:
    """The objectives' VALUES per pair from a squeeze map (include/dgdm_hip.h, dgdm_squeeze_objective_values): cells
    (P, N, 3) int32 and y (P, N, 2) float64 as squeeze_tables returns them, starts (N, 3) float64 on the device, pair p being finger
    p % batch of group p // batch; objectives: one per group; rowcoef (P // batch, N * batch) float32 or None, row n * batch + b as the
    guidance handle lays it out; score_std: (theta rad, x m, y m), the 2-D SCORE_STD by default; config: the map's (theta_cells, x_cells
    and x_half are read) -> (P // batch, batch) float64.  Shapes and dtypes are checked here, the rest by the library (ValueError)."""
    cfg = squeeze_config(**config)
    B = int(batch)
    if score_std is None:
        from .dynamics.dataloader import SCORE_STD
        score_std = SCORE_STD[1]
    if not (isinstance(cells, torch.Tensor) and cells.is_cuda and cells.dtype == torch.int32 and cells.dim() == 3 and cells.shape[2] == 3):
        raise ValueError(f"squeeze_objective_values: int32 device cells (P, N, 3) expected, got {tuple(getattr(cells, 'shape', ()))}")
    P, N = int(cells.shape[0]), int(cells.shape[1])
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float64 and tuple(y.shape) == (P, N, 2)):
        raise ValueError(f"squeeze_objective_values: float64 device y ({P}, {N}, 2) expected, got {tuple(getattr(y, 'shape', ()))}")
    if not (isinstance(starts, torch.Tensor) and starts.is_cuda and starts.dtype == torch.float64 and tuple(starts.shape) == (N, 3)):
        raise ValueError(f"squeeze_objective_values: float64 device starts ({N}, 3) expected, got {tuple(getattr(starts, 'shape', ()))}")
    if B < 1 or P % B or len(objectives) != P // B:
        raise ValueError(f"squeeze_objective_values: {P} pairs in groups of {B} with {len(objectives)} objectives")
    rc = None
    if rowcoef is not None:
        if not (rowcoef.is_cuda and rowcoef.dtype == torch.float32 and rowcoef.numel() == (P // B) * N * B):
            raise ValueError(f"squeeze_objective_values: float32 device rowcoef of {P // B} x {N * B} entries expected, got "
                             f"{tuple(rowcoef.shape)} {rowcoef.dtype}")
        rc = rowcoef.contiguous()
    if len(score_std) != 3:
        raise ValueError("squeeze_objective_values: score_std holds three entries (theta, x, y)")
    cells, y, starts = cells.contiguous(), y.contiguous(), starts.contiguous()
    arr = (_lib.Objective * max(P // B, 1))(*objectives)
    std = (C.c_double * 3)(*[float(v) for v in score_std])
    out = torch.empty((P // B, B), dtype=torch.float64, device=cells.device)
    _check_value(lib().dgdm_squeeze_objective_values(C.byref(cfg), dptr(cells), dptr(y), dptr(starts), P, N, B, arr, dptr(rc), std, dptr(out),
                                                     stream_ptr()))
    return out


def squeeze_slice(meshes, gz, normals: bool = False) -> Dict[str, object]:
    """dgdm_squeeze_slice (include/dgdm_hip.h "squeeze simulator, 3-D fingers"): the cross-sections of triangle meshes on the planes
    z = gz[j].  meshes: a sequence of (vertices (nv, 3) float64 in metres, triangles (nt, 3) int32), host arrays; gz (mv,) strictly
    ascending.  -> segments (n, 4) float64 on the current device = (A_x, A_y, B_x, B_y), listed by (object, level, triangle), and
    offsets (O, mv + 1) int32, host: level j of object o is segments offsets[o, j] .. offsets[o, j + 1] - 1.  Two calls: the count,
    then the emit into a tensor of that size.  Synchronises the stream.
    normals=True: dgdm_squeeze_slice_normals emits instead, and the result also holds 'normals' (n, 3) float64 on the device, every
    segment's crossing triangle's (V1 - V0) x (V2 - V0) - what squeeze_tables_3d's friction_3d reads; segments and offsets are the same
    bits."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError("squeeze_slice: no meshes")
    vs = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3) for v, _ in meshes]
    fs = [np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3) for _, f in meshes]
    verts, tris = np.concatenate(vs), np.concatenate(fs)
    voff = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int64)
    z = np.ascontiguousarray(gz, dtype=np.float64).reshape(-1)
    O, mv = len(meshes), len(z)
    offsets = np.zeros((O, mv + 1), dtype=np.int32)
    n = C.c_int64(0)
    args = (verts.ctypes.data, voff.ctypes.data, tris.ctypes.data, toff.ctypes.data, O, z.ctypes.data, mv)
    _check_value(lib().dgdm_squeeze_slice(*args, None, 0, offsets.ctypes.data, C.byref(n), stream_ptr()))
    dev = torch.device("cuda", torch.cuda.current_device())
    segments = torch.empty((int(n.value), 4), dtype=torch.float64, device=dev)
    if not normals:
        if n.value:
            _check_value(lib().dgdm_squeeze_slice(*args, dptr(segments), int(n.value), offsets.ctypes.data, C.byref(n), stream_ptr()))
        return {"segments": segments, "offsets": offsets}
    nrm = torch.empty((int(n.value), 3), dtype=torch.float64, device=dev)
    if n.value:
        _check_value(lib().dgdm_squeeze_slice_normals(*args, dptr(segments), int(n.value), offsets.ctypes.data, C.byref(n), stream_ptr(), dptr(nrm)))
    return {"segments": segments, "offsets": offsets, "normals": nrm}


def squeeze_tables_3d(surfaces, gx, segments, offsets, pairs, starts=None, rot=None, tables: bool = False, workspace_bytes: Optional[int] = None,
                      friction_3d: float = 0.0, gz=None, normals=None, jam: bool = False, contact: bool = False, **config) -> Dict[str, torch.Tensor]:
    """dgdm_squeeze_map_3d on the current device.  surfaces (F, 2, mv, mu) float64: the lower and upper jaw face at travel 0 on the levels
    and the abscissae gx (mu,), strictly ascending; segments (n, 4) / offsets (O, mv + 1): squeeze_slice's, for the same levels; the
    rest and the outputs as squeeze_tables.  config: the keys of SQUEEZE_DEFAULTS (finger_half_len is unused here).
    friction_3d: the Coulomb coefficient of dgdm_squeeze_map_3d_friction ("squeeze simulator, 3-D fingers, with Coulomb friction": a 3-D
    antipodal jamming rule, not the 2-D `friction`); that entry runs when friction_3d > 0 or when its tables are asked for - jam
    (P, theta_cells, x_cells) int32 and contact (P, theta_cells, x_cells, 2) int32 (the lower and upper contact's code), both also
    returned with tables=True - and it needs gz (mv,), the levels the meshes were sliced on, and normals (n, 3), squeeze_slice(...,
    normals=True)'s; flags then carries 8 / 16 (start / settled cell jammed).  Otherwise dgdm_squeeze_map_3d runs, as it always did."""
    from .sim.squeeze import check_friction
    fmu = check_friction(friction_3d, "squeeze_tables_3d: friction_3d")
    with_friction = fmu > 0.0 or bool(jam) or bool(contact)
    if with_friction and (gz is None or normals is None):
        missing = " and ".join(n for n, v in (("gz", gz), ("normals", normals)) if v is None)
        raise ValueError(f"squeeze_tables_3d: friction_3d (or jam / contact) needs {missing}: the levels the meshes were sliced on and "
                         "squeeze_slice(..., normals=True)'s normals")
    cfg = squeeze_config(**config)
    f64 = _squeeze_mover()
    sf, sg = f64(surfaces), f64(segments).reshape(-1, 4)
    g = np.ascontiguousarray(gx, dtype=np.float64).reshape(-1)
    of = np.ascontiguousarray(offsets, dtype=np.int32)
    if sf.dim() != 4 or sf.shape[1] != 2 or sf.shape[3] != len(g) or of.ndim != 2 or of.shape[1] != sf.shape[2] + 1:
        raise ValueError(f"squeeze_tables_3d: surfaces (F, 2, mv, mu), gx (mu,) and offsets (O, mv + 1) expected, got {tuple(sf.shape)}, "
                         f"{g.shape} and {of.shape}")
    mu, mv, O = int(sf.shape[3]), int(sf.shape[2]), int(of.shape[0])
    sizer = lib().dgdm_squeeze_map_3d_friction_workspace_bytes if with_friction else lib().dgdm_squeeze_map_3d_workspace_bytes
    out, tail, keep = _squeeze_front("squeeze_tables_3d", cfg, f64, lambda n: sizer(C.byref(cfg), n, mu, mv, O), pairs, starts, rot, tables,
                                     workspace_bytes)
    args = (C.byref(cfg), dptr(sf), int(sf.shape[0]), g.ctypes.data, mu, mv, dptr(sg) if len(sg) else None, int(len(sg)), of.ctypes.data, O) + tail
    if not with_friction:
        _check_value(lib().dgdm_squeeze_map_3d(*args))
        return out
    z = np.ascontiguousarray(gz, dtype=np.float64).reshape(-1)
    nr = f64(normals).reshape(-1, 3)
    if len(z) != mv or len(nr) != len(sg):
        raise ValueError(f"squeeze_tables_3d: gz ({mv},) and normals ({len(sg)}, 3) expected, got {z.shape} and {tuple(nr.shape)}")
    shape = (len(keep[0]), cfg.theta_cells, cfg.x_cells)
    if tables or jam:
        out["jam"] = torch.empty(shape, dtype=torch.int32, device=sf.device)
    if tables or contact:
        out["contact"] = torch.empty(shape + (2,), dtype=torch.int32, device=sf.device)
    _check_value(lib().dgdm_squeeze_map_3d_friction(*args, z.ctypes.data, dptr(nr) if len(nr) else None, fmu, dptr(out.get("jam")),
                                                    dptr(out.get("contact"))))
    return out


def squeeze_label_3d(surfaces, gx, segments, offsets, objects: Sequence[int], starts, n_tally: int, threshold: Sequence[float],
                     score_std: Sequence[float], pos_norm: Optional[float] = None, layout: str = "mean", rot=None, out: Optional[torch.Tensor] = None,
                     column_offset: int = 0, object_stride: Optional[int] = None, counts: bool = True, tables: bool = False,
                     workspace_bytes: Optional[int] = None, **config):
    """dgdm_squeeze_label_3d (include/dgdm_hip.h "squeeze-simulator labels, 3-D fingers", DESIGN.md §4.1b "source: squeeze_3d") on the
    current device: squeeze_label's rows for 3-D fingers from the sliced squeeze.  surfaces (F, 2, mv, mu) float64, gx (mu,), segments
    (n, 4) / offsets (O, mv + 1): squeeze_tables_3d's (the bank is the O sliced meshes); objects: M indices into the bank; everything
    else, the workspace rule and (rows, counts) as squeeze_label - there is no friction.  tables=True -> (rows, counts, tables): S /
    touch_l / touch_r (F * M, theta_cells, x_cells) float64 of every pair, finger-major, for comparison with squeeze_tables_3d's.
    Synchronises the stream once."""
    cfg = squeeze_config(**config)
    f64 = _squeeze_mover()
    sf, sg = f64(surfaces), f64(segments).reshape(-1, 4)
    g = np.ascontiguousarray(gx, dtype=np.float64).reshape(-1)
    of = np.ascontiguousarray(offsets, dtype=np.int32)
    if sf.dim() != 4 or sf.shape[1] != 2 or sf.shape[3] != len(g) or of.ndim != 2 or of.shape[1] != sf.shape[2] + 1:
        raise ValueError(f"squeeze_label_3d: surfaces (F, 2, mv, mu), gx (mu,) and offsets (O, mv + 1) expected, got {tuple(sf.shape)}, "
                         f"{g.shape} and {of.shape}")
    mu, mv, O = int(sf.shape[3]), int(sf.shape[2]), int(of.shape[0])
    out, cnt, head, tail, keep = _squeeze_label_front("squeeze_label_3d", cfg, f64, sf, objects, starts, n_tally, threshold, score_std, pos_norm, layout,
                                                      rot, out, column_offset, object_stride, counts, workspace_bytes,
                                                      lambda n, M: lib().dgdm_squeeze_label_3d_workspace_bytes(C.byref(cfg), n, M, mu, mv, O))
    oi, M, rt, st, nt, ns = head
    shape = (int(sf.shape[0]) * M, cfg.theta_cells, cfg.x_cells)
    tab = {k: torch.empty(shape, dtype=torch.float64, device=sf.device) for k in ("S", "touch_l", "touch_r")} if tables else {}
    _check_value(lib().dgdm_squeeze_label_3d(C.byref(cfg), dptr(sf), int(sf.shape[0]), g.ctypes.data, mu, mv, dptr(sg) if len(sg) else None, int(len(sg)),
                                             of.ctypes.data, O, oi.ctypes.data, M, dptr(rt), dptr(st), nt, ns, *tail, dptr(tab.get("S")),
                                             dptr(tab.get("touch_l")), dptr(tab.get("touch_r")), dptr(keep[0]), keep[1], stream_ptr()))
    return (out, cnt, tab) if tables else (out, cnt)


def squeeze_values_3d(surfaces, gx, segments, offsets, group_first: Sequence[int], batch: int, objectives: Sequence[_lib.Objective], starts,
                      rowcoef: Optional[torch.Tensor] = None, score_std: Optional[Sequence[float]] = None, rot=None, tables: bool = False,
                      workspace_bytes: Optional[int] = None, **config):
    """dgdm_squeeze_values_3d (include/dgdm_hip.h "squeeze objective of 3-D fingers") on the current device: the
    objectives' VALUES of groups of 3-D fingers from the sliced squeeze - squeeze_tables_3d followed by squeeze_objective_values, bit for
    bit, with no per-start output stored and the tables made for blocks of fingers that meet the same object.  surfaces (F, 2, mv, mu)
    float64, gx (mu,), segments (n, 4) / offsets (O, mv + 1): squeeze_tables_3d's; group g is the `batch` consecutive fingers from
    group_first[g] on, against the bank's object objectives[g].object (two groups may name the same fingers); starts (N, 3) float64;
    rowcoef (groups, N * batch) float32 or None, as the guidance handle lays it out; score_std (theta rad, x m, y m), the 3-D SCORE_STD
    by default; config: the keys of SQUEEZE_DEFAULTS -> (groups, batch) float64; tables=True -> (values, tables): S / touch_l / touch_r
    (groups * batch, theta_cells, x_cells) float64 in pair order, for comparison with squeeze_tables_3d's.  The workspace follows
    squeeze_label_3d's rule, counted in groups: as many groups as fit SQUEEZE_WORKSPACE_BYTES, at least one, never more than the call
    has; workspace_bytes overrides it and does not change a bit of the values.  Synchronises the stream once."""
    cfg = squeeze_config(**config)
    f64 = _squeeze_mover()
    sf, sg = f64(surfaces), f64(segments).reshape(-1, 4)
    g = np.ascontiguousarray(gx, dtype=np.float64).reshape(-1)
    of = np.ascontiguousarray(offsets, dtype=np.int32)
    if sf.dim() != 4 or sf.shape[1] != 2 or sf.shape[3] != len(g) or of.ndim != 2 or of.shape[1] != sf.shape[2] + 1:
        raise ValueError(f"squeeze_values_3d: surfaces (F, 2, mv, mu), gx (mu,) and offsets (O, mv + 1) expected, got {tuple(sf.shape)}, "
                         f"{g.shape} and {of.shape}")
    mu, mv, O = int(sf.shape[3]), int(sf.shape[2]), int(of.shape[0])
    gf = np.ascontiguousarray(group_first, dtype=np.int32).reshape(-1)
    n_groups, B = len(gf), int(batch)
    if len(objectives) != n_groups:
        raise ValueError(f"squeeze_values_3d: {n_groups} groups with {len(objectives)} objectives")
    if score_std is None:
        from .dynamics.dataloader import SCORE_STD
        score_std = SCORE_STD[0]
    if len(score_std) != 3:
        raise ValueError("squeeze_values_3d: score_std holds three entries (theta, x, y)")
    st = f64(starts).reshape(-1, 3)
    N, T = int(st.shape[0]), cfg.theta_cells
    rt = f64(squeeze_rotation_table(T) if rot is None else rot)
    if rt.shape != (T, 2):
        raise ValueError(f"squeeze_values_3d: rot of shape {tuple(rt.shape)} (need ({T}, 2))")
    rc = None
    if rowcoef is not None:
        if not (isinstance(rowcoef, torch.Tensor) and rowcoef.is_cuda and rowcoef.dtype == torch.float32 and rowcoef.numel() == n_groups * N * max(B, 0)):
            raise ValueError(f"squeeze_values_3d: float32 device rowcoef of {n_groups} x {N * B} entries expected, got "
                             f"{tuple(getattr(rowcoef, 'shape', ()))} {getattr(rowcoef, 'dtype', None)}")
        rc = rowcoef.contiguous()
    sizer = lambda n: int(lib().dgdm_squeeze_values_3d_workspace_bytes(C.byref(cfg), n, B, mu, mv, O))      # noqa: E731
    fit = sizer(min(max(n_groups, 1), max(65535 // max(B, 1), 1)))       # all groups in one chunk; negative: what the library refuses
    if fit < 0:
        _check_value(fit)
    if workspace_bytes is not None:
        ws_bytes = int(workspace_bytes)
    elif fit <= SQUEEZE_WORKSPACE_BYTES:
        ws_bytes = fit
    else:                                           # the library cuts the budget into chunks of as many groups as fit it
        ws_bytes = max(SQUEEZE_WORKSPACE_BYTES, sizer(1))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=sf.device)
    values = torch.empty((n_groups, max(B, 0)), dtype=torch.float64, device=sf.device)
    shape = (n_groups * max(B, 0), T, cfg.x_cells)
    tab = {k: torch.empty(shape, dtype=torch.float64, device=sf.device) for k in ("S", "touch_l", "touch_r")} if tables else {}
    arr = (_lib.Objective * max(n_groups, 1))(*objectives)
    std = (C.c_double * 3)(*[float(v) for v in score_std])
    _check_value(lib().dgdm_squeeze_values_3d(C.byref(cfg), dptr(sf), int(sf.shape[0]), g.ctypes.data, mu, mv, dptr(sg) if len(sg) else None,
                                              int(len(sg)), of.ctypes.data, O, dptr(rt), dptr(st), N, n_groups, B, gf.ctypes.data, arr, dptr(rc), std,
                                              dptr(values), dptr(tab.get("S")), dptr(tab.get("touch_l")), dptr(tab.get("touch_r")), dptr(ws), ws_bytes,
                                              stream_ptr()))
    return (values, tab) if tables else values


def prof_enable(on: bool) -> None:
    check(lib().dgdm_prof_enable(int(on)))


STAGES = ("trunk", "unet", "xobj", "tables", "guide_misc", "ddim")      # include/dgdm_hip.h DGDM_STAGE_*


def prof_read_stages() -> Dict[str, Tuple[int, float, float]]:
    """{stage: (bracketed regions, total ms, algorithmic work)} since prof_enable(True); clears the records."""
    out = {}
    for i, name in enumerate(STAGES):
        n, ms, wk = C.c_int64(), C.c_double(), C.c_double()
        check(lib().dgdm_prof_read_stage(i, C.byref(n), C.byref(ms), C.byref(wk)))
        out[name] = (n.value, ms.value, wk.value)
    return out


def prof_read() -> Tuple[int, float, float]:
    n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
    check(lib().dgdm_prof_read(C.byref(n), C.byref(ms), C.byref(fl)))
    return n.value, ms.value, fl.value
