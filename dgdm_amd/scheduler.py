"""Host side of the DDIM scheduler the reference takes from diffusers 0.11.1
(``DDIMScheduler(num_train_timesteps, beta_schedule='squaredcos_cap_v2', clip_sample=True,
prediction_type='epsilon')``, generator/train.py:83; dynamics/trainer.py:36).

Only the tables live here (a few hundred floats, built once); the per-element update is the HIP
kernel behind ``dgdm_ddim_guided_step``.  diffusers is not vendored by the reference and is absent
from this image, so this follows the published algorithm - parity unpinned.

Duck-types what ``generator/diffusion.py`` touches: ``timesteps``, ``alphas_cumprod``,
``config.num_train_timesteps``, ``set_timesteps``, ``step(...).prev_sample``, ``add_noise``.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch

from . import engine


class DDIMSchedulerOutput:
    def __init__(self, prev_sample: torch.Tensor):
        self.prev_sample = prev_sample


class DDIMScheduler:
    def __init__(self, num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2", clip_sample: bool = True,
                 prediction_type: str = "epsilon", **unused):
        if beta_schedule != "squaredcos_cap_v2" or not clip_sample or prediction_type != "epsilon":
            raise NotImplementedError("only the configuration generator/train.py:83 uses is implemented")
        T = int(num_train_timesteps)
        self.config = SimpleNamespace(num_train_timesteps=T, beta_schedule=beta_schedule, clip_sample=clip_sample,
                                      prediction_type=prediction_type)
        bar = lambda s: math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2      # noqa: E731
        self.betas = torch.tensor([min(1 - bar((i + 1) / T) / bar(i / T), 0.999) for i in range(T)], dtype=torch.float32)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.from_numpy(np.arange(0, T)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        self.num_inference_steps = int(num_inference_steps)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        self.timesteps = torch.from_numpy((np.arange(0, self.num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64))

    def coefficients(self, t: int, eta: Optional[float] = None):
        """float32 sqrt(abar_t), sqrt(1-abar_t), sqrt(abar_prev), sqrt(1-abar_prev) as the reference's tensor ops give them.

        eta given: those four followed by (sigma, dir) of ``eta_coefficients`` - six values."""
        t = int(t)
        prev = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        four = (float(a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_p ** 0.5), float((1 - a_p) ** 0.5))
        return four if eta is None else four + self.eta_coefficients(t, eta)

    def eta_coefficients(self, t: int, eta: float) -> Tuple[float, float]:
        """(sigma, dir) of the stochastic step, diffusers 0.11.1 ``DDIMScheduler.step(eta=...)`` restated in the float32 tensor
        operations it uses (``_get_variance``, ``std_dev_t = eta * variance ** 0.5``, ``(1 - alpha_prod_t_prev - std_dev_t**2) ** 0.5``):

            variance = (1 - abar_prev) / (1 - abar_t) * (1 - abar_t / abar_prev)
            sigma    = eta * variance ** 0.5
            dir      = (1 - abar_prev - sigma**2) ** 0.5
            x_prev   = sqrt(abar_prev) * clip(x0_pred) + dir * eps + sigma * z

        with ``clip_sample=True``, ``use_clipped_model_output=False`` (eps is NOT re-derived from the clipped x0) and epsilon prediction.
        The last step has abar_prev = final_alpha_cumprod = 1, hence sigma = 0: no noise enters a finished design.  eta = 0 gives
        dir == sqrt(1-abar_prev) of ``coefficients`` bit for bit.  diffusers is not on hand to compare with: parity unpinned, like the
        eta = 0 step."""
        t = int(t)
        prev = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        variance = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        sigma = float(eta) * variance ** 0.5
        return (float(sigma), float((1 - a_p - sigma ** 2) ** 0.5))

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, eta: float = 0.0, bounds=None, variance_noise=None,
             noise_key=None, **unused) -> DDIMSchedulerOutput:
        """bounds (not a diffusers argument): an edit's (lo, hi) per entry, which replace clip_sample's [-1, 1] (dgdm_amd/edit.py).

        eta > 0 needs a noise source: ``variance_noise``, a tensor like `sample` (diffusers' own argument), or ``noise_key = (seed, key,
        step_index)`` (not a diffusers argument), the keyed device normal of include/dgdm_hip.h for ONE chain: `sample` as a whole is the
        chain, element for element.  Neither: ValueError - this scheduler does not draw from a torch generator."""
        coef = self.coefficients(int(timestep))
        if eta == 0.0:
            return DDIMSchedulerOutput(engine.ddim_guided_step(sample, model_output, None, 0, coef, 0.0, bounds))
        if variance_noise is None and noise_key is None:
            raise ValueError("eta > 0 needs variance_noise or noise_key=(seed, key, step_index)")
        if variance_noise is not None and noise_key is not None:
            raise ValueError("variance_noise and noise_key are two sources of the same noise: give one")
        kw = dict(variance_noise=variance_noise)
        if noise_key is not None:
            seed, key, step_index = noise_key
            kw = dict(seed=int(seed), chain_keys=[int(key)], step_index=int(step_index))
        return DDIMSchedulerOutput(engine.ddim_guided_step(sample, model_output, None, 0, coef, 0.0, bounds,
                                                           eta_coef=self.eta_coefficients(int(timestep), eta), **kw))

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        ts = torch.unique(timesteps.detach().cpu())
        if len(ts) != 1:
            raise NotImplementedError("add_noise is used with one shared timestep on the sampling path (generator/diffusion.py:184-189)")
        a = self.alphas_cumprod[int(ts[0])]
        return engine.ddim_add_noise(original_samples, noise, float(a ** 0.5), float((1 - a) ** 0.5))
