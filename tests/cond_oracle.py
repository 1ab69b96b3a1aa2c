"""Restatement for the conditional eps-net tests: ``ConditionalUnet1D.forward(sample, timestep, global_cond)``
(generator/diffusion_utils.py:238-285) composed from the oracle's own blocks, and one training step as its autograd.

Every block's FiLM vector is ``cond_encoder(cat(step embedding, global_cond))``; ``oracle.dgdm_oracle._film_res_block`` applies the
encoder's Mish to whatever it is handed, so feeding it the concatenation IS the reference's arithmetic (pinned to the reference's own
class by tests/test_cond_oracle.py on tests/golden/g15_unet_cond.npz).  Works in float32 or float64 according to ``sd``."""
import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import dgdm_oracle as orc

SD = Dict[str, torch.Tensor]


def global_cond_dim(sd: SD) -> int:
    return int(sd["mid_modules.0.cond_encoder.1.weight"].shape[1] - sd["diffusion_step_encoder.1.weight"].shape[1])


def unet1d_forward_cond(sd: SD, sample: torch.Tensor, timestep: torch.Tensor, cond: Optional[torch.Tensor], n_groups: int = 8) -> torch.Tensor:
    """sample (B, L, 1), timestep (B,), cond (B, gc) or None (gc == 0) -> (B, L, 1), in sd's dtype."""
    dt = sd["diffusion_step_encoder.1.weight"].dtype
    x = sample.to(dt).transpose(1, 2)
    dsed = sd["diffusion_step_encoder.1.weight"].shape[1]
    half = dsed // 2
    fr = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
    arg = timestep.expand(x.shape[0])[:, None] * fr[None, :]
    g = torch.cat((arg.sin(), arg.cos()), dim=-1).to(dt)
    g = F.linear(g, sd["diffusion_step_encoder.1.weight"], sd["diffusion_step_encoder.1.bias"])
    g = F.linear(F.mish(g), sd["diffusion_step_encoder.3.weight"], sd["diffusion_step_encoder.3.bias"])
    if cond is not None:
        g = torch.cat((g, cond.to(dt)), dim=-1)                                  # :254-257
    x = orc._film_res_block(sd, "down_modules.0.0", x, g, n_groups)
    x = orc._film_res_block(sd, "down_modules.0.1", x, g, n_groups)
    x = F.conv1d(x, sd["down_modules.0.2.conv.weight"], sd["down_modules.0.2.conv.bias"], stride=2, padding=1)
    x = orc._film_res_block(sd, "down_modules.1.0", x, g, n_groups)
    skip = x = orc._film_res_block(sd, "down_modules.1.1", x, g, n_groups)
    x = orc._film_res_block(sd, "mid_modules.0", x, g, n_groups)
    x = orc._film_res_block(sd, "mid_modules.1", x, g, n_groups)
    x = torch.cat((x, skip), dim=1)
    x = orc._film_res_block(sd, "up_modules.0.0", x, g, n_groups)
    x = orc._film_res_block(sd, "up_modules.0.1", x, g, n_groups)
    x = F.conv_transpose1d(x, sd["up_modules.0.2.conv.weight"], sd["up_modules.0.2.conv.bias"], stride=2, padding=1)
    x = orc._conv_gn_mish(sd, "final_conv.0", x, n_groups)
    x = F.conv1d(x, sd["final_conv.1.weight"], sd["final_conv.1.bias"])
    return x.transpose(1, 2)


def loss_and_grads(sd: SD, num_train_timesteps: int, x0: torch.Tensor, noise: torch.Tensor, ts: torch.Tensor,
                   cond: Optional[torch.Tensor]) -> Tuple[float, torch.Tensor, SD]:
    """The generator's loss with a condition: noisy = add_noise(x0, noise, t); mse_loss(net(noisy, t, global_cond=c), noise) ->
    (loss, noise prediction, d loss / d every parameter)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    dt = next(iter(p.values())).dtype
    noisy = orc.DDIM(num_train_timesteps).add_noise(x0, noise, ts)
    pred = unet1d_forward_cond(p, noisy, ts, cond)
    loss = F.mse_loss(pred, noise.to(dt))
    loss.backward()
    return float(loss.detach()), pred.detach(), {k: v.grad.detach() for k, v in p.items()}


class CondTrainer:
    """Adam on ``loss_and_grads`` (torch.optim.Adam, as generator/diffusion.py:711-714 configures it)."""

    def __init__(self, sd: SD, num_train_timesteps: int, lr: float):
        self.p = {k: torch.nn.Parameter(v.detach().clone()) for k, v in sd.items()}
        self.T, self.lr = num_train_timesteps, lr
        self.opt = torch.optim.Adam(self.p.values(), lr=lr)
        self.grads: SD = {}

    @property
    def sd(self) -> SD:
        return {k: v.detach() for k, v in self.p.items()}

    def step(self, x0, noise, ts, cond) -> Tuple[float, torch.Tensor]:
        for g in self.opt.param_groups:
            g["lr"] = self.lr
        loss, pred, self.grads = loss_and_grads(self.sd, self.T, x0, noise, ts, cond)
        self.opt.zero_grad()
        for k, v in self.p.items():
            v.grad = self.grads[k].clone()
        self.opt.step()
        return loss, pred
