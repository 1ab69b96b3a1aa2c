"""CPU check of the oracle's eps-net at dimensions other than the shipped ones: ``oracle.unet1d_forward(..., n_groups)`` against a model
assembled here from plain ``torch.nn`` layers, written from the architecture the oracle's docstrings cite (the 1-D conditional U-Net of
Diffusion Policy: sinusoidal step embedding -> Linear -> Mish -> Linear; residual blocks of two Conv1d(k5) -> GroupNorm -> Mish stages with
a FiLM scale | shift from Mish -> Linear of the condition after the first stage and a 1x1 residual convolution where the widths differ;
Conv1d(k3, s2, p1) down, ConvTranspose1d(k4, s2, p1) up, skip concatenation; Conv1d-GroupNorm-Mish and a 1x1 convolution at the end).
The module tree reproduces the state_dict's key names, so the synthetic weights load with ``strict=True``."""
import math

import torch
from torch import nn

from dgdm_amd import synth
from oracle import dgdm_oracle as orc
from tests import cond_oracle as co


class _SinEmb(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, t):
        half = self.dim // 2
        fr = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
        arg = t[:, None] * fr[None, :]
        return torch.cat((arg.sin(), arg.cos()), dim=-1).double()


class _ConvBlock(nn.Module):
    def __init__(self, cin, cout, k, groups):
        super().__init__()
        self.block = nn.Sequential(nn.Conv1d(cin, cout, k, padding=k // 2), nn.GroupNorm(groups, cout), nn.Mish())

    def forward(self, x):
        return self.block(x)


class _ResBlock(nn.Module):
    def __init__(self, cin, cout, cond, k, groups):
        super().__init__()
        self.blocks = nn.ModuleList([_ConvBlock(cin, cout, k, groups), _ConvBlock(cout, cout, k, groups)])
        self.cond_encoder = nn.Sequential(nn.Mish(), nn.Linear(cond, 2 * cout))
        self.residual_conv = nn.Conv1d(cin, cout, 1) if cin != cout else nn.Identity()
        self.cout = cout

    def forward(self, x, cond):
        out = self.blocks[0](x)
        e = self.cond_encoder(cond).reshape(x.shape[0], 2, self.cout, 1)
        out = e[:, 0] * out + e[:, 1]
        out = self.blocks[1](out)
        return out + self.residual_conv(x)


class _Resample(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.conv = conv

    def forward(self, x):
        return self.conv(x)


class _Unet(nn.Module):
    def __init__(self, down_dims, dsed, groups, gc=0, k=5):
        super().__init__()
        d0, d1 = down_dims
        cond = dsed + gc
        self.diffusion_step_encoder = nn.Sequential(_SinEmb(dsed), nn.Linear(dsed, 4 * dsed), nn.Mish(), nn.Linear(4 * dsed, dsed))
        rb = lambda ci, co: _ResBlock(ci, co, cond, k, groups)      # noqa: E731
        self.down_modules = nn.ModuleList([
            nn.ModuleList([rb(1, d0), rb(d0, d0), _Resample(nn.Conv1d(d0, d0, 3, 2, 1))]),
            nn.ModuleList([rb(d0, d1), rb(d1, d1), nn.Identity()])])
        self.mid_modules = nn.ModuleList([rb(d1, d1), rb(d1, d1)])
        self.up_modules = nn.ModuleList([nn.ModuleList([rb(2 * d1, d0), rb(d0, d0), _Resample(nn.ConvTranspose1d(d0, d0, 4, 2, 1))])])
        self.final_conv = nn.Sequential(_ConvBlock(d0, d0, k, groups), nn.Conv1d(d0, 1, 1))

    def forward(self, sample, timestep, global_cond=None):
        x = sample.transpose(1, 2)
        g = self.diffusion_step_encoder(timestep)
        if global_cond is not None:
            g = torch.cat((g, global_cond), dim=-1)
        skips = []
        for r0, r1, down in self.down_modules:
            x = r1(r0(x, g), g)
            skips.append(x)
            x = down(x)
        for m in self.mid_modules:
            x = m(x, g)
        for r0, r1, up in self.up_modules:
            x = torch.cat((x, skips.pop()), dim=1)      # the deepest level's skip; the first level's is never consumed
            x = up(r1(r0(x, g), g))
        return self.final_conv(x).transpose(1, 2)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_oracle_unet_other_dims_vs_torch_nn():
    """down_dims (128, 128) (identity residual in down1.0), n_groups 4, dsed 12, L 6: float64, 1e-12.  The default n_groups = 8 gives a
    different answer on the same weights (the argument is live), and the conditional restatement takes the same argument."""
    dims, groups, dsed, L, B = (128, 128), 4, 12, 6, 3
    sd = {k: v.double() for k, v in synth.synth_state_dict(synth.unet_spec(down_dims=dims, dsed=dsed), 31).items()}
    assert "down_modules.1.0.residual_conv.weight" not in sd
    net = _Unet(dims, dsed, groups).double()
    net.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, L, 1, generator=g, dtype=torch.float64)
    t = torch.tensor([0, 517, 999])
    with torch.no_grad():
        ref = net(x, t)
        got = orc.unet1d_forward(sd, x, t, n_groups=groups)
        assert got.shape == (B, L, 1) and _rel(got, ref) < 1e-12, _rel(got, ref)
        assert _rel(orc.unet1d_forward(sd, x, t), ref) > 1e-3
        assert torch.equal(co.unet1d_forward_cond(sd, x, t, None, n_groups=groups), got)
        # with a condition
        sdc = {k: v.double() for k, v in synth.synth_state_dict(synth.unet_spec(down_dims=dims, dsed=dsed, global_cond_dim=5), 32).items()}
        netc = _Unet(dims, dsed, groups, gc=5).double()
        netc.load_state_dict(sdc, strict=True)
        c = torch.randn(B, 5, generator=g, dtype=torch.float64)
        e = _rel(co.unet1d_forward_cond(sdc, x, t, c, n_groups=groups), netc(x, t, c))
        assert e < 1e-12, e
