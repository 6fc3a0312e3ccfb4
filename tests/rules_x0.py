"""The x0-form rules of include/dmx.h (dmx_model_set_prediction_x0) restated in torch (TEST INFRASTRUCTURE).

In the style of oracle/rules.py, where they belong once that module may change: pure torch, tables as
arguments, one torch op per IEEE operation in the order dmx.h states, dtype-preserving — fp32 inputs give
the bit-exact fp32 reference, float64 inputs the float64 one.  Nothing here imports dmx, diff or the library.
"""
import contextlib

import torch

from oracle import ref, rules
from oracle.rules import rel, row, trajectory  # noqa: F401  (re-exported for the tests)


def x0_split(out, x_net, t, p_o, p_x):
    """The conversion at the network timesteps t, x_net the latent the network was evaluated at:
    x0 = p_o[t-1] x_net - p_x[t-1] out;  eps = p_o[t-1] out + p_x[t-1] x_net.  -> (x0, eps)"""
    po, px = row(p_o, t), row(p_x, t)
    return po * x_net - px * out, po * out + px * x_net


def ddpm_x0_update(x0, eps, t, d_s, d_d, sd, nz):
    """x' = (d_s[t-1] x0 + d_d[t-1] eps) + nz sd[t-1], nz = 0 at t == 1."""
    nz = nz.clone()
    nz[t == 1] = 0
    return (row(d_s, t) * x0 + row(d_d, t) * eps) + nz * row(sd, t)


def ddim_x0_update(x0, eps, pos, sched, nz=None):
    """dmx_ddim_sched in x0-form:  x' = (k_s x0 + k_d eps) + k_n nz;  k_e and k_a are not read.
    nz None: the noise term is not added at all."""
    _, _, _, k_s, k_d, k_n = sched
    out = row(k_s, pos) * x0 + row(k_d, pos) * eps
    return out if nz is None else out + row(k_n, pos) * nz


def dpm_x0_update(x, x0, pos, sched, hist):
    """dmx_dpm_sched in x0-form:  y = k_x x + k_c x0;  x' = y + k_p hist where k_p != 0, else y;  hist <- x0.
    -> (x', x0).  No eps; k_e and k_a are not read."""
    _, _, _, k_x, k_c, k_p = sched
    y = row(k_x, pos) * x + row(k_c, pos) * x0
    return torch.where(row(k_p, pos) != 0, y + row(k_p, pos) * hist, y), x0


def posterior_sd(alphas, alpha_bars):
    """coef_tables' sd with alpha_bar_prev clamped to 1 at t = 1, in the inputs' dtype."""
    abp = torch.cat([torch.ones_like(alpha_bars[:1]), alpha_bars[:-1]])
    return torch.sqrt((1 - alphas) * (1 - abp) / (1 - alpha_bars))


@contextlib.contextmanager
def x0_rules(p_o, p_x, d_s, d_d):
    """oracle.rules.trajectory with the x0-form updates: inside, what its eps_of returns is read as the mixed
    network output and x as the latent it was evaluated at; its "ddpm" schedule is (betas, alphas, alpha_bars)
    of the Diffuser.  The three updates trajectory looks up at call time are replaced and restored (as
    rules.identity_attention does with ref.attention)."""
    def ddpm(x, out, t, alphas, alpha_bars, noise, clamp_prev=True):
        x0, eps = x0_split(out, x, t, p_o, p_x)
        return ddpm_x0_update(x0, eps, t, d_s, d_d, posterior_sd(alphas, alpha_bars), noise)

    def ddim(x, out, pos, sched, nz=None):
        x0, eps = x0_split(out, x, sched[0][pos - 1], p_o, p_x)
        return ddim_x0_update(x0, eps, pos, sched, nz)

    def dpm(x, out, pos, sched, hist):
        x0, _ = x0_split(out, x, sched[0][pos - 1], p_o, p_x)
        return dpm_x0_update(x, x0, pos, sched, hist)

    saved = ref.ddpm_update, rules.ddim_update, rules.dpm_update
    ref.ddpm_update, rules.ddim_update, rules.dpm_update = ddpm, ddim, dpm
    try:
        yield
    finally:
        ref.ddpm_update, rules.ddim_update, rules.dpm_update = saved
