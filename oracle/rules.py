"""The sampling rules of include/dmx.h restated in torch, once (TEST INFRASTRUCTURE).

Pure torch on top of oracle.ref: nothing here imports dmx, diff or the library, so host tests and tools
use it without a device.  Tables come in as arguments (Diffuser.ddim_tables(..., "cpu") and its kin).
Every function keeps the dtype of its inputs and spends one torch op per IEEE operation, in the order
dmx.h states: fp32 inputs give the bit-exact fp32 reference, float64 inputs the float64 one.  The rule of
the next sampling feature goes here, not into its test file.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import ref

ALL6 = ("sa1", "sa2", "sa3", "sa4", "sa5", "sa6")


def rel(a, b):
    """rel-L2 of a against b, in double on the CPU."""
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class Foreign(torch.nn.Module):
    """A network behind a wrapper that is not a dmx network (no .native()): every step takes the
    model-call + standalone-update path."""

    def __init__(self, inner):
        super().__init__()
        self.inner = [inner]

    def forward(self, x, t, y, cond_vals=None, cond_mask=None):
        return self.inner[0](x, t, y, cond_vals=cond_vals, cond_mask=cond_mask)


def row(k, pos):
    """Row pos - 1 of the table k, pos an int or (B,) long: broadcasts over (B,C,h,w)."""
    return k[pos - 1].view(-1, 1, 1, 1)


# ---- the updates ------------------------------------------------------------------------------------
def ddim_update(x, eps, pos, sched, nz=None):
    """dmx_ddim_sched:  x0 = (x - k_e eps) / k_a;  x' = (k_s x0 + k_d eps) + k_n nz.
    nz None: the noise term is not added at all (eta = 0: k_n = 0, nothing read or drawn)."""
    _, k_e, k_a, k_s, k_d, k_n = sched
    x0 = (x - row(k_e, pos) * eps) / row(k_a, pos)
    out = row(k_s, pos) * x0 + row(k_d, pos) * eps
    return out if nz is None else out + row(k_n, pos) * nz


def dpm_update(x, eps, pos, sched, hist):
    """dmx_dpm_sched:  x0 = (x - k_e eps) / k_a;  y = k_x x + k_c x0;  x' = y + k_p hist where k_p != 0,
    else y;  hist <- x0.  -> (x', x0).  hist is a select's unused side where k_p == 0: NaN there is harmless."""
    _, k_e, k_a, k_x, k_c, k_p = sched
    x0 = (x - row(k_e, pos) * eps) / row(k_a, pos)
    y = row(k_x, pos) * x + row(k_c, pos) * x0
    return torch.where(row(k_p, pos) != 0, y + row(k_p, pos) * hist, y), x0


def invert_update(src, eps, c, tables):
    """dmx_invert_sched, row c - 1 (c: countdown positions):  y = i_x src + i_e eps;  src <- y where
    adv != 0.  -> (y, src afterwards)."""
    _, i_x, i_e, adv = tables
    y = row(i_x, c) * src + row(i_e, c) * eps
    return y, torch.where(row(adv, c) != 0, y, src)


def known_blend(xg, z0, e0, m, pos, tabs):
    """dmx_known_sched:  kn = q_a z0 + q_e e0;  x' = kn where m == 0, xg where m == 1, else
    m xg + (1 - m) kn.  m None: every element kept, kn is returned and xg not read."""
    kn = row(tabs[0], pos) * z0 + row(tabs[1], pos) * e0
    if m is None:
        return kn
    return torch.where(m == 0, kn, torch.where(m == 1, xg, m * xg + (1 - m) * kn))


# ---- the mixes ----------------------------------------------------------------------------------------
def compose_mix(es, w):
    """dmx_compose, es: K + 1 tensors (n,c,h,w), es[0] the base; w (K,n):
    d_k = e_k - e_0;  s = w_1 d_1;  s = s + w_k d_k (k = 2..K);  eps = e_0 + s."""
    def col(k):
        return w[k].view(-1, 1, 1, 1)
    s = col(0) * (es[1] - es[0])
    for k in range(2, len(es)):
        s = s + col(k - 1) * (es[k] - es[0])
    return es[0] + s


def cfg_rescale(eu, ec, g, phi):
    """dmx_guidance:  eg = eu + g (ec - eu) in the inputs' dtype;  r[n] = 1 + phi (std(ec[n]) / std(eg[n]) - 1)
    in double over each sample's elements, 1 where std(eg[n]) is not a positive finite number.
    -> (eg, r as double); the step's eps is eg * r cast to eg's dtype."""
    eg = eu + g * (ec - eu)
    sg = eg.double().flatten(1).std(1)
    sc = ec.double().flatten(1).std(1)
    ok = torch.isfinite(sg) & (sg > 0)
    r = torch.where(ok, 1.0 + phi * (sc / torch.where(ok, sg, torch.ones_like(sg)) - 1.0), torch.ones_like(sg))
    return eg, r


def cfg_rescaled(eu, ec, g, phi):
    """dmx_guidance: the step's eps = eg * fp32(r[n]) of cfg_rescale."""
    eg, r = cfg_rescale(eu, ec, g, phi)
    return eg * r.float().view(-1, 1, 1, 1)


def to_eps(out, x_net, t, p_o, p_x):
    """dmx_model_set_prediction (DMX_PRED_V), at the network timesteps t:  eps = p_o[t-1] out + p_x[t-1] x_net,
    x_net the latent the network was evaluated at."""
    return row(p_o, t) * out + row(p_x, t) * x_net


# ---- predictions from the oracle ----------------------------------------------------------------------
def cfg_eps(sd, x, t, y, vals, mask, guidance=3.0, null_label=0):
    """The step's prediction at the network timesteps t (not positions: a caller holding a position maps it
    with sched[0][pos - 1]):  eu + g (ec - eu), or one conditional forward where g is not positive."""
    with torch.no_grad():
        ec, _ = ref.unet_cond_geom_forward(sd, x, t, y, vals, mask)
        if not guidance > 0:
            return ec
        eu, _ = ref.unet_cond_geom_forward(sd, x, t, torch.full_like(y, null_label), vals, mask)
    return eu + guidance * (ec - eu)


def guided_eps(sd, x, t, y, vals, mask, guided, phi=0.0, g=3.0):
    """A step under a guidance interval: one conditional forward where not `guided`, else CFG over the null
    label 0, rescaled where phi > 0 -> (eps, r or None)."""
    ec, _ = ref.unet_cond_geom_forward(sd, x, t, y, vals, mask)
    if not guided:
        return ec, None
    eu, _ = ref.unet_cond_geom_forward(sd, x, t, torch.zeros_like(y), vals, mask)
    eg, r = cfg_rescale(eu, ec, g, phi)
    return (eg * r.float().view(-1, 1, 1, 1) if phi > 0 else eg), r


@contextlib.contextmanager
def identity_attention(names):
    """dmx_perturb: ref.attention with softmax(s) = I in the blocks `names` — the attention output of a
    token is its own value vector.  unet_trunk looks `attention` up at call time; the original is restored."""
    orig = ref.attention

    def attention(sd, p, x):
        if p not in names:
            return orig(sd, p, x)
        n, c, hh, ww = x.shape
        tok = x.reshape(n, c, hh * ww).transpose(1, 2)
        xl = F.layer_norm(tok, (c,), sd[f"{p}.ln.weight"], sd[f"{p}.ln.bias"], 1e-5)
        qkv = F.linear(xl, sd[f"{p}.mha.in_proj_weight"], sd[f"{p}.mha.in_proj_bias"])
        a = F.linear(qkv[..., 2 * c:], sd[f"{p}.mha.out_proj.weight"], sd[f"{p}.mha.out_proj.bias"]) + xl
        f = F.layer_norm(a, (c,), sd[f"{p}.ff_self.0.weight"], sd[f"{p}.ff_self.0.bias"], 1e-5)
        f = F.linear(f, sd[f"{p}.ff_self.1.weight"], sd[f"{p}.ff_self.1.bias"])
        f = F.linear(F.gelu(f), sd[f"{p}.ff_self.3.weight"], sd[f"{p}.ff_self.3.bias"])
        return (f + a).transpose(1, 2).reshape(n, c, hh, ww)

    ref.attention = attention
    try:
        yield
    finally:
        ref.attention = orig


def perturbed_forward(sd, x, t, y, vals, mask, names=()):
    """The oracle's eps with identity attention in the blocks `names` (() = the plain forward)."""
    with identity_attention(set(names)) if names else contextlib.nullcontext(), torch.no_grad():
        return ref.unet_cond_geom_forward(sd, x, t, y, vals, mask)[0]


def composed_eps(sd, x, t, comp, pt=None):
    """dmx_compose (+ dmx_perturb): one oracle forward per branch of comp = (y_rows, v_rows, m_rows, w), the
    branches of pt = (block bits, branch bits) perturbed in its blocks, then the mix."""
    y_rows, v_rows, m_rows, w = comp
    blocks, branches = pt if pt is not None else (0, 0)
    names = [n for i, n in enumerate(ALL6) if blocks >> i & 1]
    es = [perturbed_forward(sd, x, t, y_rows[k], v_rows[k], m_rows[k], names if branches >> k & 1 else ())
          for k in range(y_rows.shape[0])]
    return compose_mix(es, w)


# ---- one loop for the samplers ------------------------------------------------------------------------
def trajectory(x, rule, sched, eps_of, noise_of=None, p0=None, blend=None):
    """Positions p0 (default S) .. 1 of one sampler from x.  rule "ddpm": sched = ref.schedule(T), position p
    is the timestep p; "ddim" / "dpm": sched the rule's tables, the timestep is sched[0][p - 1].
    eps_of(x, t, pos) -> eps with t and pos (B,) long; noise_of(p) -> the step's noise, called once per
    DDPM / DDIM step after eps_of (None, or no noise_of: DDIM adds no noise term); blend(x, pos) -> x after
    every step.  The DPM history starts as NaN: its first row is first-order and does not read it."""
    B = x.shape[0]
    hist = torch.full_like(x, float("nan"))
    with torch.no_grad():
        for p in range(int(sched[0].numel()) if p0 is None else p0, 0, -1):
            pos = torch.full((B,), p, dtype=torch.long)
            t = pos if rule == "ddpm" else sched[0][pos - 1]
            eps = eps_of(x, t, pos)
            if rule == "ddpm":
                x = ref.ddpm_update(x, eps, t, sched[1], sched[2], noise_of(p))
            elif rule == "ddim":
                x = ddim_update(x, eps, pos, sched, noise_of(p) if noise_of is not None else None)
            else:
                x, hist = dpm_update(x, eps, pos, sched, hist)
            if blend is not None:
                x = blend(x, pos)
    return x
