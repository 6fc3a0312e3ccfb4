"""The oracle's intermediates of one conditional U-Net forward, under the names of the native debug taps
(NativeModel.forward_taps; TEST INFRASTRUCTURE ONLY, see ``oracle/__init__.py``).

Every block output is recomputed with the functions of ``oracle/ref.py`` in the order unet_trunk runs
them, so ``oracle_taps(...)["eps"]`` is unet_cond_geom_forward's eps bit for bit.  Nothing is cast: the
taps run in the dtype of the weights and inputs they are handed (float64 weights and inputs give the
float64 taps; t and y stay integers and the sinusoidal table of t keeps the reference's fp32 values).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ref


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().flatten() if t.dim() == 4 else t.flatten()


def oracle_taps(sd, x, t, y, vals, mask):
    """{tap name: flat tensor, sample-major (NHWC / (N, L, C) order; eps NCHW as the model returns it)}."""
    T = {}
    emb = ref.cond_embedding(sd, t, y, vals, mask)
    heads = [F.linear(F.silu(emb), sd[f"{b}.emb_layer.1.weight"], sd[f"{b}.emb_layer.1.bias"])
             for b in ("down1", "down2", "down3", "up1", "up2", "up3")]
    T["emb"] = torch.cat(heads, dim=1).flatten()

    def res(name, p, h, residual):
        T[name + ".r1"] = nhwc(F.conv2d(h, sd[f"{p}.double_conv.0.weight"], None, 1, 1))
        o = ref.resblock(sd, p, h, residual)
        T[name] = nhwc(o)
        return o

    def attn(name, h):
        n, c, hh, ww = h.shape
        tok = h.reshape(n, c, hh * ww).transpose(1, 2)
        xl = F.layer_norm(tok, (c,), sd[f"{name}.ln.weight"], sd[f"{name}.ln.bias"], 1e-5)
        T[name + ".xl"] = xl.flatten()
        T[name + ".qkv"] = F.linear(xl, sd[f"{name}.mha.in_proj_weight"], sd[f"{name}.mha.in_proj_bias"]).flatten()
        o = ref.attention(sd, name, h)
        T[name] = nhwc(o)
        return o

    x1 = res("inc", "inc", x, False)
    cur = x1
    skips = []
    for i in range(3):
        skips.append(cur)
        d = f"down{i + 1}"
        h0 = res(d + ".0", d + ".maxpool_conv.1", F.max_pool2d(cur, 2), True)
        h1 = ref.resblock(sd, d + ".maxpool_conv.2", h0, False) + ref.emb_head(sd, d, emb)
        T[d + ".1"] = nhwc(h1)
        cur = attn(f"sa{i + 1}", h1)
    for i, b in enumerate(("bot1", "bot2", "bot3")):
        cur = res(f"bot{i + 1}", b, cur, False)
    for i in range(3):
        u = f"up{i + 1}"
        skip = skips[2 - i]
        h = F.interpolate(cur, scale_factor=2, mode="bilinear", align_corners=True)
        dy, dx = skip.size(2) - h.size(2), skip.size(3) - h.size(3)
        if dy or dx:
            h = F.pad(h, [max(0, dx // 2), max(0, dx - dx // 2), max(0, dy // 2), max(0, dy - dy // 2)])
        h = torch.cat([skip, h], 1)
        h0 = res(u + ".0", u + ".conv.0", h, True)
        h1 = ref.resblock(sd, u + ".conv.1", h0, False) + ref.emb_head(sd, u, emb)
        T[u + ".1"] = nhwc(h1)
        cur = attn(f"sa{4 + i}", h1)
    T["eps"] = F.conv2d(cur, sd["out.weight"], sd["out.bias"]).flatten()
    return T
