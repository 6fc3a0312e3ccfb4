"""Layer-by-layer comparison of the native U-Net forward against the oracle (GPU box).

  python tools/debug_layers.py [--hw 32] [--n 3]
Prints rel-L2 of every tapped block output (NHWC) vs the oracle's intermediate.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffusion-model_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from dmx import synth  # noqa: E402
from oracle.taps import oracle_taps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=32)
    ap.add_argument("--n", type=int, default=3)
    a = ap.parse_args()
    from models.unet_cond_geom import UnetCondWithGeomHead
    sd = synth.unet_cond_geom_weights(0)
    m = UnetCondWithGeomHead()
    m.load_state_dict(sd)
    dev = torch.device("cuda:0")
    m.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    x = torch.randn((a.n, 4, a.hw, a.hw), generator=g)
    t = torch.tensor([1000, 517, 1, 42, 7] * (a.n // 5 + 1))[: a.n]
    y = torch.tensor([0, 2, 3, 1, 1] * (a.n // 5 + 1))[: a.n]
    vals = torch.rand((a.n, 12), generator=g)
    mask = (torch.rand((a.n, 12), generator=g) > 0.5).float()
    with torch.no_grad():
        nat = m.native().forward_taps(x.to(dev), t.to(dev), y.to(dev), vals.to(dev), mask.to(dev))
        ora = oracle_taps(sd, x, t, y, vals, mask)
    for k, v in nat.items():
        v = v.flatten().double().cpu()
        if k not in ora:
            print(f"{k:14s} (no oracle)  norm={float(v.norm()):.4e}")
            continue
        o = ora[k].double()
        if o.numel() != v.numel():
            print(f"{k:14s} SIZE MISMATCH native {v.numel()} oracle {o.numel()}")
            continue
        r = float((v - o).norm() / o.norm().clamp_min(1e-30))
        print(f"{k:14s} rel={r:.3e}  maxabs={float((v - o).abs().max()):.3e}  norm={float(o.norm()):.4e}")


if __name__ == "__main__":
    main()
