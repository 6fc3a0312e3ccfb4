"""Time one whole training iteration with the objective in torch ops and in the native kernels.

At the bench.py training leg's shape (B = 32 latents of 4 x 28 x 28, UnetCondWithGeomHead, dmx.optim.Adam,
geom_lambda 0.5, cfg_drop_prob 0.1) two loops take turns in one process on one model:

    torch-op loop      torch.randint / Diffuser.add_noise / the loop's dropout / model(...) / F.mse_loss /
                       masked_geom_mse / loss.backward() / opt.step()      (train_latent_cond.py:136-163)
    native objective   Diffuser.training_loss(...).loss.backward() / opt.step()

Each turn runs `--steps` iterations back to back, timed with device events from the first iteration's
start to the last one's end (the host's share included where the device waits for it); the host's wall
clock per iteration is printed beside it.  Per loop: the median over the turns, their min and max
(the turn-to-turn spread).  The native leg is skipped where Diffuser.training_loss does not exist, so
the same file run on an older checkout gives that checkout's torch-op loop.

    python tools/objective_bench.py [--steps 20] [--turns 9] [--once LEG] [--json FILE] [--prediction v]

--prediction v adds a third loop that takes its turns with the other two: the native objective of a
v-model (Diffuser(prediction="v")), whose noising launch stores one more latent-sized tensor, the target.

--once LEG runs one warmed-up iteration of one leg ("torch" or "native") between two synchronisations
and nothing else: the region to look at in a kernel trace of its own run.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "diffusion-model_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_legs(dev, B=32, hw=28, lam=0.5, p_drop=0.1, prediction="eps"):
    import diff
    import dmx.optim as O
    from dmx import synth
    from losses.geom_losses import masked_geom_mse
    from models.unet_cond_geom import UnetCondWithGeomHead
    model = UnetCondWithGeomHead()
    model.load_state_dict(synth.unet_cond_geom_weights(0))
    model.to(dev).train()
    d = diff.Diffuser(1000, device=dev)
    g = torch.Generator().manual_seed(7)
    z = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    vals = torch.rand((B, 12), generator=g).to(dev)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(dev)
    classes = torch.randint(1, 4, (B,), generator=g).to(dev)
    opt = O.Adam(model.parameters(), lr=1e-5)
    T = d.num_timesteps

    def torch_loop():
        t = torch.randint(1, T + 1, (B,), device=dev)
        z_noisy, noise = d.add_noise(z, t)
        drop = torch.rand(B, device=dev) < p_drop
        y_used = torch.where(drop, torch.zeros_like(classes), classes)
        keep = (~drop).float().unsqueeze(1)
        vals_used, mask_used = vals * keep, mask * keep
        eps, geom = model(z_noisy, t, y_used, cond_vals=vals_used, cond_mask=mask_used)
        loss = F.mse_loss(eps, noise) + lam * masked_geom_mse(geom, vals, mask * keep)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    def native(d=d):
        res = d.training_loss(model, z, classes, vals, mask, geom_lambda=lam, cfg_drop_prob=p_drop)
        opt.zero_grad(set_to_none=True)
        res.loss.backward()
        opt.step()

    legs = {"torch": ("torch-op loop", torch_loop)}
    if hasattr(diff.Diffuser, "training_loss"):
        legs["native"] = ("native objective", native)
        if prediction == "v":
            dv = diff.Diffuser(1000, device=dev, prediction="v")
            legs["native_v"] = ("native objective v", lambda: native(dv))
    return legs


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    host = (time.perf_counter() - t0) / steps
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, host * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20, help="iterations per turn")
    ap.add_argument("--turns", type=int, default=9)
    ap.add_argument("--once", default=None, choices=["torch", "native", "native_v"])
    ap.add_argument("--prediction", default="eps", choices=["eps", "v"])
    ap.add_argument("--json", default=None, help="also write the records to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("objective_bench needs the GPU: there is nothing to time on the host")
    dev = torch.device("cuda:0")
    legs = make_legs(dev, prediction="v" if args.once == "native_v" else args.prediction)
    for _, fn in legs.values():  # warm-up: code objects, the tape and backward arenas, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if args.once:
        legs[args.once][1]()
        torch.cuda.synchronize()
        return
    times = {k: ([], []) for k in legs}
    for _ in range(args.turns):
        for k, (_, fn) in legs.items():
            ms, host = timed(fn, args.steps)
            times[k][0].append(ms)
            times[k][1].append(host)
    recs = []
    for k, (name, _) in legs.items():
        ms, host = times[k]
        recs.append(dict(name=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
                         host_ms_median=statistics.median(host), turns=args.turns, steps=args.steps))
        r = recs[-1]
        print(f"{name:<18} {r['ms_median']:.3f} ms / iteration (min {r['ms_min']:.3f}, max {r['ms_max']:.3f} over "
              f"{args.turns} turns of {args.steps}; host {r['host_ms_median']:.3f} ms)", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
