"""Time the optimizer step on the conditional U-Net's real parameter list.

Five variants take turns in one process on one device, each on its own copy of the parameters with
gradients from randn, timed with device events over `--steps` back-to-back steps per turn:

    torch foreach     torch.optim.Adam(foreach=True)
    torch fused       torch.optim.Adam(fused=True)
    dmx plain         dmx.optim.Adam
    torch clip+ema    clip_grad_norm_ + torch.optim.Adam(fused=True) + torch._foreach_lerp_ EMA
    dmx clip+ema      dmx.optim.Adam(max_grad_norm=1, ema_decay=0.9999)

For each variant: the median over the turns, their min and max, and the bytes/s reached against the
traffic the step cannot avoid (28 B per element: read p, g, m, v and write p, m, v; +8 B for the EMA,
+4 B for the norm pass) and against the HBM rate (6.3 TB/s achievable, MI355X).  A turn's time is
what the device needed from the first step's start to the last step's end, the host's preparation
included where the device waits for it; the host-only time of a step (wall clock of the enqueue
loop) is printed beside it so the two can be told apart.

Then the whole training iteration (U-Net forward, loss, backward, optimizer step) at the bench.py
training leg's shape, B = 32 latents of 28 x 28, with torch's Adam and with the native one, turn by turn.

    python tools/optim_bench.py [--steps 50] [--turns 7] [--iter-steps 10] [--no-iter]
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

HBM = 6.3e12  # achievable bytes/s


def param_copies(dev):
    from dmx import synth
    sd = synth.unet_cond_geom_weights(0)
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(sd)
    return [torch.nn.Parameter(p.detach().to(dev).clone()) for p in m.parameters()]


def make_variants(dev):
    import dmx.optim as O
    out = []

    def add(name, bytes_per_elem, build):
        ps = param_copies(dev)
        g = torch.Generator(device=dev).manual_seed(1)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-2
        out.append(dict(name=name, bpe=bytes_per_elem, step=build(ps), n=sum(p.numel() for p in ps), tensors=len(ps)))

    add("torch foreach", 28, lambda ps: torch.optim.Adam(ps, lr=1e-4, foreach=True).step)
    add("torch fused", 28, lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True).step)
    add("dmx plain", 28, lambda ps: O.Adam(ps, lr=1e-4).step)

    def torch_clip_ema(ps):
        opt = torch.optim.Adam(ps, lr=1e-4, fused=True)
        ema = [p.detach().clone() for p in ps]
        data = [p.data for p in ps]

        def step():
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            opt.step()
            torch._foreach_lerp_(ema, data, 1.0 - 0.9999)
        return step
    add("torch clip+ema", 40, torch_clip_ema)
    add("dmx clip+ema", 40, lambda ps: O.Adam(ps, lr=1e-4, max_grad_norm=1.0, ema_decay=0.9999).step)
    return out


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


def summarize(name, ms, host, extra=None):
    rec = dict(name=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
               host_ms_median=statistics.median(host))
    rec.update(extra or {})
    return rec


def optimizer_runs(dev, steps, turns):
    vs = make_variants(dev)
    for v in vs:  # warm-up: state allocation, code objects, the allocator
        for _ in range(3):
            v["step"]()
    torch.cuda.synchronize()
    times = {v["name"]: ([], []) for v in vs}
    for _ in range(turns):
        for v in vs:
            ms, host = timed(v["step"], steps)
            times[v["name"]][0].append(ms)
            times[v["name"]][1].append(host)
    recs = []
    for v in vs:
        ms, host = times[v["name"]]
        floor_bytes = v["bpe"] * v["n"]
        med = statistics.median(ms)
        recs.append(summarize(v["name"], ms, host, dict(
            elements=v["n"], tensors=v["tensors"], floor_bytes=floor_bytes, floor_ms=floor_bytes / HBM * 1e3,
            bytes_per_s=floor_bytes / (med * 1e-3), hbm_fraction=floor_bytes / (med * 1e-3) / HBM)))
    return recs


def iteration_runs(dev, steps, turns, B=32, hw=28):
    import dmx.optim as O
    from dmx import synth
    from losses.geom_losses import masked_geom_mse
    from models.unet_cond_geom import UnetCondWithGeomHead
    model = UnetCondWithGeomHead()
    model.load_state_dict(synth.unet_cond_geom_weights(0))
    model.to(dev).train()
    g = torch.Generator().manual_seed(7)
    z = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    noise = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    vals = torch.rand((B, 12), generator=g).to(dev)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(dev)
    classes = torch.randint(1, 4, (B,), generator=g).to(dev)
    t = torch.randint(1, 1001, (B,), generator=g).to(dev)
    opts = {"iteration, torch Adam": torch.optim.Adam(model.parameters(), lr=1e-4),
            "iteration, torch fused Adam": torch.optim.Adam(model.parameters(), lr=1e-4, fused=True),
            "iteration, dmx Adam": O.Adam(model.parameters(), lr=1e-4)}

    in_step = {k: [0.0, 0] for k in opts}  # host seconds inside opt.step(), calls

    def make(k, opt):
        def step():
            eps, geom = model(z, t, classes, cond_vals=vals, cond_mask=mask)
            loss = F.mse_loss(eps, noise) + 0.5 * masked_geom_mse(geom, vals, mask)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            t0 = time.perf_counter()
            opt.step()
            in_step[k][0] += time.perf_counter() - t0
            in_step[k][1] += 1
        return step
    fns = {k: make(k, o) for k, o in opts.items()}
    for fn in fns.values():
        for _ in range(2):
            fn()
    times = {k: ([], []) for k in fns}
    for _ in range(turns):
        for k, fn in fns.items():
            ms, host = timed(fn, steps)
            times[k][0].append(ms)
            times[k][1].append(host)
    return [summarize(k, *times[k], dict(batch=B, latent=hw, opt_step_host_ms=in_step[k][0] / in_step[k][1] * 1e3))
            for k in fns]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50, help="optimizer steps per turn")
    ap.add_argument("--turns", type=int, default=7)
    ap.add_argument("--iter-steps", type=int, default=10, help="training iterations per turn")
    ap.add_argument("--no-iter", action="store_true", help="skip the whole-iteration leg")
    ap.add_argument("--json", default=None, help="also write the records to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs the GPU: there is nothing to time on the host")
    dev = torch.device("cuda:0")
    recs = optimizer_runs(dev, args.steps, args.turns)
    for r in recs:
        print(f"{r['name']:<16} {r['ms_median']:.4f} ms (min {r['ms_min']:.4f}, max {r['ms_max']:.4f}; host "
              f"{r['host_ms_median']:.4f} ms/step)  floor {r['floor_ms']:.4f} ms  {r['bytes_per_s'] / 1e12:.3f} TB/s = "
              f"{100 * r['hbm_fraction']:.1f} % of the HBM rate", flush=True)
    if not args.no_iter:
        it = iteration_runs(dev, args.iter_steps, args.turns)
        for r in it:
            print(f"{r['name']:<28} {r['ms_median']:.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f}; host "
                  f"{r['host_ms_median']:.3f} ms/step, of which opt.step() {r['opt_step_host_ms']:.3f} ms)", flush=True)
        recs += it
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
