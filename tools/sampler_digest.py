"""SHA-256 digests of what the Python samplers return, one line per configuration, through public entry
points only — so the same file run in two checkouts shows whether a change to the host-side sampling code
(diff.py, dmx/distributed.py) moved a single bit.

  python tools/sampler_digest.py [--out digests.txt]     one "<name> <sha256 | raises ExceptionType>" per line
  python tools/sampler_digest.py --time N                 instead: N timed Diffuser.sample_latent_cond calls
                                                          per noise source at bench.py's shape, one JSON line

Grid (Diffuser(40), GUARD_CHUNK = 4, B = 3, latents 4 x 8 x 8, synthetic weights):
  sampler    ddpm, ddim eta 0, ddim eta 0.5, dpmpp_2m (6 steps)
  noise      host, device
  variant    CFG g = 3, g = 0, interval, interval + rescale 0.5, composed (base "dropped" + one `also`),
             init_latent + mask + strength 0.5
  model      the dmx network, and the same network behind a wrapper without .native() (a foreign model)
  precision  x3, fp32
and one digest each for denoise_cond, ddim_step, dpm_step (both models and precisions, host noise) and
ShardedCondSampler.sample at world size 1 (every sampler, both noise sources).

There is no fallback: without a GPU this fails."""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "diffusion-model_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

COUNTS, B, Z, T, G = {1: 2, 3: 1}, 3, (4, 8, 8), 40, 3.0
SAMPLERS = {"ddpm": {}, "ddim_eta0": dict(sampler="ddim", steps=6, eta=0.0),
            "ddim_eta0.5": dict(sampler="ddim", steps=6, eta=0.5), "dpmpp_2m": dict(sampler="dpmpp_2m", steps=6)}


def sha(t):
    return hashlib.sha256(t.detach().to(torch.float32).cpu().contiguous().numpy().tobytes()).hexdigest()


def variants():
    g = torch.Generator().manual_seed(2)
    z0 = torch.randn((B,) + Z, generator=g)
    mask = (torch.rand(Z[1:], generator=g) > 0.5).float()
    also = [dict(classes=2, weight=1.5)]
    return {"cfg3": dict(guidance_scale=G), "g0": dict(guidance_scale=0.0),
            "interval": dict(guidance_scale=G, guidance_interval=(8, 30)),
            "interval_rescale": dict(guidance_scale=G, guidance_interval=(8, 30), guidance_rescale=0.5),
            "composed": dict(guidance_scale=G, base="dropped", also=also),
            "known": dict(guidance_scale=G, init_latent=z0, mask=mask, strength=0.5)}


def attempt(fn):
    try:
        return sha(fn())
    except (UnboundLocalError, TypeError, ValueError) as e:  # (a rejected configuration is behaviour too)
        return f"raises {type(e).__name__}"


def digests(emit):
    import diff
    from dmx import synth
    from dmx.distributed import ShardedCondSampler
    from models.unet_cond_geom import UnetCondWithGeomHead
    from oracle.rules import Foreign  # the network as a duck-typed model: every step takes the foreign branch
    dev = torch.device("cuda", 0)
    model = UnetCondWithGeomHead()
    model.load_state_dict(synth.unet_cond_geom_weights(0))
    model.to(dev).eval()
    models = {"native": model, "foreign": Foreign(model)}
    gen = torch.Generator().manual_seed(4)
    cond = torch.rand((B, 12), generator=gen)
    var = variants()

    def diffuser(noise):
        d = diff.Diffuser(T, device=dev)
        d.GUARD_CHUNK = 4
        d.noise_source = noise
        return d

    for prec in ("x3", "fp32"):
        model.native().set_precision(prec)
        for mname, m in models.items():
            for sname, skw in SAMPLERS.items():
                for noise in ("host", "device"):
                    for vname, vkw in var.items():
                        d = diffuser(noise)
                        torch.manual_seed(21)
                        emit(f"sample_latent_cond/{prec}/{mname}/{sname}/{noise}/{vname}",
                             attempt(lambda: d.sample_latent_cond(m, COUNTS, z_shape=Z, vae=None, progress=False,
                                                                  cond=cond, **skw, **vkw)))
            # the public one-step entries, host noise
            d = diffuser("host")
            x = torch.randn((B,) + Z, generator=gen).to(dev)
            y = torch.tensor([1, 1, 3], device=dev)
            vals, msk = cond.to(dev), torch.ones((B, 12), device=dev)
            pos = torch.full((B,), 3, dtype=torch.long, device=dev)
            for g in (G, 0.0):
                kw = dict(y=y, guidance_scale=g, cond_vals=vals, cond_mask=msk)
                torch.manual_seed(22)
                emit(f"denoise_cond/{prec}/{mname}/g{g}",
                     attempt(lambda: d.denoise_cond(m, x, torch.full((B,), 17, device=dev), **kw)))
                torch.manual_seed(22)
                emit(f"ddim_step/{prec}/{mname}/g{g}", attempt(lambda: d.ddim_step(m, x, pos, 6, 0.5, **kw)))
                hist = torch.full_like(x, 0.25)
                emit(f"dpm_step/{prec}/{mname}/g{g}", attempt(lambda: d.dpm_step(m, x, pos, hist, 6, **kw)))
                emit(f"dpm_step.hist/{prec}/{mname}/g{g}", sha(hist))
        for sname, skw in SAMPLERS.items():
            for noise in ("host", "device"):
                for vname in ("cfg3", "interval_rescale", "composed", "known"):
                    d = diffuser(noise)
                    torch.manual_seed(21)
                    emit(f"sharded_ws1/{prec}/{sname}/{noise}/{vname}",
                         attempt(lambda: ShardedCondSampler(d, model, None).sample(COUNTS, z_shape=Z, decode=False,
                                                                                   cond=cond, **skw, **var[vname])))
    model.native().set_precision("x3")


def timing(n):
    """bench.py's shape: B = 64, 4 x 28 x 28, Diffuser(200), g = 3, no decode; per noise source one untimed
    call (workspace, graph capture), then n timed ones."""
    import diff
    from dmx import synth
    from models.unet_cond_geom import UnetCondWithGeomHead
    dev = torch.device("cuda", 0)
    model = UnetCondWithGeomHead()
    model.load_state_dict(synth.unet_cond_geom_weights(0))
    model.to(dev).eval()
    counts = [(1, 22), (2, 21), (3, 21)]
    out = {}
    for noise in ("device", "host"):
        d = diff.Diffuser(200, device=dev)
        d.noise_source = noise
        secs = []
        for k in range(n + 1):
            torch.manual_seed(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = d.sample_latent_cond(model, counts, z_shape=(4, 28, 28), vae=None, progress=False, guidance_scale=G)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        assert bool(torch.isfinite(x).all()) and d.range_fallbacks == 0
        out[noise] = {"first_call_s": round(secs[0], 4), "timed_s": [round(v, 4) for v in secs[1:]],
                      "sha256": sha(x)[:16]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the digest lines to this file")
    ap.add_argument("--time", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_digest needs an MI355X: no GPU visible, and there is no fallback")
    torch.cuda.set_device(0)
    if args.time:
        return timing(args.time)
    lines = []

    def emit(name, value):
        lines.append(f"{name} {value}")
        print(lines[-1], flush=True)

    digests(emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
