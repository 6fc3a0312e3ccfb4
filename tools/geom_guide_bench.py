"""Geometry guidance: what a guided step costs, and which seed shows that it guides.

GPU (default):  python tools/geom_guide_bench.py [--batch 64 --hw 32 --steps 16 --reps 7]
  * the geometry-guided device loop against the plain CFG loop, per step, the two interleaved in
    one process (guided, plain, guided, ...) so that they share the machine: median and min..max;
  * within the same run, three lone timings at the same shape: the taped forward
    (dmx_train_forward), the data-only backward (dmx_train_backward_input) and the full parameter
    backward (dmx_train_backward);
  * the expected step (plain step + taped forward + data-only backward) and the gap to it.
  Times are host clocks around work that ends in a device synchronise; every shape is warmed up.
  One JSON line goes to stdout.  Without a GPU this mode fails.

CPU:  python tools/geom_guide_bench.py --oracle-seeds N
  The oracle restatement of tests/test_gpu_geom.py::test_it_guides (host-noise DDIM, S = 8, CFG 3,
  B = 4 at 8x8, synthetic weights seed 0) for seeds 0..N-1 with geom_scale 0 and 1000: the final
  latent's masked loss by the oracle at t = 1, averaged over the rows, and the drop."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "diffusion-model_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def oracle_seeds(n_seeds: int, scale: float) -> None:
    import diff
    from dmx import synth
    from oracle import train_ref
    from oracle.rules import ddim_update
    from test_gpu_geom import G, final_loss, guide_inputs, mix_ref, oracle_grad
    sd = synth.unet_cond_geom_weights(0)
    d = diff.Diffuser(1000, device="cpu")
    sched = d.ddim_tables(8, 0.0, "cpu")
    y = torch.tensor([1, 2, 3, 1])
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for seed in range(n_seeds):
        vals, mask = guide_inputs(seed)
        losses = []
        for s in (0.0, scale):
            torch.manual_seed(seed)
            x = torch.randn((4, 4, 8, 8))
            for p in range(8, 0, -1):
                pos = torch.full((4,), p, dtype=torch.long)
                t = sched[0][pos - 1]
                _, grad, _, ec = oracle_grad(sd, x, t, y, vals, mask)
                with torch.no_grad():
                    eu = train_ref.forward(sd, x, t, torch.zeros_like(y), vals, mask)[0]
                    eps = mix_ref(eu + G * (ec - eu), grad, torch.full((4,), s), sched[1], pos)
                    x = ddim_update(x, eps, pos, sched, torch.zeros_like(x))
            losses.append(final_loss(sd, x, y, vals, mask))
        print(f"seed {seed}: masked loss {losses[0]:.5f} -> {losses[1]:.5f} "
              f"({100 * (1 - losses[1] / losses[0]):.1f} % lower)", flush=True)


def timed(fn, dev, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms, per=1):
    v = [m / per for m in ms]
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def gpu_bench(B: int, hw: int, steps: int, reps: int, scale: float) -> None:
    if not torch.cuda.is_available():
        raise SystemExit("geom_guide_bench: no GPU (the timings are GPU timings; there is no fallback)")
    import diff
    from dmx import synth
    from models.unet_cond_geom import UnetCondWithGeomHead
    dev = torch.device("cuda:0")
    m = UnetCondWithGeomHead()
    m.load_state_dict(synth.unet_cond_geom_weights(0))
    m.to(dev).eval()
    nm = m.native()
    d = diff.Diffuser(1000, device=dev)
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    y = torch.randint(1, 4, (B,), generator=g).to(dev)
    vals = torch.rand((B, 12), generator=g).to(dev)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(dev)
    sched = d.ddim_tables(50, 0.0, dev)
    gs = torch.full((B,), scale, device=dev)
    x, t = torch.empty_like(x0), torch.zeros((1,), dtype=torch.long, device=dev)

    def loop(guided):
        x.copy_(x0)
        t.fill_(50)
        nm.sample_loop(x, t, y, 0, vals, mask, 3.0, None, steps, seed=1, sched=sched,
                       **(dict(geom=(gs, sched[1])) if guided else {}))

    for guided in (True, False, True, False):  # (the larger plan first; both graphs captured and replayed once)
        loop(guided)
    torch.cuda.synchronize(dev)
    t_g, t_p = [], []
    for _ in range(reps):
        t_g += timed(lambda: loop(True), dev, 1)
        t_p += timed(lambda: loop(False), dev, 1)
    # lone legs at the same shape
    tt = torch.full((B,), 500, dtype=torch.long, device=dev)
    d_eps = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    d_geom = torch.randn((B, 12), generator=g).to(dev)
    state = {}

    def fwd():
        state["tape"] = nm.train_forward(x0, tt, y, vals, mask)[2]

    for _ in range(2):
        fwd()
        nm.input_grad(state["tape"], None, d_geom)
        nm.train_backward(state["tape"], d_eps, d_geom)
    t_f, t_bi, t_bp = [], [], []
    for _ in range(reps):
        t_f += timed(fwd, dev, 1)
        t_bi += timed(lambda: nm.input_grad(state["tape"], None, d_geom), dev, 1)
        t_bp += timed(lambda: nm.train_backward(state["tape"], d_eps, d_geom), dev, 1)
    res = dict(batch=B, hw=hw, steps=steps, reps=reps, scale=scale,
               guided_step=summary(t_g, steps), plain_step=summary(t_p, steps), taped_forward=summary(t_f),
               backward_input=summary(t_bi), backward_params=summary(t_bp))
    expect = (res["plain_step"]["median_ms"] + res["taped_forward"]["median_ms"]
              + res["backward_input"]["median_ms"])
    res["expected_guided_step_ms"] = round(expect, 4)
    res["gap_ms"] = round(res["guided_step"]["median_ms"] - expect, 4)
    res["ratio_guided_to_plain"] = round(res["guided_step"]["median_ms"] / res["plain_step"]["median_ms"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hw", type=int, default=32)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1000.0)
    ap.add_argument("--oracle-seeds", type=int, default=0)
    a = ap.parse_args()
    if a.oracle_seeds > 0:
        oracle_seeds(a.oracle_seeds, a.scale)
    else:
        gpu_bench(a.batch, a.hw, a.steps, a.reps, a.scale)
