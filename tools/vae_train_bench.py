"""train_vae.py's step on the drop-in VAE: B = 64 images of 224 x 224, fp32, forward (native
dmx_vae_train_forward + the torch loss), loss.backward() (native dmx_vae_train_backward) and a torch
Adam step — against the same step done by torch autograd over oracle.ref.vae_forward on the same GPU,
in the same process, the two interleaved repeat by repeat (the parent of this feature has no VAE
backward to compare with).

  python tools/vae_train_bench.py [--batch 64] [--size 224] [--warmup 2] [--repeats 5] [--no-baseline]
      one JSON line: images/s and event-timed ms of forward / backward / optimizer for both, the
      native model's dmx_model_workspace_bytes and torch's peak allocation.
  python tools/vae_train_bench.py --native-steps K
      K native steps after the warm-up and nothing else: the run to put under
      `rocprofv3 --kernel-trace --stats` for the per-kernel table (kernel time comes from the
      profiler in a run of its own; the end-to-end figures above are taken with it off).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "diffusion-model_amd"), ROOT]
from dmx import synth  # noqa: E402
from models.vae import VAE  # noqa: E402


def _timed(dev, phases):
    """Run the phases in order with a device event between them -> ms per phase."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
    ev[0].record()
    for i, f in enumerate(phases):
        f()
        ev[i + 1].record()
    torch.cuda.synchronize(dev)
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(phases))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--native-steps", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_train_bench: needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    x = torch.rand((B, 3, S, S), generator=torch.Generator().manual_seed(7)).to(dev)
    sd = synth.vae_weights(0)

    vae = VAE()
    vae.load_state_dict(sd)
    vae.to(dev).train()
    opt = torch.optim.Adam(vae.parameters(), lr=1e-4)
    st = {}

    def n_fwd():
        st["loss"] = vae(x)[2]

    def n_bwd():
        opt.zero_grad(set_to_none=True)
        st["loss"].backward()

    native = [n_fwd, n_bwd, opt.step]

    if args.native_steps > 0:
        for _ in range(args.warmup + args.native_steps):
            for f in native:
                f()
        torch.cuda.synchronize(dev)
        print(json.dumps({"native_steps": args.native_steps, "loss": float(st["loss"])}))
        return

    phases = {"native": native}
    if not args.no_baseline:
        from oracle import ref
        params = {k: v.to(dev).clone().requires_grad_(True) for k, v in sd.items()}
        bopt = torch.optim.Adam(params.values(), lr=1e-4)
        bs = {}
        hl = S // 8

        def b_fwd():
            eps = torch.randn((B, 4, hl, hl), device=dev)
            bs["loss"] = ref.vae_forward(params, x, eps)[2]

        def b_bwd():
            bopt.zero_grad(set_to_none=True)
            bs["loss"].backward()

        phases["torch_autograd"] = [b_fwd, b_bwd, bopt.step]

    for _ in range(args.warmup):
        for fs in phases.values():
            _timed(dev, fs)
    torch.cuda.reset_peak_memory_stats(dev)
    ms = {k: [] for k in phases}
    for _ in range(args.repeats):  # interleaved: one step of each per repeat
        for k, fs in phases.items():
            ms[k].append(_timed(dev, fs))
    out = {"batch": B, "size": S, "repeats": args.repeats, "dtype": "fp32 semantics",
           "workspace_bytes": vae.native().workspace_bytes(),
           "torch_peak_allocated_bytes": int(torch.cuda.max_memory_allocated(dev))}
    for k, rows in ms.items():
        tot = sorted(sum(r) for r in rows)
        med = tot[len(tot) // 2]
        mean = [sum(r[i] for r in rows) / len(rows) for i in range(3)]
        out[k] = {"images_per_s": round(B / (med * 1e-3), 2), "step_ms_median": round(med, 3),
                  "step_ms_min": round(tot[0], 3), "step_ms_max": round(tot[-1], 3),
                  "forward_ms": round(mean[0], 3), "backward_ms": round(mean[1], 3), "optimizer_ms": round(mean[2], 3)}
    assert torch.isfinite(st["loss"]), "non-finite training loss"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
