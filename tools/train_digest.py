"""SHA-256 digests of what the training entry points return, one line per result, through public Python
entry points only — so the same file run against two builds of the library (DMX_LIB, dmx/_lib.py) shows
whether a change to the training host code (train_engine.h, vae_train_engine.h, the arena driver) moved
a single bit of a forward, a gradient or a geometry-guided step.

  python tools/train_digest.py [--out digests.txt]        one "<name> <sha256>" per line

Synthetic weights (dmx.synth, seed 0), seeded inputs:
  unet    train_forward + train_backward: eps, geom and every gradient tensor — UnetCondWithGeomHead with
          vals / mask, without them, and with d_geom = None; UnetCond with remove_deep_conv — at B = 3 8x8,
          B = 2 16x16, B = 2 28x28 and B = 32 28x28 (bench.py's training shape: its split counts and
          two-pass column sums); input_grad (the data-only backward) at B = 2 16x16 and 28x28
  guided  one eager geometry-guided step and a 9-step graph loop (the 8-step graph and the 1-step graph
          both replay) for DDPM, DDIM and DPM-Solver++(2M) at B = 2 16x16
  vae     vae_train_forward + vae_train_backward: x_recon, z, kl and every gradient tensor, with all three
          cotangents and with each one alone, at 2x3x32x32 and 1x3x64x32
  attn    one dmx_attn_core_backward call at n = 2, L = 64, C = 64
and workspace_bytes() of each model after its cases, as a line of its own.

There is no fallback: without a GPU this fails."""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "diffusion-model_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

UNET_SHAPES = [(3, 8), (2, 16), (2, 28), (32, 28)]
INPUT_GRAD_SHAPES = [(2, 16), (2, 28)]
VAE_SHAPES = [(2, 32, 32), (1, 64, 32)]
G = 3.0


def sha(t):
    return hashlib.sha256(t.detach().to(torch.float32).cpu().contiguous().numpy().tobytes()).hexdigest()


def unet_inputs(B, hw, dev):
    g = torch.Generator().manual_seed(1000 * B + hw)
    x = torch.randn((B, 4, hw, hw), generator=g)
    t = torch.randint(1, 1001, (B,), generator=g)
    y = torch.randint(0, 4, (B,), generator=g)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    d_eps = torch.randn((B, 4, hw, hw), generator=g) * 1e-3  # gradient-sized
    d_geom = torch.randn((B, 12), generator=g) * 1e-2
    return [v.to(dev) for v in (x, t, y, vals, mask, d_eps, d_geom)]


def unet_digests(emit, dev):
    from dmx import synth
    from models.unet_cond import UnetCond
    from models.unet_cond_geom import UnetCondWithGeomHead
    geom = UnetCondWithGeomHead()
    geom.load_state_dict(synth.unet_cond_geom_weights(0))
    geom.to(dev).eval()
    sd = synth.unet_cond_geom_weights(0, remove_deep_conv=True)
    shallow = UnetCond(cfg_drop_prob=0.0, remove_deep_conv=True)
    shallow.load_state_dict({k: v for k, v in sd.items() if not k.startswith("geom_head.")})
    shallow.to(dev).eval()

    def step(tag, nm, x, t, y, vals, mask, d_eps, d_geom):
        eps, gp, tape = nm.train_forward(x, t, y, vals, mask)
        emit(f"{tag}/eps", sha(eps))
        if gp is not None:
            emit(f"{tag}/geom", sha(gp))
        grads = nm.train_backward(tape, d_eps, d_geom)
        for name, _ in nm.keys:
            emit(f"{tag}/grad/{name}", sha(grads[name]))
        return tape

    nm = geom.native()
    for B, hw in UNET_SHAPES:
        x, t, y, vals, mask, d_eps, d_geom = unet_inputs(B, hw, dev)
        tag = f"unet/geom/B{B}_{hw}x{hw}"
        tape = step(f"{tag}/cond", nm, x, t, y, vals, mask, d_eps, d_geom)
        if (B, hw) in INPUT_GRAD_SHAPES:
            emit(f"{tag}/cond/input_grad/both", sha(nm.input_grad(tape, d_eps, d_geom)))
            emit(f"{tag}/cond/input_grad/d_geom", sha(nm.input_grad(tape, None, d_geom)))
        step(f"{tag}/nocond", nm, x, t, y, None, None, d_eps, d_geom)
        step(f"{tag}/no_d_geom", nm, x, t, y, vals, mask, d_eps, None)
    guided_digests(emit, dev, geom)
    emit("unet/geom/workspace_bytes", nm.workspace_bytes())
    nm = shallow.native()
    for B, hw in UNET_SHAPES:
        x, t, y, vals, mask, d_eps, d_geom = unet_inputs(B, hw, dev)
        step(f"unet/shallow/B{B}_{hw}x{hw}", nm, x, t, y, None, None, d_eps, None)
    emit("unet/shallow/workspace_bytes", nm.workspace_bytes())


def guided_digests(emit, dev, model):
    import diff
    nm = model.native()
    B, hw, S, steps = 2, 16, 12, 9
    x0, _, y, vals, mask, _, _ = unet_inputs(B, hw, dev)
    y = y.clamp_min(1)
    scale = torch.tensor([1000.0, 1500.0], device=dev)
    d = diff.Diffuser(1000, device=dev)
    for kind in ("ddpm", "ddim", "dpm"):
        if kind == "ddpm":
            tables, sched, sig = d.coef_tables(dev, True), None, d.geom_sig(dev)
        else:
            sched = d.ddim_tables(S, 0.5, dev) if kind == "ddim" else d.dpm_tables(S, "uniform", dev)
            tables, sig = None, sched[1]
        kw = dict(sched=sched) if sched is not None else {}
        out, hist = torch.empty_like(x0), torch.full_like(x0, 0.25)
        hk = dict(hist=hist) if kind == "dpm" else {}
        nm.step(x0, out, torch.full((B,), 5, dtype=torch.long, device=dev), y, 0, vals, mask, G, tables, None, seed=7,
                geom=(scale, sig), **kw, **hk)
        emit(f"guided/{kind}/step", sha(out))
        if kind == "dpm":
            emit(f"guided/{kind}/step.hist", sha(hist))
        x, hist = x0.clone(), torch.full_like(x0, float("nan"))
        hk = dict(hist=hist) if kind == "dpm" else {}
        t = torch.full((1,), S, dtype=torch.long, device=dev)
        nm.sample_loop(x, t, y, 0, vals, mask, G, tables, steps, seed=7, use_graph=True, geom=(scale, sig), **kw, **hk)
        torch.cuda.synchronize(dev)
        emit(f"guided/{kind}/loop{steps}", sha(x))
        if kind == "dpm":
            emit(f"guided/{kind}/loop{steps}.hist", sha(hist))


def vae_digests(emit, dev):
    from dmx import synth
    from models.vae import VAE
    v = VAE()
    v.load_state_dict(synth.vae_weights(0))
    v.to(dev).eval()
    nm = v.native()
    for n, h, w in VAE_SHAPES:
        g = torch.Generator().manual_seed(100 * h + w)
        x = torch.rand((n, 3, h, w), generator=g).to(dev)
        eps = torch.randn((n, 4, h // 8, w // 8), generator=g).to(dev)
        cot = dict(d_recon=(torch.randn((n, 3, h, w), generator=g) * 1e-3).to(dev),
                   d_z=(torch.randn((n, 4, h // 8, w // 8), generator=g) * 1e-2).to(dev),
                   d_kl=(torch.rand((n,), generator=g) * 1e-2).to(dev))
        tag = f"vae/{n}x3x{h}x{w}"
        x_recon, z, kl, tape = nm.vae_train_forward(x, eps)
        for name, out in (("x_recon", x_recon), ("z", z), ("kl", kl)):
            emit(f"{tag}/{name}", sha(out))
        for which in ("all", "d_recon", "d_z", "d_kl"):
            grads = nm.vae_train_backward(tape, **(cot if which == "all" else {which: cot[which]}))
            for name, _ in nm.keys:
                emit(f"{tag}/{which}/grad/{name}", sha(grads[name]))
    emit("vae/workspace_bytes", nm.workspace_bytes())


def attn_digest(emit, dev):
    from dmx import _lib
    lib = _lib.load()
    n, L, C = 2, 64, 64
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn((n, L, 3 * C), generator=g) * 1.5
    dout = (torch.randn((n, L, C), generator=g) * 1e-3).to(dev)
    q, k, v = (t.reshape(n, L, 4, C // 4).transpose(1, 2) for t in qkv.split(C, dim=2))
    o = (torch.softmax(q @ k.transpose(-1, -2) / (C // 4) ** 0.5, dim=-1) @ v).transpose(1, 2).reshape(n, L, C)
    qkv, o = qkv.to(dev), o.contiguous().to(dev)  # (the forward on the host: its bits are an input, hashed below)
    dqkv = torch.full_like(qkv, float("nan"))
    with torch.cuda.device(dev):
        _lib.check(lib.dmx_attn_core_backward(*(ctypes.c_void_p(t.data_ptr()) for t in (qkv, o, dout, dqkv)), n, L, C,
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    emit("attn/o_input", sha(o))
    emit(f"attn/dqkv/n{n}_L{L}_C{C}", sha(dqkv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the digest lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_digest needs an MI355X: no GPU visible, and there is no fallback")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def emit(name, value):
        lines.append(f"{name} {value}")
        print(lines[-1], flush=True)

    unet_digests(emit, dev)
    vae_digests(emit, dev)
    attn_digest(emit, dev)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
