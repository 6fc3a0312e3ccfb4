"""Which kernels each plan class of tests/test_gpu_vae_train_classes.py reaches.

Run (a kernel trace of its own, no counters, the program after `--`):

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o vae_classes -- \
      python tools/vae_train_class_trace.py

runs one taped forward and one three-cotangent backward of the native VAE training step per shape of CLASSES, after
a warm-up step (the one-time weight splits), with a torch.cumsum between the shapes: its scan kernel is the
separator in the trace.

Summarise (CPU only):

  python tools/vae_train_class_trace.py --summarise <dir>/.../vae_classes_kernel_trace.csv \
      profiles/vae_train_class_kernels.txt

writes, per shape, the library's kernels in the order of their first dispatch with their template arguments and
dispatch counts."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "diffusion-model_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(1, 8, 8), (5, 40, 24), (2, 56, 48), (17, 16, 16), (17, 32, 32), (64, 16, 16), (65, 8, 8), (64, 32, 32),
          (1, 128, 128)]
SEPARATOR = re.compile(r"scan|cumsum", re.I)


def run():
    import torch
    from dmx import synth
    from models.vae import VAE
    dev = torch.device("cuda:0")
    v = VAE()
    v.load_state_dict(synth.vae_weights(0))
    model = v.to(dev).train().native()

    def step(n, h, w):
        g = torch.Generator().manual_seed(n)
        x = torch.rand((n, 3, h, w), generator=g).to(dev)
        eps = torch.randn((n, 4, h // 8, w // 8), generator=g).to(dev)
        x_recon, z, kl, tape = model.vae_train_forward(x, eps)
        d_recon = 2.0 * (x_recon - x) / x.numel()
        d_z = 0.3 * 2.0 * z / z.numel()
        d_kl = torch.full((n,), 0.5 / n, device=dev)
        model.vae_train_backward(tape, d_recon, d_z, d_kl)
        torch.cuda.synchronize()

    step(1, 8, 8)
    for s in SHAPES:
        torch.cumsum(torch.ones(64, device=dev), 0)
        torch.cuda.synchronize()
        step(*s)
        print("ran", s, flush=True)


def summarise(src, dst):
    with open(src, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if SEPARATOR.search(name) and "dmx::" not in name:
            cur = {}
            groups.append(cur)
        elif cur is not None and "dmx::" in name:
            name = re.sub(r"\s*\[clone[^\]]*\]|\.kd$", "", name)
            name = re.sub(r"^void\s+", "", name)
            name = re.sub(r"\(.*\)$", "", name)  # the argument list; the template arguments stay
            cur[name] = cur.get(name, 0) + 1
    if len(groups) != len(SHAPES):
        raise SystemExit(f"{len(groups)} separators in the trace, {len(SHAPES)} shapes")
    with open(dst, "w") as f:
        f.write("# Kernels of one native VAE training step (taped forward + three-cotangent backward) per plan class of\n"
                "# tests/test_gpu_vae_train_classes.py, in the order of their first dispatch: name<template arguments> x\n"
                "# dispatches.  One rocprofv3 --kernel-trace run of tools/vae_train_class_trace.py on an MI355X.\n")
        for s, g in zip(SHAPES, groups):
            f.write(f"\n[{s[0]}, {s[1]}, {s[2]}]\n")
            for name, cnt in g.items():
                f.write(f"{name} x {cnt}\n")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3])
    else:
        run()
