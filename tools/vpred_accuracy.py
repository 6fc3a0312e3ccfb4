"""How much accuracy a v-model's update loses by going through eps.  CPU only, float64.

A v-model's step converts its output to eps = sqrt(ab) v + sqrt(1-ab) x in fp32 and runs the eps-form
update, whose x0 = (x - sqrt(1-ab) eps) / sqrt(ab) cancels near t = T (sqrt(ab_T) = 0.0064 on the default
schedule).  The direct form x0 = sqrt(ab) x - sqrt(1-ab) v does not.  For every timestep t of the schedule
and the steps t -> max(t - stride, 0) of a few strides (1: the full schedule; 20: S = 50; t: straight to
x0) — DDIM with eta = 0 and the first-order DPM-Solver++ row, whose second-order term k_p hist does not
touch the cancellation — this prints the relative L2 error against the direct form evaluated in float64
with the schedule's float64 coefficients, of
    v via eps     the shipped rule: conversion, then the eps-form update, fp32 ops on the fp32 tables
    v direct x0   x0 and eps from v directly, then x' = k_s x0 + k_d eps (DPM: k_x x + k_c x0), likewise fp32
    eps-mode      for scale, today's rule: the fp32 eps-form update on an eps of the same distribution,
                  against that update in float64 with float64 coefficients
on x, v ~ N(0, 1), n samples of 4x16x16 per timestep.  At stride 1 the DDPM posterior mean is listed too:
(x - c1 eps) / c2 against d_s x0 + d_d eps (Diffuser.x0_tables), the x0-form's rule.

--schedule ztsnr: the same on the zero-terminal-SNR schedule (Diffuser(zero_terminal_snr=True)), where
ab_T = 0: the eps-form columns divide by sqrt(ab_T) = 0 at t = T (printed as inf / nan) and lose digits
below it; "v direct x0" is the x0-form the step tails then run.

    python tools/vpred_accuracy.py [--n 8] [--strides 1,20,0] [--schedule default|ztsnr] [--json FILE]
                                                                                  (stride 0: to x0)
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "diffusion-model_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def rel_rows(a, b):
    """per-row relative L2 of a against b (float64)."""
    a, b = a.double().flatten(1), b.double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


def study(n, strides, schedule="default"):
    import diff
    d = diff.Diffuser(1000, prediction="v", zero_terminal_snr=schedule == "ztsnr")
    T = d.num_timesteps
    p_o, p_x = d.pred_tables("cpu")
    ab = torch.cat([torch.ones(1, dtype=torch.float64), d._host[1].double()])  # ab[0] := 1
    g = torch.Generator().manual_seed(0)
    shape = (T, n * 4 * 16 * 16)  # row t - 1: the samples at timestep t
    x, v, e = (torch.randn(shape, generator=g) for _ in range(3))
    t = torch.arange(1, T + 1)
    f32, f64 = torch.float32, torch.float64
    out = {}
    for stride in strides:  # the step t -> s = max(t - stride, 0); stride 0: straight to s = 0 (x' = x0)
        s_idx = torch.zeros_like(t) if stride == 0 else torch.clamp(t - stride, min=0)
        ab_t, ab_s = ab[t], ab[s_idx]
        # the rows of ddim_tables (eta = 0) / dpm_tables (first order) for these pairs: float64, rounded once
        k_e, k_a = torch.sqrt(1 - ab_t).float(), torch.sqrt(ab_t).float()
        k_s, k_d = torch.sqrt(ab_s).float(), torch.sqrt(1 - ab_s).float()
        k_x = (torch.sqrt(1 - ab_s) / torch.sqrt(1 - ab_t))
        k_c = (torch.sqrt(ab_s) - k_x * torch.sqrt(ab_t)).float()
        k_x = k_x.float()
        c64 = dict(e=torch.sqrt(1 - ab_t), a=torch.sqrt(ab_t), s=torch.sqrt(ab_s), d=torch.sqrt(1 - ab_s))
        c64["x"] = c64["d"] / c64["e"]
        c64["c"] = c64["s"] - c64["x"] * c64["a"]
        c32 = dict(e=k_e, a=k_a, s=k_s, d=k_d, x=k_x, c=k_c)
        for rule in ("ddim", "dpm"):
            def update(k, x, eps, x0):
                if rule == "ddim":
                    return k["s"].view(-1, 1) * x0 + k["d"].view(-1, 1) * eps
                return k["x"].view(-1, 1) * x + k["c"].view(-1, 1) * x0

            def via_eps(k, x, eps):
                return update(k, x, eps, (x - k["e"].view(-1, 1) * eps) / k["a"].view(-1, 1))

            # the truth: the direct form in float64 with the schedule's own float64 coefficients
            xd, vd = x.double(), v.double()
            x0_64 = c64["a"].view(-1, 1) * xd - c64["e"].view(-1, 1) * vd
            eps64 = c64["a"].view(-1, 1) * vd + c64["e"].view(-1, 1) * xd
            truth = update(c64, xd, eps64, x0_64)
            # fp32, with the fp32 tables the kernels read
            eps32 = p_o.view(-1, 1) * v + p_x.view(-1, 1) * x
            x0_32 = p_o.view(-1, 1) * x - p_x.view(-1, 1) * v
            res = {"v_via_eps": rel_rows(via_eps(c32, x, eps32), truth),
                   "v_direct_x0": rel_rows(update(c32, x, eps32, x0_32), truth),
                   "eps_mode": rel_rows(via_eps(c32, x, e), via_eps(c64, xd, e.double()))}
            out[f"{rule} stride {stride if stride else 't (to x0)'}"] = {k: r.tolist() for k, r in res.items()}
        if stride == 1:  # the DDPM posterior mean: the eps-form's (x - c1 eps) / c2 against d_s x0 + d_d eps
            col = lambda k: k.view(-1, 1)  # noqa: E731
            a64, ab64, abp = d._host[0].double(), ab[1:], ab[:-1]
            c1, c2, _ = d.coef_tables("cpu")
            d_s, d_d = d.x0_tables("cpu")
            d64 = (torch.sqrt(abp), (1 - abp) * torch.sqrt(a64) / torch.sqrt(1 - ab64))
            e64 = ((1 - a64) / torch.sqrt(1 - ab64), torch.sqrt(a64))
            xd, vd = x.double(), v.double()
            x0_64 = col(c64["a"]) * xd - col(c64["e"]) * vd
            eps64 = col(c64["a"]) * vd + col(c64["e"]) * xd
            truth = col(d64[0]) * x0_64 + col(d64[1]) * eps64
            eps32 = col(p_o) * v + col(p_x) * x
            x0_32 = col(p_o) * x - col(p_x) * v
            res = {"v_via_eps": rel_rows((x - col(c1) * eps32) / col(c2), truth),
                   "v_direct_x0": rel_rows(col(d_s) * x0_32 + col(d_d) * eps32, truth),
                   "eps_mode": rel_rows((x - col(c1) * e) / col(c2), (xd - col(e64[0]) * e.double()) / col(e64[1]))}
            out["ddpm mean stride 1"] = {k: r.tolist() for k, r in res.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=8, help="samples of 4x16x16 per timestep")
    ap.add_argument("--strides", default="1,20,0", help="comma-separated; 0 stands for t (the step to x0)")
    ap.add_argument("--schedule", default="default", choices=["default", "ztsnr"],
                    help="ztsnr: the zero-terminal-SNR schedule (ab_T = 0)")
    ap.add_argument("--json", default=None, help="also write every timestep's figures to this file")
    args = ap.parse_args()
    res = study(args.n, [int(v) for v in args.strides.split(",")], args.schedule)
    rows = [1, 2, 10, 20, 100, 250, 500, 750, 900, 950, 980, 990, 999, 1000]
    print(f"schedule: {args.schedule}")
    for rule, cols in res.items():
        print(f"{rule}: rel-L2 of the fp32 update against float64, at t =")
        print("      t  " + "".join(f"{k:>14}" for k in cols))
        for t in rows:
            print(f"  {t:5d}  " + "".join(f"{cols[k][t - 1]:14.3e}" for k in cols))
        for k in cols:
            finite = [i for i in range(len(cols[k])) if cols[k][i] == cols[k][i] and cols[k][i] != float("inf")]
            worst = max(finite, key=lambda i: cols[k][i])
            bad = len(cols[k]) - len(finite)
            print(f"  worst {k}: {cols[k][worst]:.3e} at t = {worst + 1}" + (f"; non-finite at {bad} timestep(s)" if bad else ""))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
