"""Few-step sampling (strided DDIM, DPM-Solver++(2M)) against the full DDPM walk on one MI355X: prints
one JSON line.

  python tools/sampler_bench.py [--rounds 5] [--prediction eps|v|v_x0]
      [--groups loops,known_loops,guidance_loops,composed_loops,pag_loops,end_to_end,cache]

--prediction v runs every group with the model read as a v-predictor (Diffuser(prediction="v")): the same
launches, each tail converting its mixed output to eps before the update.  Run it beside the default on
one build for the cost of the conversion.  --prediction v_x0 reads it as a v-predictor in x0-form
(Diffuser(prediction="v", x0_form=True), the form a zero-terminal-SNR schedule needs; the schedule itself stays
the default one, so that the legs are those of --prediction v): beside v, the cost of the x0-form tails.

Workload: bench.py's — B = 64, 32x32x4 latents, CFG 3.0, device (Philox) noise, synthetic weights.

1. ms per step of the graph loops.  The strided loop (S = 50 of T = 1000, eta = 1 so that it draws
   noise as the DDPM step does), the DPM-Solver++(2M) loop (S = 50, log-SNR spacing; it draws nothing and
   reads and writes its history buffer) and the DDPM loop alternate in one process, the DDPM leg twice per
   round (legs ddpm_a, ddim, dpmpp_2m, ddpm_b), so the spread between two measurements of the SAME loop is
   known and the few-step legs are judged against it, not against a preset figure.  A DDIM-inversion
   leg (S = 50, R = 1: 100 rows; a row is one forward, the inverting tail reads and on the last row of
   a position writes its source latent) runs between dpmpp_2m and ddpm_b: ms per row.  A model
   keeps the graphs of its last four loops: every leg first runs 8 steps untimed (a capture, or a
   replay where its graphs are still held), then 48 steps (six launches of the 8-step graph)
   between two device events.  Reported: the median over the rounds.
   The known-region loop (img2img / inpainting: the same DPM-Solver++(2M) loop with the known-region blend
   launched after every step) is measured likewise against the plain DPM loop, the plain leg twice per
   round (legs dpmpp_2m_a, known, dpmpp_2m_b), and judged against that leg's own spread.
   The guidance controls likewise (legs dpmpp_2m_a, unguided, rescaled, dpmpp_2m_b): the unguided loop
   (guidance 0 with y given: one B-sample forward per step) and the rescaled CFG loop (phi = 0.7: three
   tail launches instead of one), with the unguided / plain ratio.
   Composed guidance likewise (legs dpmpp_2m_a, composed_k1, composed_k2, composed_k4, unbatched_k2,
   dpmpp_2m_b): the composed loop with K = 1 (the plain step's rows), K = 2 and K = 4 branches over the
   base, each as a ratio to the plain step, and what a user would run without the batched step — three
   B-sample forwards, compose_eps and the standalone update per step, eager — with the model's workspace
   after the K = 2 and the K = 4 loops.
   Perturbed-attention guidance likewise (legs dpmpp_2m_a, composed_k2, pag_sa3, pag_all6, dpmpp_2m_b): three
   ordinary branches against the same three with the last one's attention replaced by the identity in sa3
   or in all six blocks, each PAG leg as a ratio to composed_k2 and to the plain step, with the workspace.
2. Wall-clock images/s of Diffuser.sample_latent_cond with the VAE decode to uint8 images, for
   (ddpm, T = 1000), (ddim, S = 50, eta = 0) and (dpmpp_2m, S = 20, log-SNR spacing): the first call (it captures the graphs) and the best of
   the calls after it, separately.  The decode is warmed before either, so the first-call figures differ
   from the steady ones by the sampler's own start-up only.  (dpmpp_2m, S = 20) is also run with a guidance
   interval that covers half of its positions (the middle ten), to be compared with the plain leg of
   the same run: its loop alternates unguided / guided / unguided segments, so it shows whether their
   graphs are reused.  Last, invert_latent_cond(S = 20, strength 0.3, R = 2) followed by
   sample_latent_cond(start_latent=..., ddim) and the decode: the edit round trip, in images/s.
3. Feature caching (group `cache`, not in the default groups): the DDPM loop plain and with
   cache = (N, 0) for N = 2, 3, 5, legs plain_a, n2, n3, n5, plain_b interleaved in one process, 8 steps
   untimed and then 60 (whole cycles of every N) between two device events: ms per step, each cached leg
   as a ratio to the plain mean, the spread of the two plain legs.  The plain leg replays its 8-step
   graph, a cached leg one one-step graph per step.  Then the refresh step against the plain step, both as
   60 one-step loop calls (one-step graph replays with the same host work).  Then images/s of
   sample_latent_cond(ddpm, T = 1000) with the decode, plain against cache_interval = 3.

There is no fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "diffusion-model_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

B, HW, T, S, GUIDANCE = 64, 32, 1000, 50, 3.0
WARM, TIMED = 8, 48


def make_inputs(dev, seed=0):
    """bench.py's synthetic inputs: x_T ~ N(0,1), y cycles 1,2,3, cond U[0,1) masked to the class keys."""
    from diff import CLASS_KEYS, KEY_ORDER
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, HW, HW), generator=g)
    y = torch.tensor([1 + i % 3 for i in range(B)], dtype=torch.long)
    mask = torch.zeros((B, 12))
    for i in range(B):
        for k in CLASS_KEYS[int(y[i])]:
            mask[i, KEY_ORDER.index(k)] = 1.0
    vals = torch.rand((B, 12), generator=g) * mask
    return x.to(dev), y.to(dev), vals.to(dev), mask.to(dev)


def loop_legs(nm, d, dev, rounds):
    x0, y, vals, mask = make_inputs(dev)
    x = torch.empty_like(x0)
    t_dev = torch.zeros((1,), dtype=torch.long, device=dev)
    tables = d.coef_tables(dev, True)
    sched = d.ddim_tables(S, 1.0, dev)
    dpm_sched, hist = d.dpm_tables(S, "logsnr", dev), torch.empty_like(x0)
    inv_tab, src = d.invert_tables(S, None, 1, dev), torch.empty_like(x0)
    inv_rows = int(inv_tab[0].numel())

    def leg(kind):
        # (the few-step legs start at position S: no history needed; the inversion at its first row)
        start = T if kind == "ddpm" else inv_rows if kind == "invert" else S
        kw = {"ddpm": dict(seed=1234), "ddim": dict(seed=1234, sched=sched),
              "dpm": dict(sched=dpm_sched, hist=hist), "invert": dict(invert=(inv_tab, src))}[kind]
        tab = tables if kind == "ddpm" else None
        x.copy_(x0)
        src.copy_(x0)
        t_dev.fill_(start)
        nm.sample_loop(x, t_dev, y, 0, vals, mask, GUIDANCE, tab, WARM, **kw)  # captures this loop's graphs
        x.copy_(x0)
        src.copy_(x0)
        t_dev.fill_(start)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        nm.sample_loop(x, t_dev, y, 0, vals, mask, GUIDANCE, tab, TIMED, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert int(t_dev.item()) == start - TIMED and bool(torch.isfinite(x).all())
        return e0.elapsed_time(e1) / TIMED

    ms = {"ddpm_a": [], "ddim": [], "dpmpp_2m": [], "invert": [], "ddpm_b": []}
    leg("ddpm")  # workspace, split planes, time table
    for _ in range(rounds):
        ms["ddpm_a"].append(leg("ddpm"))
        ms["ddim"].append(leg("ddim"))
        ms["dpmpp_2m"].append(leg("dpm"))
        ms["invert"].append(leg("invert"))
        ms["ddpm_b"].append(leg("ddpm"))
    med = {k: statistics.median(v) for k, v in ms.items()}
    ddpm_mean = 0.5 * (med["ddpm_a"] + med["ddpm_b"])
    return {"ms_per_step_ddpm_a": round(med["ddpm_a"], 4), "ms_per_step_ddpm_b": round(med["ddpm_b"], 4),
            "ms_per_step_ddim": round(med["ddim"], 4), "ms_per_step_dpmpp_2m": round(med["dpmpp_2m"], 4),
            "ms_per_row_invert": round(med["invert"], 4),
            "invert_minus_ddim_ms": round(med["invert"] - med["ddim"], 4),
            "ddpm_spread_ms": round(abs(med["ddpm_a"] - med["ddpm_b"]), 4),
            "ddim_minus_ddpm_mean_ms": round(med["ddim"] - ddpm_mean, 4),
            "dpmpp_2m_minus_ddpm_mean_ms": round(med["dpmpp_2m"] - ddpm_mean, 4),
            "dpmpp_2m_minus_ddim_ms": round(med["dpmpp_2m"] - med["ddim"], 4),
            "per_round_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}


def known_legs(nm, d, dev, rounds):
    """The DPM-Solver++(2M) loop with and without the known-region blend after every step: same schedule,
    buffers and method as loop_legs; the blend's operands are a latent, a draw and a half-plane mask."""
    x0, y, vals, mask = make_inputs(dev)
    x = torch.empty_like(x0)
    t_dev = torch.zeros((1,), dtype=torch.long, device=dev)
    sched, hist = d.dpm_tables(S, "logsnr", dev), torch.empty_like(x0)
    g = torch.Generator().manual_seed(5)
    z0, e0 = (torch.randn((B, 4, HW, HW), generator=g).to(dev) for _ in range(2))
    kmask = torch.zeros((B, 1, HW, HW), device=dev)
    kmask[..., HW // 2:] = 1.0
    known = (z0, e0, kmask) + tuple(d.known_tables(d.dpm_timesteps(S, "logsnr"), dev))

    def leg(blend):
        kw = dict(sched=sched, hist=hist, known=known) if blend else dict(sched=sched, hist=hist)
        x.copy_(x0)
        t_dev.fill_(S)
        nm.sample_loop(x, t_dev, y, 0, vals, mask, GUIDANCE, None, WARM, **kw)  # captures this loop's graphs
        x.copy_(x0)
        t_dev.fill_(S)
        torch.cuda.synchronize()
        e_0, e_1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e_0.record()
        nm.sample_loop(x, t_dev, y, 0, vals, mask, GUIDANCE, None, TIMED, **kw)
        e_1.record()
        torch.cuda.synchronize()
        assert int(t_dev.item()) == S - TIMED and bool(torch.isfinite(x).all())
        return e_0.elapsed_time(e_1) / TIMED

    ms = {"dpmpp_2m_a": [], "known": [], "dpmpp_2m_b": []}
    leg(False)
    for _ in range(rounds):
        ms["dpmpp_2m_a"].append(leg(False))
        ms["known"].append(leg(True))
        ms["dpmpp_2m_b"].append(leg(False))
    med = {k: statistics.median(v) for k, v in ms.items()}
    plain_mean = 0.5 * (med["dpmpp_2m_a"] + med["dpmpp_2m_b"])
    return {"ms_per_step_dpmpp_2m_a": round(med["dpmpp_2m_a"], 4),
            "ms_per_step_dpmpp_2m_b": round(med["dpmpp_2m_b"], 4), "ms_per_step_known": round(med["known"], 4),
            "dpmpp_2m_spread_ms": round(abs(med["dpmpp_2m_a"] - med["dpmpp_2m_b"]), 4),
            "known_minus_dpmpp_2m_mean_ms": round(med["known"] - plain_mean, 4),
            "per_round_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}


def guidance_legs(nm, d, dev, rounds):
    """The DPM-Solver++(2M) loop plain (CFG), unguided (one conditional forward per step) and with the
    rescaled tail: same schedule, buffers and method as loop_legs."""
    x0, y, vals, mask = make_inputs(dev)
    x = torch.empty_like(x0)
    t_dev = torch.zeros((1,), dtype=torch.long, device=dev)
    sched, hist = d.dpm_tables(S, "logsnr", dev), torch.empty_like(x0)

    def leg(kind):
        g = 0.0 if kind == "unguided" else GUIDANCE
        kw = dict(sched=sched, hist=hist, **(dict(rescale=0.7) if kind == "rescaled" else {}))
        x.copy_(x0)
        t_dev.fill_(S)
        nm.sample_loop(x, t_dev, y, 0, vals, mask, g, None, WARM, **kw)  # captures this loop's graphs once
        x.copy_(x0)
        t_dev.fill_(S)
        torch.cuda.synchronize()
        e_0, e_1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e_0.record()
        nm.sample_loop(x, t_dev, y, 0, vals, mask, g, None, TIMED, **kw)
        e_1.record()
        torch.cuda.synchronize()
        assert int(t_dev.item()) == S - TIMED and bool(torch.isfinite(x).all())
        return e_0.elapsed_time(e_1) / TIMED

    ms = {"dpmpp_2m_a": [], "unguided": [], "rescaled": [], "dpmpp_2m_b": []}
    leg("plain")
    c0 = nm.graph_captures()
    for _ in range(rounds):
        ms["dpmpp_2m_a"].append(leg("plain"))
        ms["unguided"].append(leg("unguided"))
        ms["rescaled"].append(leg("rescaled"))
        ms["dpmpp_2m_b"].append(leg("plain"))
    med = {k: statistics.median(v) for k, v in ms.items()}
    plain_mean = 0.5 * (med["dpmpp_2m_a"] + med["dpmpp_2m_b"])
    return {"ms_per_step_dpmpp_2m_a": round(med["dpmpp_2m_a"], 4),
            "ms_per_step_dpmpp_2m_b": round(med["dpmpp_2m_b"], 4),
            "ms_per_step_unguided": round(med["unguided"], 4), "ms_per_step_rescaled": round(med["rescaled"], 4),
            "dpmpp_2m_spread_ms": round(abs(med["dpmpp_2m_a"] - med["dpmpp_2m_b"]), 4),
            "unguided_over_dpmpp_2m_mean": round(med["unguided"] / plain_mean, 4),
            "rescaled_minus_dpmpp_2m_mean_ms": round(med["rescaled"] - plain_mean, 4),
            "graph_captures_in_rounds": nm.graph_captures() - c0,
            "per_round_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}


def composed_legs(nm, d, dev, rounds):
    """The DPM-Solver++(2M) loop plain (CFG) and composed with K = 1, 2, 4 branches over the base, and the
    unbatched K = 2 step (K + 1 forwards, compose_eps, dpm_update): same schedule, buffers and method as
    loop_legs.  Branch 0 is the null label with the call's rows, branch 1 the call's condition; further
    branches cycle the labels and reuse the rows; every weight is GUIDANCE."""
    from dmx import engine
    x0, y, vals, mask = make_inputs(dev)
    x = torch.empty_like(x0)
    t_dev = torch.zeros((1,), dtype=torch.long, device=dev)
    sched, hist = d.dpm_tables(S, "logsnr", dev), torch.empty_like(x0)

    def tables(K):
        ys = [torch.zeros_like(y), y] + [1 + (y + k) % 3 for k in range(K - 1)]
        return (torch.stack(ys).contiguous(), torch.stack([vals] * (K + 1)).contiguous(),
                torch.stack([mask] * (K + 1)).contiguous(), torch.full((K, B), GUIDANCE, device=dev))

    comps = {K: tables(K) for K in (1, 2, 4)}

    def leg(K):  # K = 0: the plain CFG loop
        kw = dict(sched=sched, hist=hist, **(dict(compose=comps[K]) if K else {}))
        a = (None, 0, None, None, 0.0) if K else (y, 0, vals, mask, GUIDANCE)
        x.copy_(x0)
        t_dev.fill_(S)
        nm.sample_loop(x, t_dev, *a, None, WARM, **kw)  # captures this loop's graphs once
        x.copy_(x0)
        t_dev.fill_(S)
        torch.cuda.synchronize()
        e_0, e_1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e_0.record()
        nm.sample_loop(x, t_dev, *a, None, TIMED, **kw)
        e_1.record()
        torch.cuda.synchronize()
        assert int(t_dev.item()) == S - TIMED and bool(torch.isfinite(x).all())
        return e_0.elapsed_time(e_1) / TIMED

    def unbatched(K):
        y_rows, v_rows, m_rows, w = comps[K]
        xx = x0.clone()

        def steps(n, p):
            cur = xx
            for i in range(n):
                pos = torch.full((B,), p - i, dtype=torch.long, device=dev)
                tt = sched[0][pos - 1]
                es = [nm.forward(cur, tt, y_rows[k], v_rows[k], m_rows[k])[0] for k in range(K + 1)]
                cur = engine.dpm_update(cur, engine.compose_eps(es, w), None, 0.0, pos, sched, hist)
            return cur

        steps(WARM, S)
        torch.cuda.synchronize()
        e_0, e_1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e_0.record()
        out = steps(TIMED, S)
        e_1.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        return e_0.elapsed_time(e_1) / TIMED

    ws = {}
    leg(0)
    leg(1)
    leg(2)
    ws["workspace_bytes_k2"] = nm.workspace_bytes()
    leg(4)
    ws["workspace_bytes_k4"] = nm.workspace_bytes()
    ms = {"dpmpp_2m_a": [], "composed_k1": [], "composed_k2": [], "composed_k4": [], "unbatched_k2": [],
          "dpmpp_2m_b": []}
    for _ in range(rounds):
        ms["dpmpp_2m_a"].append(leg(0))
        ms["composed_k1"].append(leg(1))
        ms["composed_k2"].append(leg(2))
        ms["composed_k4"].append(leg(4))
        ms["unbatched_k2"].append(unbatched(2))
        ms["dpmpp_2m_b"].append(leg(0))
    med = {k: statistics.median(v) for k, v in ms.items()}
    plain_mean = 0.5 * (med["dpmpp_2m_a"] + med["dpmpp_2m_b"])
    out = {"ms_per_step_" + k: round(v, 4) for k, v in med.items()}
    out.update({"dpmpp_2m_spread_ms": round(abs(med["dpmpp_2m_a"] - med["dpmpp_2m_b"]), 4),
                "composed_k1_minus_dpmpp_2m_mean_ms": round(med["composed_k1"] - plain_mean, 4),
                "composed_k2_over_dpmpp_2m_mean": round(med["composed_k2"] / plain_mean, 4),
                "composed_k4_over_dpmpp_2m_mean": round(med["composed_k4"] / plain_mean, 4),
                "unbatched_k2_over_composed_k2": round(med["unbatched_k2"] / med["composed_k2"], 4), **ws,
                "per_round_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}})
    return out


def pag_legs(nm, d, dev, rounds):
    """The DPM-Solver++(2M) loop plain (CFG), composed with three ordinary branches (K = 2) and with
    perturbed-attention guidance — the same three branches, the last one the main condition's rows with
    identity attention in sa3 alone or in all six blocks: same schedule, buffers and method as loop_legs.
    The plain leg runs first and last in every round: the spread of one loop measured twice."""
    x0, y, vals, mask = make_inputs(dev)
    x = torch.empty_like(x0)
    t_dev = torch.zeros((1,), dtype=torch.long, device=dev)
    sched, hist = d.dpm_tables(S, "logsnr", dev), torch.empty_like(x0)
    ys = torch.stack([torch.zeros_like(y), y, y]).contiguous()
    comp = (ys, torch.stack([vals] * 3).contiguous(), torch.stack([mask] * 3).contiguous(),
            torch.stack([torch.full((B,), 2 * GUIDANCE, device=dev), torch.full((B,), -GUIDANCE, device=dev)]))
    modes = {"dpmpp_2m": None, "composed_k2": {}, "pag_sa3": dict(perturb=(0b000100, 0b100)),
             "pag_all6": dict(perturb=(0b111111, 0b100))}

    def leg(kind):
        extra = modes[kind]
        kw = dict(sched=sched, hist=hist, **(dict(compose=comp, **extra) if extra is not None else {}))
        a = (None, 0, None, None, 0.0) if extra is not None else (y, 0, vals, mask, GUIDANCE)
        x.copy_(x0)
        t_dev.fill_(S)
        nm.sample_loop(x, t_dev, *a, None, WARM, **kw)  # captures this loop's graphs once
        x.copy_(x0)
        t_dev.fill_(S)
        torch.cuda.synchronize()
        e_0, e_1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e_0.record()
        nm.sample_loop(x, t_dev, *a, None, TIMED, **kw)
        e_1.record()
        torch.cuda.synchronize()
        assert int(t_dev.item()) == S - TIMED and bool(torch.isfinite(x).all())
        return e_0.elapsed_time(e_1) / TIMED

    for kind in ("pag_all6", "pag_sa3", "composed_k2", "dpmpp_2m"):  # (the arena reaches its size first)
        leg(kind)
    ws = nm.workspace_bytes()
    c0 = nm.graph_captures()
    ms = {"dpmpp_2m_a": [], "composed_k2": [], "pag_sa3": [], "pag_all6": [], "dpmpp_2m_b": []}
    for _ in range(rounds):
        ms["dpmpp_2m_a"].append(leg("dpmpp_2m"))
        ms["composed_k2"].append(leg("composed_k2"))
        ms["pag_sa3"].append(leg("pag_sa3"))
        ms["pag_all6"].append(leg("pag_all6"))
        ms["dpmpp_2m_b"].append(leg("dpmpp_2m"))
    med = {k: statistics.median(v) for k, v in ms.items()}
    plain_mean = 0.5 * (med["dpmpp_2m_a"] + med["dpmpp_2m_b"])
    out = {"ms_per_step_" + k: round(v, 4) for k, v in med.items()}
    out.update({"dpmpp_2m_spread_ms": round(abs(med["dpmpp_2m_a"] - med["dpmpp_2m_b"]), 4),
                "composed_k2_over_dpmpp_2m_mean": round(med["composed_k2"] / plain_mean, 4),
                "pag_sa3_over_composed_k2": round(med["pag_sa3"] / med["composed_k2"], 4),
                "pag_all6_over_composed_k2": round(med["pag_all6"] / med["composed_k2"], 4),
                "pag_sa3_over_dpmpp_2m_mean": round(med["pag_sa3"] / plain_mean, 4),
                "pag_all6_over_dpmpp_2m_mean": round(med["pag_all6"] / plain_mean, 4),
                "workspace_bytes": ws, "graph_captures_in_rounds": nm.graph_captures() - c0,
                "per_round_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}})
    return out


def cache_legs(nm, d, dev, rounds):
    """The DDPM loop plain and feature-cached (refresh every N-th step): see the module docstring."""
    x0, y, vals, mask = make_inputs(dev)
    x = torch.empty_like(x0)
    t_dev = torch.zeros((1,), dtype=torch.long, device=dev)
    tables = d.coef_tables(dev, True)
    timed = 60

    def leg(n, calls=1):
        kw = dict(seed=1234, **({} if n == 1 else dict(cache=(n, 0))))
        per = timed // calls
        x.copy_(x0)
        t_dev.fill_(T)
        nm.sample_loop(x, t_dev, y, 0, vals, mask, GUIDANCE, tables, WARM if calls == 1 else 1, **kw)
        x.copy_(x0)
        t_dev.fill_(T)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            nm.sample_loop(x, t_dev, y, 0, vals, mask, GUIDANCE, tables, per, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert int(t_dev.item()) == T - timed and bool(torch.isfinite(x).all())
        return e0.elapsed_time(e1) / timed

    ms = {"plain_a": [], "n2": [], "n3": [], "n5": [], "plain_b": [], "plain_1step": [], "refresh_1step": []}
    leg(1)  # workspace, split planes, time table
    c0 = nm.graph_captures()
    for _ in range(rounds):
        ms["plain_a"].append(leg(1))
        ms["n2"].append(leg(2))
        ms["n3"].append(leg(3))
        ms["n5"].append(leg(5))
        ms["plain_b"].append(leg(1))
    for _ in range(rounds):  # every call is one step: the plain one-step graph against the refresh kind's
        ms["plain_1step"].append(leg(1, calls=timed))
        ms["refresh_1step"].append(leg(2, calls=timed))
    med = {k: statistics.median(v) for k, v in ms.items()}
    plain = 0.5 * (med["plain_a"] + med["plain_b"])
    out = {"ms_per_step_" + k: round(v, 4) for k, v in med.items()}
    out.update({"plain_spread_ms": round(abs(med["plain_a"] - med["plain_b"]), 4),
                "n2_over_plain_mean": round(med["n2"] / plain, 4), "n3_over_plain_mean": round(med["n3"] / plain, 4),
                "n5_over_plain_mean": round(med["n5"] / plain, 4),
                "refresh_minus_plain_1step_ms": round(med["refresh_1step"] - med["plain_1step"], 4),
                "graph_captures_in_rounds": nm.graph_captures() - c0, "workspace_bytes": nm.workspace_bytes(),
                "per_round_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}})
    return out


def pred_kw(prediction):
    """--prediction as Diffuser keywords."""
    return dict(prediction="v", x0_form=True) if prediction == "v_x0" else dict(prediction=prediction)


def cache_end_to_end(model, dev, prediction="eps"):
    """sample_latent_cond(ddpm, T = 1000) with the decode: plain, cache_interval = 3, plain again."""
    import diff
    from dmx import synth
    from models.vae import VAE
    vae = VAE()
    vae.load_state_dict(synth.vae_weights(1))
    vae = vae.to(dev).eval()
    _, y, vals, mask = make_inputs(dev, seed=11)
    counts = [(c, int((y == c).sum())) for c in (1, 2, 3)]
    order = torch.argsort(y, stable=True)
    vals, mask = vals[order].contiguous(), mask[order].contiguous()
    kw = dict(z_shape=(4, HW, HW), vae=vae, to_pil=True, progress=False, guidance_scale=GUIDANCE, cond=vals,
              cond_mask=mask)
    d = diff.Diffuser(T, device=dev, **pred_kw(prediction))
    d.noise_source = "device"
    d._decode(vae, torch.randn((B, 4, HW, HW), device=dev), True)  # decode workspace
    out = {}
    for name, extra in (("plain_a", {}), ("n3", dict(cache_interval=3)), ("plain_b", {})):
        secs = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            imgs = d.sample_latent_cond(model, counts, **kw, **extra)
            secs.append(time.perf_counter() - t0)
            assert len(imgs) == B and imgs[0].size == (8 * HW, 8 * HW)
        out[name] = {"first_call_s": round(secs[0], 4), "steady_s": round(secs[1], 4),
                     "steady_images_per_s": round(B / secs[1], 2)}
    out["range_fallbacks"] = d.range_fallbacks
    return out


def end_to_end(model, dev, prediction="eps"):
    import diff
    from dmx import synth
    from models.vae import VAE
    vae = VAE()
    vae.load_state_dict(synth.vae_weights(1))
    vae = vae.to(dev).eval()
    _, y, vals, mask = make_inputs(dev, seed=11)
    counts = [(c, int((y == c).sum())) for c in (1, 2, 3)]
    order = torch.argsort(y, stable=True)  # the sampler lays out classes in count order
    vals, mask = vals[order].contiguous(), mask[order].contiguous()
    kw = dict(z_shape=(4, HW, HW), vae=vae, to_pil=True, progress=False, guidance_scale=GUIDANCE, cond=vals,
              cond_mask=mask)
    d = diff.Diffuser(T, device=dev, **pred_kw(prediction))
    d.noise_source = "device"
    d._decode(vae, torch.randn((B, 4, HW, HW), device=dev), True)  # decode workspace
    out = {}
    tau20 = d.dpm_timesteps(20)
    half = dict(sampler="dpmpp_2m", steps=20, guidance_interval=(tau20[5], tau20[14]))  # positions 6..15
    for name, extra, calls in (("ddim_S50_eta0", dict(sampler="ddim", steps=S, eta=0.0), 4),
                               ("dpmpp_2m_S20", dict(sampler="dpmpp_2m", steps=20), 4),
                               ("dpmpp_2m_S20_interval_half", half, 4), ("ddpm_T1000", {}, 2)):
        secs = []
        c0 = model.native().graph_captures()
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            imgs = d.sample_latent_cond(model, counts, **kw, **extra)
            secs.append(time.perf_counter() - t0)
            assert len(imgs) == B and imgs[0].size == (8 * HW, 8 * HW)
        out[name] = {"first_call_s": round(secs[0], 4), "first_call_images_per_s": round(B / secs[0], 2),
                     "steady_s": round(min(secs[1:]), 4), "steady_images_per_s": round(B / min(secs[1:]), 2),
                     "calls_s": [round(v, 4) for v in secs],
                     "graph_captures": model.native().graph_captures() - c0}
    # the edit round trip: invert 6 of 20 positions with two refinements (18 rows), sample back, decode
    g = torch.Generator().manual_seed(12)
    z0 = (0.8 * torch.randn((B, 4, HW, HW), generator=g)).to(dev)
    kw_inv = dict(guidance_scale=GUIDANCE, cond=vals, cond_mask=mask)
    kw_back = dict(kw, start_latent=None, strength=0.3, sampler="ddim", steps=20)
    del kw_back["z_shape"]
    secs = []
    c0 = model.native().graph_captures()
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = d.invert_latent_cond(model, z0, counts, steps=20, strength=0.3, refine=2, **kw_inv)
        imgs = d.sample_latent_cond(model, counts, **dict(kw_back, start_latent=lat))
        secs.append(time.perf_counter() - t0)
        assert len(imgs) == B and imgs[0].size == (8 * HW, 8 * HW)
    out["invert_S20_s0.3_R2_plus_resample"] = {
        "first_call_s": round(secs[0], 4), "first_call_images_per_s": round(B / secs[0], 2),
        "steady_s": round(min(secs[1:]), 4), "steady_images_per_s": round(B / min(secs[1:]), 2),
        "calls_s": [round(v, 4) for v in secs], "graph_captures": model.native().graph_captures() - c0}
    out["range_fallbacks"] = d.range_fallbacks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--groups", default="loops,known_loops,guidance_loops,composed_loops,pag_loops,end_to_end")
    ap.add_argument("--prediction", default="eps", choices=["eps", "v"] + ["v_x0"],  # (v_x0: v in x0-form)
                    help="what the network's output is read as")
    args = ap.parse_args()
    groups = args.groups.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench needs an MI355X: no GPU visible, and there is no fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import diff
    from dmx import synth
    from models.unet_cond_geom import UnetCondWithGeomHead
    model = UnetCondWithGeomHead()
    model.load_state_dict(synth.unet_cond_geom_weights(0))
    model.to(dev).eval()
    res = {"workload": f"B={B}, {HW}x{HW}x4, CFG {GUIDANCE}, device noise, synthetic weights; T={T}, S={S}",
           "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "prediction": args.prediction}

    def diffuser():  # (the loop legs drive the native model themselves: it is told the prediction here)
        d = diff.Diffuser(T, device=dev, **pred_kw(args.prediction))
        d._set_prediction(model.native())
        return d
    for name, fn in (("loops", loop_legs), ("known_loops", known_legs), ("guidance_loops", guidance_legs),
                     ("composed_loops", composed_legs), ("pag_loops", pag_legs)):
        if name in groups:
            res[name] = fn(model.native(), diffuser(), dev, args.rounds)
    if "end_to_end" in groups:
        res["end_to_end"] = end_to_end(model, dev, args.prediction)
    if "cache" in groups:
        res["cache"] = cache_legs(model.native(), diffuser(), dev, args.rounds)
        res["cache"]["ddpm_T1000_end_to_end"] = cache_end_to_end(model, dev, args.prediction)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
