"""GPU: feature caching — refresh and reuse steps, loops, samplers and the validity
rules, against the oracle of tests/test_cache_host.py (full / shallow, restated from oracle.ref).

A refresh step is the plain step bit for bit and leaves D = sa5's output in the model; a reuse step
runs inc, up3, sa6 and the head on the stored D.  Bounds are the project's: TOL = 2e-5 for one step,
TRAJ_TOL = 1e-4 for a trajectory (rel-L2 against the fp32 torch-CPU oracle).

Measured on an MI355X (synthetic weights; every figure is printed by its test before it is asserted,
and DESIGN §6s has the whole table).  cached_features() against the oracle's D: 1.8e-6 (x3; f16 mode
7.2e-4 against that mode's forward bound 2e-3).  Reuse step at (x_b, t = 440) on the D of (x_a, t = 740): B = 2 32x32 x3 2.5e-7,
fp32 2.5e-7; 28x28 x3 2.4e-7, fp32 2.5e-7; B = 3 2.2e-7; B = 32 2.4e-7; B = 2 unguided 1.1e-7 — where the
oracle's cached eps differs from its full eps by 0.28 - 0.54 and the x_out built on them by 1.4e-2 -
4.2e-2.  Trajectories: DDIM S = 6 32x32 N = 3 2.0e-6, N = 2 1.9e-6, 28x28 N = 3 1.8e-6, N = 2 1.8e-6;
DPM-Solver++(2M) N = 2 1.9e-6; DDPM T = 12 host noise N = 4 6.5e-7 (cached against uncached oracle 0.030 -
0.097).  Chunks of 4, S = 10, N = 3: 1.5e-6, and the same with one chunk replayed in fp32."""
import pytest
import torch

from oracle import ref
from oracle.rules import ddim_update, dpm_update, rel
from support import make_model, on, run_worker
from test_cache_host import CachedEps, cached_trajectory, refresh_positions, step_inputs

pytestmark = pytest.mark.gpu

TOL = 2e-5        # one step (the project's step bound)
TRAJ_TOL = 1e-4   # a trajectory (the project's trajectory bound)
F16_TOL = 2e-3    # a network output in f16 mode (the project's f16 forward bound, test_gpu_f16.TOL_FWD)
G = 3.0
S50, POS_A, POS_B = 50, 37, 22   # the DDIM schedule of the step tests: t = 740 and t = 440


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    return make_model(cuda, unet_sd)


@pytest.fixture(scope="module")
def d(cuda):
    import diff
    return diff.Diffuser(1000, device=cuda)


def ddim_step(nm, sched, x, p, y, vals, mask, g=G, cache=None, out=None):
    """One native DDIM step at position p -> x_out (a new tensor unless `out` is given)."""
    dev = x.device
    out = torch.empty_like(x) if out is None else out
    pos = torch.full((x.shape[0],), p, dtype=torch.long, device=dev)
    nm.step(x, out, pos, y, 0, vals, mask, g, None, sched=sched, **({} if cache is None else dict(cache=cache)))
    return out


# ---- 1: a refresh step is the plain step -----------------------------------------------------------
@pytest.mark.parametrize("B,hw,prec", [(2, 32, "x3"), (2, 32, "f16"), (32, 32, "x3")])
def test_refresh_step_is_the_plain_step_bit_for_bit(model, d, cuda, unet_sd, B, hw, prec):
    nm = model.native()
    x_a, _, y, vals, mask = step_inputs(B, hw, 100 + B)
    x, yd, vd, md = on(cuda, x_a, y, vals, mask)
    g = torch.Generator().manual_seed(7)
    noise = torch.randn(x_a.shape, generator=g).to(cuda)
    ddim, dpm, tables = d.ddim_tables(S50, 0.5, cuda), d.dpm_tables(S50, "logsnr", cuda), d.coef_tables(cuda, True)
    pos = torch.full((B,), POS_A, dtype=torch.long, device=cuda)
    t = torch.full((B,), 740, dtype=torch.long, device=cuda)
    with nm.precision_override(prec):
        for rule in ("ddpm", "ddim", "dpm"):
            outs = []
            for cache in (None, (3, 0), (3, 3), (1, 0)):
                kw = {} if cache is None else dict(cache=cache)
                out = torch.empty_like(x)
                hist = torch.randn(x_a.shape, generator=torch.Generator().manual_seed(8)).to(cuda)
                if rule == "ddpm":
                    nm.step(x, out, t, yd, 0, vd, md, G, tables, noise, **kw)
                elif rule == "ddim":
                    nm.step(x, out, pos, yd, 0, vd, md, G, None, noise, sched=ddim, **kw)
                else:
                    nm.step(x, out, pos - 1, yd, 0, vd, md, G, None, sched=dpm, hist=hist, **kw)
                outs.append((out, hist))
            for out, hist in outs[1:]:
                assert torch.equal(out, outs[0][0]) and torch.equal(hist, outs[0][1]), rule
            assert torch.isfinite(outs[0][0]).all()
        # the feature the last refresh left (DPM at position POS_A - 1) against the oracle's
        D = nm.cached_features()
        assert tuple(D.shape) == (2 * B, hw // 2, hw // 2, 64)
        if B == 2:
            e = CachedEps(unet_sd, y, vals, mask, G)
            e(x_a, d.dpm_tables(S50, "logsnr", "cpu")[0][POS_A - 2].expand(B), True)
            err = rel(D, e.features())
            print(f"[cache D {prec}] B={B} {hw}x{hw}: rel-L2 vs oracle = {err:.3e}")
            # D is an output of the forward: in f16 mode (operands rounded to fp16) it is held to that mode's
            # forward bound, which TOL is not meant for; B = 32 is compared in the reuse test below
            assert err <= (F16_TOL if prec == "f16" else TOL), err


# ---- 2: a reuse step against the oracle ------------------------------------------------------------
@pytest.mark.parametrize("B,hw,prec,g", [(2, 32, "x3", G), (2, 32, "fp32", G), (2, 28, "x3", G), (2, 28, "fp32", G),
                                         (3, 32, "x3", G), (32, 32, "x3", G), (2, 32, "x3", 0.0)])
def test_reuse_step_against_the_oracle(model, d, cuda, unet_sd, B, hw, prec, g):
    nm = model.native()
    x_a, x_b, y, vals, mask = step_inputs(B, hw, 200 + B + hw)
    xa, xb, yd, vd, md = on(cuda, x_a, x_b, y, vals, mask)
    sched, csched = d.ddim_tables(S50, 0.0, cuda), d.ddim_tables(S50, 0.0, "cpu")
    with nm.precision_override(prec):
        ddim_step(nm, sched, xa, POS_A, yd, vd, md, g, cache=(3, 0))
        D = nm.cached_features()
        out = ddim_step(nm, sched, xb, POS_B, yd, vd, md, g, cache=(3, 1))
        assert torch.equal(nm.cached_features(), D)  # a reuse step leaves D alone
    assert D.shape[0] == (2 * B if g > 0 else B)
    e = CachedEps(unet_sd, y, vals, mask, g)
    e(x_a, csched[0][POS_A - 1].expand(B), True)
    tb = csched[0][POS_B - 1].expand(B)
    eps_cached = e(x_b, tb, False)
    eps_full = CachedEps(unet_sd, y, vals, mask, g)(x_b, tb, True)
    gap = rel(eps_cached, eps_full)
    exp = ddim_update(x_b, eps_cached, POS_B, csched)
    err, err_d = rel(out, exp), rel(D, e.features())
    wrong = rel(ddim_update(x_b, eps_full, POS_B, csched), exp)
    print(f"[cache reuse {prec}] B={B} {hw}x{hw} g={g}: rel-L2 vs oracle = {err:.3e} (D {err_d:.3e}); oracle cached vs "
          f"full eps {gap:.3e}, x_out {wrong:.3e}")
    assert gap > 1e-2, gap          # a reuse step that silently ran the full network cannot pass:
    assert wrong > 100 * TOL, wrong  # its x_out would sit this far from the cached oracle's
    assert err <= TOL, err
    assert err_d <= TOL, err_d


# ---- 3: shards ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [16, 28])
def test_refresh_reuse_pair_equals_its_shards(model, d, cuda, hw):
    nm = model.native()
    B = 5
    x_a, x_b, y, vals, mask = step_inputs(B, hw, 300 + hw)
    xa, xb, yd, vd, md = on(cuda, x_a, x_b, y, vals, mask)
    sched = d.ddim_tables(S50, 0.0, cuda)

    def pair(s, e):
        r = ddim_step(nm, sched, xa[s:e].contiguous(), POS_A, yd[s:e], vd[s:e].contiguous(), md[s:e].contiguous(),
                      cache=(2, 0))
        u = ddim_step(nm, sched, xb[s:e].contiguous(), POS_B, yd[s:e], vd[s:e].contiguous(), md[s:e].contiguous(),
                      cache=(2, 1))
        return r, u, nm.cached_features()

    whole, lo, hi = pair(0, B), pair(0, 3), pair(3, B)
    assert torch.equal(whole[0], torch.cat([lo[0], hi[0]]))
    assert torch.equal(whole[1], torch.cat([lo[1], hi[1]]))
    # D: the null half first, then the conditional half, each in batch order
    assert torch.equal(whole[2], torch.cat([lo[2][:3], hi[2][:2], lo[2][3:], hi[2][2:]]))


# ---- 4: the loop's forms are one computation ---------------------------------------------------------
@pytest.mark.parametrize("B,hw", [(4, 16), (32, 32)])
def test_loop_forms_are_bit_equal(model, d, cuda, unet_sd, B, hw):
    x_a, _, y, vals, mask = step_inputs(B, hw, 400 + B)
    sched = d.ddim_tables(7, 1.0, cuda)  # eta = 1: every step but the last draws Philox noise
    outs = {}

    def loop(nm, use_graph):
        x, yd, vd, md = on(cuda, x_a.clone(), y, vals, mask)
        t_dev = torch.full((1,), 7, dtype=torch.long, device=cuda)
        nm.sample_loop(x, t_dev, yd, 0, vd, md, G, None, 7, seed=41, use_graph=use_graph, sched=sched, cache=(3, 0))
        torch.cuda.synchronize()
        assert int(t_dev.item()) == 0
        return x

    nm = model.native()
    outs["graph"] = loop(nm, True)
    outs["graph again"] = loop(nm, True)
    outs["eager"] = loop(nm, False)
    x, yd, vd, md = on(cuda, x_a.clone(), y, vals, mask)
    for k in range(7):
        out = torch.empty_like(x)
        pos = torch.full((B,), 7 - k, dtype=torch.long, device=cuda)
        nm.step(x, out, pos, yd, 0, vd, md, G, None, None, seed=41, sched=sched, cache=(3, k))
        x = out
    outs["steps"] = x
    outs["fresh model"] = loop(make_model(cuda, unet_sd).native(), True)
    assert torch.isfinite(outs["graph"]).all()
    for k, v in outs.items():
        assert torch.equal(v, outs["graph"]), k
    plain = on(cuda, x_a.clone())[0]
    nm.sample_loop(plain, torch.full((1,), 7, dtype=torch.long, device=cuda), yd, 0, vd, md, G, None, 7, seed=41,
                   sched=sched)
    assert not torch.equal(plain, outs["graph"])  # (the cached loop is another computation than the plain one)


# ---- 5, 6: trajectories of the samplers against the oracle under the chunk rule ---------------------------
def oracle_trajectory(d, unet_sd, rule, sched, x_T, y, vals, mask, n, chunk, noises=None):
    """The sampler's loop on the oracle: eps from CachedEps, the rule's update restated in torch."""
    e = CachedEps(unet_sd, y, vals, mask, G)
    B = x_T.shape[0]
    hist = [torch.full_like(x_T, float("nan"))]
    _, alphas, alpha_bars = ref.schedule(d.num_timesteps)

    def eps_of(x, p, refresh):
        t = torch.full((B,), p, dtype=torch.long) if rule == "ddpm" else sched[0][p - 1].expand(B)
        return e(x, t, refresh)

    def update(x, eps, p):
        if rule == "ddim":
            return ddim_update(x, eps, p, sched)
        if rule == "dpm":
            out, hist[0] = dpm_update(x, eps, p, sched, hist[0])
            return out
        return ref.ddpm_update(x, eps, torch.full((B,), p, dtype=torch.long), alphas, alpha_bars, noises[p])

    start = d.num_timesteps if rule == "ddpm" else int(sched[0].numel())
    return cached_trajectory(eps_of, x_T, start, n, chunk, update)


@pytest.mark.parametrize("sampler,hw,N", [("ddim", 32, 3), ("ddim", 32, 2), ("ddim", 28, 3), ("ddim", 28, 2),
                                          ("dpmpp_2m", 32, 2), ("ddpm", 32, 4)])
def test_trajectory_against_the_oracle(model, cuda, unet_sd, sampler, hw, N):
    import diff
    T = 12 if sampler == "ddpm" else 1000
    d = diff.Diffuser(T, device=cuda)
    d.noise_source = "host" if sampler == "ddpm" else "device"
    counts, B = {1: 1, 3: 1}, 2
    y = torch.tensor([1, 3])
    g = torch.Generator().manual_seed(500 + hw + N)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    kw = {} if sampler == "ddpm" else dict(sampler=sampler, steps=6)
    torch.manual_seed(62)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=G,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), cache_interval=N, **kw)
    assert d.range_fallbacks == 0
    torch.manual_seed(62)
    x_T = torch.randn((B, 4, hw, hw))
    noises = {p: torch.randn(x_T.shape) for p in range(T, 0, -1)} if sampler == "ddpm" else None
    rule = {"ddim": "ddim", "dpmpp_2m": "dpm", "ddpm": "ddpm"}[sampler]
    sched = None if rule == "ddpm" else d.ddim_tables(6, 0.0, "cpu") if rule == "ddim" else d.dpm_tables(6, "logsnr", "cpu")
    exp = oracle_trajectory(d, unet_sd, rule, sched, x_T, y, vals, mask, N, d.GUARD_CHUNK, noises)
    plain = oracle_trajectory(d, unet_sd, rule, sched, x_T, y, vals, mask, 1, d.GUARD_CHUNK, noises)
    err, gap = rel(out, exp), rel(exp, plain)
    print(f"[cache trajectory {sampler}] {hw}x{hw} N={N}: rel-L2 vs oracle = {err:.3e}; oracle cached vs uncached {gap:.3e}")
    assert gap > 1e-2, gap
    assert err <= TRAJ_TOL, err


def test_chunks_restart_the_count_and_a_replayed_chunk_refreshes_first(cuda, unet_sd):
    import diff
    model = make_model(cuda, unet_sd)
    nm = model.native()
    B, hw, S, N = 2, 32, 10, 3
    y = torch.tensor([2, 1])
    g = torch.Generator().manual_seed(600)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = "device"
    d.GUARD_CHUNK = 4
    assert refresh_positions(S, N, 4) == [10, 7, 6, 3, 2]  # chunk offsets 0 and 3
    torch.manual_seed(63)
    x_T = torch.randn((B, 4, hw, hw))
    sched = d.ddim_tables(S, 0.0, "cpu")
    exp = oracle_trajectory(d, unet_sd, "ddim", sched, x_T, y, vals, mask, N, 4)
    whole = oracle_trajectory(d, unet_sd, "ddim", sched, x_T, y, vals, mask, N, 50)  # (one chunk: refreshes 10, 7, 4, 1)

    def sample():
        torch.manual_seed(63)
        return d.sample_latent_cond(model, {2: 1, 1: 1}, z_shape=(4, hw, hw), vae=None, progress=False,
                                    guidance_scale=G, cond=vals.to(cuda), cond_mask=mask.to(cuda), sampler="ddim",
                                    steps=S, cache_interval=N)

    out = sample()
    err = rel(out, exp)
    print(f"[cache chunks] S={S} N={N} chunk 4: rel-L2 vs oracle = {err:.3e}; vs the one-chunk oracle {rel(out, whole):.3e}")
    assert d.range_fallbacks == 0 and err <= TRAJ_TOL, err
    assert rel(exp, whole) > 10 * TRAJ_TOL  # the chunk rule is visible in the result (CPU: 1.06e-2)
    # the range guard reports a trip once (a Python patch: nothing non-finite is computed): the second chunk
    # is replayed in fp32 from its own refresh step
    real, calls = nm.range_tripped, []

    def tripped_once(reset=True):
        calls.append(1)
        v = real(reset)
        return True if len(calls) == 2 else v

    nm.range_tripped = tripped_once
    try:
        out2 = sample()
    finally:
        del nm.range_tripped
    err2 = rel(out2, exp)
    print(f"[cache chunks] with the second chunk replayed in fp32: rel-L2 vs oracle = {err2:.3e}")
    assert d.range_fallbacks == 1 and nm.precision == "x3"
    assert err2 <= TRAJ_TOL, err2


@pytest.mark.parametrize("source,sampler", [("host", "ddpm"), ("device", "ddim"), ("host", "dpmpp_2m")])
def test_sharded_sampler_walks_the_same_cached_plan(model, cuda, source, sampler):
    """The sharded sampler (here one rank: its own loops, the same plan) equals the single-process one
    bit for bit under cache_interval, chunks of 4 included, and leaves the generator where it does."""
    import diff
    from dmx.distributed import ShardedCondSampler
    d = diff.Diffuser(12 if sampler == "ddpm" else 1000, device=cuda)
    d.noise_source = source
    d.GUARD_CHUNK = 4
    g = torch.Generator().manual_seed(650)
    vals = torch.rand((3, 12), generator=g).to(cuda)
    mask = (torch.rand((3, 12), generator=g) > 0.3).float().to(cuda)
    kw = dict(z_shape=(4, 16, 16), guidance_scale=G, cond=vals, cond_mask=mask, cache_interval=3,
              **({} if sampler == "ddpm" else dict(sampler=sampler, steps=10)))
    torch.manual_seed(64)
    single = d.sample_latent_cond(model, {1: 2, 3: 1}, vae=None, progress=False, **kw)
    state = torch.get_rng_state()
    torch.manual_seed(64)
    sharded = ShardedCondSampler(d, model, None).sample({1: 2, 3: 1}, decode=False, **kw)
    assert torch.isfinite(single).all() and torch.equal(sharded, single)
    assert torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(64)
    plain = d.sample_latent_cond(model, {1: 2, 3: 1}, vae=None, progress=False, **{**kw, "cache_interval": None})
    assert not torch.equal(plain, single) and d.range_fallbacks == 0


# ---- 7: a reuse step never reads a stale feature -------------------------------------------------------
def test_stale_cache_is_refused_and_nothing_is_written(cuda, unet_sd, d):
    from dmx import _lib
    model = make_model(cuda, unet_sd)
    nm = model.native()
    sched = d.ddim_tables(S50, 0.0, cuda)
    x_a, x_b, y, vals, mask = step_inputs(3, 16, 700)
    xa, xb, yd, vd, md = on(cuda, x_a, x_b, y, vals, mask)
    big = torch.randn((3, 4, 32, 32), generator=torch.Generator().manual_seed(1)).to(cuda)

    def refused(word, x=xb, rows=slice(0, 3), g=G, loop=False):
        out = torch.full_like(x[rows], 7.0)
        with pytest.raises(_lib.DmxError) as ei:
            if loop:
                t_dev = torch.full((1,), POS_B, dtype=torch.long, device=cuda)
                nm.sample_loop(out, t_dev, yd[rows], 0, vd[rows].contiguous(), md[rows].contiguous(), g, None, 2,
                               sched=sched, cache=(3, 1))
            else:
                ddim_step(nm, sched, x[rows].contiguous(), POS_B, yd[rows], vd[rows].contiguous(), md[rows].contiguous(),
                          g, cache=(3, 1), out=out)
        torch.cuda.synchronize()
        assert ei.value.code == _lib.DMX_E_STATE and word in str(ei.value), str(ei.value)
        assert bool((out == 7.0).all())

    def refresh():
        ddim_step(nm, sched, xa, POS_A, yd, vd, md, cache=(3, 0))

    assert nm.cached_features() is None
    refused("no refresh")
    refused("no refresh", loop=True)
    refresh()
    ddim_step(nm, sched, xb, POS_B, yd, vd, md, cache=(3, 1))  # (a matching one is accepted)
    refused("batch", rows=slice(0, 2))
    refused("map size", x=big)
    refused("step kind", g=0.0)
    refused("step kind", g=0.0, loop=True)
    nm.set_precision("fp32")
    refused("precision")
    nm.set_precision("x3")
    ddim_step(nm, sched, xb, POS_B, yd, vd, md, cache=(3, 1))  # (back in its mode the feature is valid again)
    nm.refresh()
    assert nm.cached_features() is not None  # (stored, but of other weights)
    refused("weights")
    refresh()
    ddim_step(nm, sched, xb, POS_B, yd, vd, md, cache=(3, 1))
    # a larger refresh reallocates the buffer; the excluded parts are DMX_E_ARG at the library too
    ddim_step(nm, sched, big, POS_A, yd, vd, md, cache=(3, 0))
    refused("map size")
    assert tuple(nm.cached_features().shape) == (6, 16, 16, 64)
    with pytest.raises(ValueError):
        nm.step(xa, torch.empty_like(xa), torch.full((3,), 5, device=cuda), yd, 0, vd, md, G, None, sched=sched,
                cache=(3, 0), perturb=(4, 4))
    # dmx_model_finalize starts a new generation of the weights as dmx_model_refresh does
    import ctypes
    refresh()
    with torch.cuda.device(cuda):
        _lib.check(nm.lib.dmx_model_finalize(nm.handle, ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)))
    refused("weights")


# ---- 8, 9: graph captures, and the plain path is untouched ------------------------------------------------
def test_graph_captures_and_the_plain_loop_is_unaffected(cuda, unet_sd, d):
    nm = make_model(cuda, unet_sd).native()
    B, hw = 2, 16
    x_a, _, y, vals, mask = step_inputs(B, hw, 800)
    sched = d.ddim_tables(9, 0.0, cuda)
    yd, vd, md = on(cuda, y, vals, mask)
    x = torch.empty((B, 4, hw, hw), device=cuda)  # one buffer: the graph keys hold its address
    t_dev = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(cache):
        x.copy_(x_a)
        t_dev.fill_(9)
        c0 = nm.graph_captures()
        nm.sample_loop(x, t_dev, yd, 0, vd, md, G, None, 9, sched=sched, **({} if cache is None else dict(cache=cache)))
        torch.cuda.synchronize()
        return x.clone(), nm.graph_captures() - c0

    cached, n = loop((3, 0))
    assert n == 2
    again, n = loop((3, 0))
    assert n == 0 and torch.equal(again, cached)
    plain, n = loop(None)
    assert n == 1 and not torch.equal(plain, cached)
    third, n = loop((3, 0))
    assert n == 0 and torch.equal(third, cached)
    other, n = loop((4, 0))  # another pattern replays the same two graphs
    assert n == 0 and not torch.equal(other, cached)
    off, n = loop((1, 0))    # interval 1 is the plain loop and shares its graphs
    assert n == 0 and torch.equal(off, plain)
    plain2, n = loop(None)
    assert n == 0 and torch.equal(plain2, plain)
    fresh = make_model(cuda, unet_sd).native()  # a model that never ran a cached call
    xf = x_a.to(cuda)
    fresh.sample_loop(xf, torch.full((1,), 9, dtype=torch.long, device=cuda), yd, 0, vd, md, G, None, 9, sched=sched)
    torch.cuda.synchronize()
    assert torch.equal(xf, plain)


# ---- 10: poison ------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys
import torch
sys.path[:0] = [os.path.join(ROOT, "diffusion-model_amd"), ROOT, os.path.join(ROOT, "tests")]
import diff
from dmx import synth
from models.unet_cond_geom import UnetCondWithGeomHead
dev = torch.device("cuda:0")
m = UnetCondWithGeomHead()
m.load_state_dict(synth.unet_cond_geom_weights(0))
nm = m.to(dev).eval().native()
d = diff.Diffuser(1000, device=dev)
sched = d.ddim_tables(50, 0.0, dev)
g = torch.Generator().manual_seed(40)
out = {}
for B, hw in ((5, 16), (5, 28), (64, 32)):
    xa = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    xb = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    vals = torch.rand((B, 12), generator=g).to(dev)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(dev)
    y = torch.tensor([1 + i % 3 for i in range(B)], device=dev)
    for k, (x, p) in enumerate(((xa, 37), (xb, 22))):
        o = torch.empty_like(x)
        nm.step(x, o, torch.full((B,), p, dtype=torch.long, device=dev), y, 0, vals, mask, 3.0, None, sched=sched,
                cache=(2, k))
        out[f"{B}_{hw}_{'refresh' if k == 0 else 'reuse'}"] = o.cpu()
    out[f"{B}_{hw}_D"] = nm.cached_features().cpu()
torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print("[cache-poison-worker] ok", flush=True)
'''


def test_cached_steps_read_no_unwritten_workspace(cuda, tmp_path):
    clean = run_worker(tmp_path, "clean", WORKER)
    poisoned = run_worker(tmp_path, "poison", WORKER, DMX_POISON="1")
    assert len(clean) == 9
    bad = [k for k in clean if not torch.isfinite(poisoned[k]).all() or not torch.equal(clean[k], poisoned[k])]
    assert bad == [], bad
