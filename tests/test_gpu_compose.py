"""GPU: composed guidance — K weighted condition branches over a chosen base, one (K+1) B forward per
step — against torch-CPU restatements that take every branch's eps from the oracle
(oracle.ref.unet_cond_geom_forward, one call per branch) and the tables from the Diffuser.

With e_k the prediction of branch k (branch 0 the base) and w_k[n] the weights, each op rounded once:
  d_k = e_k - e_0;  s = w_1 d_1;  s = s + w_k d_k (k = 2..K);  eps = e_0 + s
then the DDPM / DDIM / DPM update.  Bounds are the project's: TOL for one step, TRAJ_TOL for a trajectory.

Measured on an MI355X (rel-L2): composed steps against the oracle 2.3e-8 .. 3.9e-8 (ddpm), 4.7e-7 .. 1.3e-6
(ddim), 4.9e-7 .. 1.4e-6 (dpm); B = 32, K = 2 1.2e-6; trajectories 3.6e-7 .. 1.2e-6; foreign models 2.4e-8
(ddpm), 4.8e-7 (ddim), 4.9e-7 (dpm); the bit-equalities hold."""
import ctypes
import os

import pytest
import torch

from oracle import ref, rules
from oracle.rules import compose_mix, composed_eps, ddim_update, dpm_update, rel
from support import cond, device_noise, make_model, make_vae, mode_tables, run_worker

pytestmark = pytest.mark.gpu

TOL = 2e-5        # one step (the project's step bound)
TRAJ_TOL = 1e-4   # a trajectory (the project's trajectory bound)
G = 3.0


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    return make_model(cuda, unet_sd)


@pytest.fixture(scope="module")
def model2(cuda, unet_sd):
    """A second network with the same weights: its own arena and its own graph slots."""
    return make_model(cuda, unet_sd)


def weights(B, seed, lo=-2.0, hi=4.0, first=-1.0):
    """B weights in [lo, hi); the first one of sign `first` and at least 0.5 in size, the last exactly zero."""
    g = torch.Generator().manual_seed(seed)
    w = lo + (hi - lo) * torch.rand((B,), generator=g)
    w[0] = first * (0.5 + abs(w[0]))
    if B > 1:
        w[-1] = 0.0
    return w


def compose_case(d, name, B, seed):
    """The branch tables of a named composition on the CPU, built by the sampler's own _compose_args:
    (y, vals, mask of the call, (y_rows, vals_rows, mask_rows, weights))."""
    y, vals, mask = cond(B, seed)
    _, v2, m2 = cond(B, seed + 1)
    _, v3, m3 = cond(B, seed + 2)
    if name == "k1":       # the plain CFG step as a composition
        comp = d._compose_args(y.tolist(), vals, mask, [G] * B)
    elif name == "dropped2":   # K = 2 over the true unconditional base
        comp = d._compose_args(y.tolist(), vals, mask, weights(B, seed + 3).tolist(), "dropped",
                               [dict(classes=[1 + (i + 1) % 3 for i in range(B)], cond=v2, cond_mask=m2,
                                     weight=weights(B, seed + 4, -1.0, 2.0, first=1.0).tolist())])
    elif name == "negative3":  # K = 3 over a negative condition
        comp = d._compose_args(y.tolist(), vals, mask, weights(B, seed + 3).tolist(),
                               dict(classes=2, cond=v3, cond_mask=m3),
                               [dict(classes=3, cond=v2, cond_mask=m2,
                                     weight=weights(B, seed + 4, -1.0, 2.0, first=1.0).tolist()),
                                dict(classes=[1 + (i + 2) % 3 for i in range(B)], weight=-0.75)])
    elif name == "plain2":     # K = 2, scalar weights, base "null"
        comp = d._compose_args(y.tolist(), vals, mask, G, "null", [dict(classes=2, cond=v2, cond_mask=m2, weight=1.5)])
    else:
        raise KeyError(name)
    return y, vals, mask, comp


def to(comp, dev):
    return tuple(c.to(dev).contiguous() for c in comp)


# ---- 1: compose_eps against the restatement, bit for bit ----------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("shape", [(3, 4, 8, 8), (2, 3, 5, 7), (1, 1, 1, 1)])
def test_compose_eps_vs_restatement(cuda, shape, K):
    from dmx import engine
    gen = torch.Generator().manual_seed(sum(shape) + K)
    n = shape[0]
    es = [torch.randn(shape, generator=gen) for _ in range(K + 1)]
    w = torch.stack([weights(n, 10 * k + n, -3.0, 5.0) for k in range(K)])
    if n == 1:
        w[0, 0] = -1.25
    exp = compose_mix(es, w)
    out = engine.compose_eps([e.to(cuda) for e in es], w.to(cuda))
    assert out.shape == exp.shape and torch.equal(out.cpu(), exp)
    stacked = engine.compose_eps(torch.stack(es).to(cuda), w.to(cuda))       # the stacked form
    assert torch.equal(stacked.cpu(), exp)
    if K == 1:  # the tails' CFG expression
        assert torch.equal(exp, es[0] + w[0].view(-1, 1, 1, 1) * (es[1] - es[0]))
    const = engine.compose_eps([e.to(cuda) for e in es], [float(k + 1) for k in range(K)])   # (K,) weights
    assert torch.equal(const.cpu(), compose_mix(es, torch.tensor([[float(k + 1)] * n for k in range(K)])))
    with pytest.raises(ValueError):
        engine.compose_eps([e.to(cuda) for e in es], w[:, :1].expand(-1, n + 1).to(cuda))
    with pytest.raises(ValueError):
        engine.compose_eps([es[0].to(cuda)], w.to(cuda))


# ---- 2: K = 1 is the plain step -----------------------------------------------------------------------
def step_call(nm, d, cuda, kind, x, out, y, vals, mask, g, nz, hist, pos, t, **kw):
    args = (y, 0, vals, mask, g)
    if kind == "ddpm":
        nm.step(x, out, t, *args, d.coef_tables(cuda, True), nz, **kw)
    elif kind == "ddim":
        nm.step(x, out, pos, *args, None, nz, sched=d.ddim_tables(5, 0.5, cuda), **kw)
    else:
        nm.step(x, out, pos, *args, None, None, sched=d.dpm_tables(5, "uniform", cuda), hist=hist, **kw)


@pytest.mark.parametrize("B,hw", [(4, 32), (3, 28)])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_k1_is_the_plain_step(model, cuda, kind, B, hw):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    gen = torch.Generator().manual_seed(100 + hw)
    x, h0, nz = (torch.randn((B, 4, hw, hw), generator=gen).to(cuda) for _ in range(3))
    y, vals, mask, comp = compose_case(d, "k1", B, 101 + hw)
    pos = torch.full((B,), 3, dtype=torch.long, device=cuda)
    t = torch.full((B,), 600, dtype=torch.long, device=cuda)
    plain, composed = torch.empty_like(x), torch.empty_like(x)
    hp, hc = h0.clone(), h0.clone()
    step_call(nm, d, cuda, kind, x, plain, y.to(cuda), vals.to(cuda), mask.to(cuda), G, nz, hp, pos, t)
    step_call(nm, d, cuda, kind, x, composed, None, None, None, 0.0, nz, hc, pos, t, compose=to(comp, cuda))
    assert torch.isfinite(plain).all()
    assert torch.equal(plain, composed)
    assert torch.equal(hp, hc)
    # Philox noise is keyed as in the plain step
    if kind != "dpm":
        step_call(nm, d, cuda, kind, x, plain, y.to(cuda), vals.to(cuda), mask.to(cuda), G, None, hp, pos, t, seed=9,
                  sample_offset=5)
        step_call(nm, d, cuda, kind, x, composed, None, None, None, 0.0, None, hc, pos, t, seed=9, sample_offset=5,
                  compose=to(comp, cuda))
        assert torch.equal(plain, composed)


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_k1_device_loop_is_the_plain_loop(model, cuda, kind):
    """Ten steps = one launch of the 8-step graph + two of the 1-step graph."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    B = 4
    gen = torch.Generator().manual_seed(120)
    x0 = torch.randn((B, 4, 32, 32), generator=gen).to(cuda)
    y, vals, mask, comp = compose_case(d, "k1", B, 121)
    y, vals, mask, comp = y.to(cuda), vals.to(cuda), mask.to(cuda), to(comp, cuda)
    kw = {}
    if kind == "ddim":
        kw = dict(sched=d.ddim_tables(25, 0.5, cuda))
    elif kind == "dpm":
        kw = dict(sched=d.dpm_tables(25, "logsnr", cuda))
    tables = d.coef_tables(cuda, True) if kind == "ddpm" else None

    def loop(use_graph, composed):
        x, hist = x0.clone(), torch.full_like(x0, float("nan"))
        t = torch.full((1,), 25, dtype=torch.long, device=cuda)
        hk = dict(hist=hist) if kind == "dpm" else {}
        if composed:
            nm.sample_loop(x, t, None, 0, None, None, 0.0, tables, 10, seed=7, use_graph=use_graph, compose=comp,
                           **kw, **hk)
        else:
            nm.sample_loop(x, t, y, 0, vals, mask, G, tables, 10, seed=7, use_graph=use_graph, **kw, **hk)
        torch.cuda.synchronize()
        assert int(t.item()) == 15
        return x.cpu()

    plain = loop(True, False)
    assert torch.isfinite(plain).all()
    assert torch.equal(loop(True, True), plain)
    assert torch.equal(loop(False, True), plain)
    assert torch.equal(loop(False, False), plain)


# ---- 3: composed steps against the oracle ---------------------------------------------------------------
_STEP_REF = {}


def step_ref(unet_sd, d, name, B, hw):
    """Inputs and the oracle's composed eps at timestep 600 — position 3 of ddim_timesteps(5), which is
    also dpm_timesteps(5, "uniform") — once per composition and size."""
    key = (name, B, hw)
    if key not in _STEP_REF:
        gen = torch.Generator().manual_seed(400 + hw + B)
        x, hist, nz = (torch.randn((B, 4, hw, hw), generator=gen) for _ in range(3))
        _, _, _, comp = compose_case(d, name, B, 401 + hw)
        t = torch.full((B,), 600, dtype=torch.long)
        _STEP_REF[key] = (x, hist, nz, comp, t, composed_eps(unet_sd, x, t, comp))
    return _STEP_REF[key]


def composed_step_vs_oracle(nm, d, cuda, unet_sd, kind, name, B, hw):
    x, hist, nz, comp, t, eps = step_ref(unet_sd, d, name, B, hw)
    pos = torch.full((B,), 3, dtype=torch.long)
    out = torch.empty((B, 4, hw, hw), device=cuda)
    if kind == "ddpm":
        _, a, ab = ref.schedule(1000)
        exp = ref.ddpm_update(x, eps, t, a, ab, nz)
    elif kind == "ddim":
        exp = ddim_update(x, eps, pos, d.ddim_tables(5, 0.5, "cpu"), nz)
    else:
        exp, exp_h = dpm_update(x, eps, pos, d.dpm_tables(5, "uniform", "cpu"), hist)
    h = hist.to(cuda)
    step_call(nm, d, cuda, kind, x.to(cuda), out, None, None, None, 0.0, nz.to(cuda), h, pos.to(cuda), t.to(cuda),
              compose=to(comp, cuda))
    if kind == "dpm":
        assert rel(h, exp_h) <= TOL
    return rel(out, exp)


@pytest.mark.parametrize("B,hw", [(3, 32), (2, 28)])
@pytest.mark.parametrize("name", ["dropped2", "negative3"])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_composed_step_vs_oracle(model, cuda, unet_sd, kind, name, B, hw):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    comp = step_ref(unet_sd, d, name, B, hw)[3]
    assert comp[0].shape[0] == (3 if name == "dropped2" else 4)
    assert bool((comp[3] < 0).any()) and bool((comp[3] > 0).any()) and bool((comp[3] == 0).any())  # mixed sign, a zero
    err = composed_step_vs_oracle(model.native(), d, cuda, unet_sd, kind, name, B, hw)
    print(f"[composed step {kind} {name} B={B} {hw}x{hw}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TOL, err


# ---- 4: rows do not depend on the batch -------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(model, cuda):
    """B = 5 equals the shards 3 + 2 (sample_offset keeps the Philox rows), bit for bit, at K = 2."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    gen = torch.Generator().manual_seed(77)
    x = torch.randn((5, 4, 16, 16), generator=gen).to(cuda)
    _, _, _, comp = compose_case(d, "dropped2", 5, 78)
    comp = to(comp, cuda)
    pos = torch.full((5,), 4, dtype=torch.long, device=cuda)
    sched = d.ddim_tables(6, 1.0, cuda)

    def run(s, e):
        out = torch.empty_like(x[s:e])
        nm.step(x[s:e].contiguous(), out, pos[s:e], None, 0, None, None, 0.0, None, None, seed=11, sample_offset=s,
                sched=sched, compose=tuple(c[:, s:e].contiguous() for c in comp))
        return out

    whole = run(0, 5)
    parts = torch.cat([run(0, 3), run(3, 5)])
    assert torch.isfinite(whole).all()
    assert torch.equal(whole, parts)


# ---- 5: the large batch class -----------------------------------------------------------------------------
def test_large_batch_class_vs_oracle(model, cuda, unet_sd):
    """B = 32, K = 2: N = 96 rows run in the 128-sample class (Winograd), the shared prefix of 32 on the split
    implicit GEMMs (igemm_x3_kernel: a prefix of 32 samples is below igemm_halo_kernel's 256-block threshold,
    tests/golden/kernel_plan.json x3-B32-32x32)."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    err = composed_step_vs_oracle(model.native(), d, cuda, unet_sd, "ddim", "dropped2", 32, 32)
    print(f"[composed step ddim dropped2 B=32 32x32] rel-L2 vs oracle = {err:.3e}")
    assert err <= TOL, err


# ---- 6: trajectories through sample_latent_cond --------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("case,T,kw", [
    ("ddpm", 12, dict()),
    ("ddim", 1000, dict(sampler="ddim", steps=10, eta=0.5)),
    ("dpmpp_2m", 1000, dict(sampler="dpmpp_2m", steps=8)),
])
def test_composed_trajectory_vs_oracle(model, cuda, unet_sd, case, T, kw, source):
    import diff
    d = diff.Diffuser(T, device=cuda)
    d.noise_source = source
    B, hw = 3, 8
    counts = {1: 2, 3: 1}
    y = torch.tensor([1, 1, 3])
    _, vals, mask = cond(B, 600)
    _, v2, m2 = cond(B, 601)
    # the dpmpp_2m case also carries a per-sample guidance scale
    g = [2.0, -1.0, 3.5] if case == "dpmpp_2m" else G
    base = "dropped" if case != "ddim" else dict(classes=2, cond=v2 * 0.5, cond_mask=m2)
    also = [dict(classes=[2, 3, 1], cond=v2, cond_mask=m2, weight=[1.5, 0.0, -0.5])]
    comp = d._compose_args(y.tolist(), vals, mask, g, base, also, device="cpu")
    assert comp[0].shape[0] == 3  # K = 2
    mode = d._sampler_mode(kw.get("sampler", "ddpm"), kw.get("steps"), kw.get("eta", 0.0), None, T)
    tau = d._mode_timesteps(mode)
    torch.manual_seed(602)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=g,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), base=base, also=also, **kw)
    assert d.range_fallbacks == 0
    torch.manual_seed(602)
    x = torch.randn((B, 4, hw, hw))
    noisy = mode is None or mode[0] == "ddim"
    if not noisy:
        noise_of = lambda p: None  # noqa: E731
    elif source == "host":
        noise_of = lambda p: torch.randn(x.shape)  # noqa: E731  (one global draw per step, in step order)
    else:
        seed = d._seed()  # drawn after x_T, as the sampler does
        noise_of = lambda p: device_noise(d, seed, x.shape, tau[p - 1], cuda)  # noqa: E731
    x = rules.trajectory(x, *mode_tables(d, mode), lambda x, t, pos: composed_eps(unet_sd, x, t, comp), noise_of)
    err = rel(out, x)
    print(f"[composed trajectory {case} {source}] B={B} {hw}x{hw} K=2: rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err


# ---- 7: graphs ------------------------------------------------------------------------------------------------
def test_composed_device_loop_graph_eager_steps_fresh(model, model2, cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    B = 4
    gen = torch.Generator().manual_seed(700)
    x0 = torch.randn((B, 4, 32, 32), generator=gen).to(cuda)
    _, _, _, comp = compose_case(d, "dropped2", B, 701)
    comp = to(comp, cuda)
    sched = d.ddim_tables(25, 1.0, cuda)

    def loop(mdl, use_graph):
        x = x0.clone()
        t = torch.full((1,), 25, dtype=torch.long, device=cuda)
        mdl.native().sample_loop(x, t, None, 0, None, None, 0.0, None, 10, seed=7, use_graph=use_graph, sched=sched,
                                 compose=comp)
        torch.cuda.synchronize()
        assert int(t.item()) == 15
        return x.cpu()

    graph, eager, again, fresh = loop(model, True), loop(model, False), loop(model, True), loop(model2, True)
    assert torch.isfinite(graph).all()
    for other in (eager, again, fresh):
        assert torch.equal(graph, other)
    nm = model.native()
    a, b = x0.clone(), torch.empty_like(x0)
    for p in range(25, 15, -1):
        nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), None, 0, None, None, 0.0, None, None, seed=7,
                t_stride=0, sched=sched, compose=comp)
        a, b = b, a
    assert torch.equal(a.cpu(), graph)


def test_composed_and_plain_loops_keep_their_graphs(cuda, unet_sd):
    """Composed, plain, composed loops on one model, one x and one scalar capture 1, 1, 0 graph pairs."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = make_model(cuda, unet_sd).native()   # a fresh arena and empty slots
    B = 2
    gen = torch.Generator().manual_seed(710)
    x0 = torch.randn((B, 4, 16, 16), generator=gen).to(cuda)
    y, vals, mask, comp = compose_case(d, "plain2", B, 711)
    y, vals, mask, comp = y.to(cuda), vals.to(cuda), mask.to(cuda), to(comp, cuda)
    sched = d.dpm_tables(10, "logsnr", cuda)
    x, hist = torch.empty_like(x0), torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(composed, use_graph=True):
        x.copy_(x0)
        hist.fill_(float("nan"))
        t.fill_(10)
        c0 = nm.graph_captures()
        if composed:
            nm.sample_loop(x, t, None, 0, None, None, 0.0, None, 10, use_graph=use_graph, sched=sched, hist=hist,
                           compose=comp)
        else:
            nm.sample_loop(x, t, y, 0, vals, mask, G, None, 10, use_graph=use_graph, sched=sched, hist=hist)
        torch.cuda.synchronize()
        assert int(t.item()) == 0
        return x.clone(), nm.graph_captures() - c0

    want_c, _ = loop(True, use_graph=False)   # (the larger plan first: the arena will not grow below)
    want_p, _ = loop(False, use_graph=False)
    assert not torch.equal(want_c, want_p)
    for composed, captures, want in ((True, 1, want_c), (False, 1, want_p), (True, 0, want_c)):
        out, cap = loop(composed)
        assert cap == captures, (composed, cap, captures)
        assert torch.equal(out, want)


# ---- 8: known region ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
def test_known_region_with_composition(model, cuda, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    gen = torch.Generator().manual_seed(920)
    B = 2
    z0 = torch.randn((B, 4, 8, 8), generator=gen)
    m = torch.ones((B, 1, 8, 8))
    m[:, :, :, :4] = 0.0          # keep the left half
    _, vals, mask = cond(B, 921)
    _, v2, m2 = cond(B, 922)
    kw = dict(z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=G, cond=vals.to(cuda),
              cond_mask=mask.to(cuda), sampler="dpmpp_2m", steps=6, init_latent=z0.to(cuda), mask=m.to(cuda),
              strength=0.7)
    torch.manual_seed(923)
    out = d.sample_latent_cond(model, {1: 1, 3: 1}, base="dropped",
                               also=[dict(classes=2, cond=v2, cond_mask=m2, weight=[1.0, -0.5])], **kw).cpu()
    torch.manual_seed(923)
    plain = d.sample_latent_cond(model, {1: 1, 3: 1}, **kw).cpu()
    keep = (m == 0).expand_as(z0)
    assert torch.equal(out[keep], z0[keep]) and torch.equal(plain[keep], z0[keep])
    assert torch.isfinite(out).all() and not torch.equal(out, plain)


# ---- the other samplers pass the keywords through ----------------------------------------------------------------
@pytest.mark.parametrize("source,kw", [("device", dict(sampler="dpmpp_2m", steps=6)),
                                       ("host", dict(sampler="ddim", steps=5, eta=1.0))])
def test_sharded_world1_equals_diffuser(model, cuda, source, kw):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    _, vals, mask = cond(5, 900)
    _, v2, m2 = cond(5, 901)
    vals, mask = vals.to(cuda), mask.to(cuda)
    ckw = dict(guidance_scale=[3.0, 2.0, -1.0, 0.0, 4.0], base="dropped",
               also=[dict(classes=[2, 2, 3, 1, 1], cond=v2, cond_mask=m2, weight=1.5)])
    torch.manual_seed(902)
    lat = dd.ShardedCondSampler(d, model, None).sample({1: 3, 3: 2}, z_shape=(4, 8, 8), cond=vals, cond_mask=mask,
                                                       decode=False, **kw, **ckw)
    s_sharded = torch.get_rng_state()
    torch.manual_seed(902)
    single = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals,
                                  cond_mask=mask, **kw, **ckw)
    assert torch.equal(lat.cpu(), single.cpu()) and torch.isfinite(single).all()
    assert torch.equal(s_sharded, torch.get_rng_state())
    torch.manual_seed(902)
    plain = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals,
                                 cond_mask=mask, **kw)
    assert not torch.equal(plain, single)
    assert torch.equal(s_sharded, torch.get_rng_state())   # the draw order does not depend on the composition


def test_entity_csv_sampler_passes_base(model, cuda, vae_sd):
    import diff
    import numpy as np
    from conftest import GOLDEN
    from entityCsvSampler import EntityCsvSampler
    vae = make_vae(cuda, vae_sd)
    csv = os.path.join(GOLDEN, "entities.csv")
    d = diff.Diffuser(1000, device=cuda)
    s = EntityCsvSampler(d, model, vae, class_id=1, base_wh=(400, 400), device=cuda)
    kw = dict(count=2, start=1, guidance_scale=3.0, sampler="dpmpp_2m", steps=4)
    torch.manual_seed(510)
    plain = s.sample(csv, **kw)
    torch.manual_seed(510)
    same = s.sample(csv, base="null", **kw)
    torch.manual_seed(510)
    other = s.sample(csv, base="dropped", **kw)
    vals, mask = s.load_cond(csv, count=2, start=1)
    torch.manual_seed(510)
    exp = d.sample_latent_cond(model, (1, 2), vae=vae, guidance_scale=3.0, cond=vals, cond_mask=mask,
                               sampler="dpmpp_2m", steps=4, progress=False, base="dropped")
    for a, b in zip(plain, same):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(other, exp):      # the keyword passes through
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert any(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(other, plain))


# ---- 9: duck-typed model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_foreign_model_composed_step_vs_oracle(model, cuda, unet_sd, kind):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    B, hw = 2, 28
    calls = []

    class Foreign(torch.nn.Module):  # not a dmx network: no .native(); returns eps only
        def forward(self, x, t, y, cond_vals=None, cond_mask=None):
            calls.append(y.tolist())
            return model(x, t, y, cond_vals=cond_vals, cond_mask=cond_mask)[0]

    x, hist, nz, comp, t, eps = step_ref(unet_sd, d, "dropped2", B, hw)
    pos = torch.full((B,), 3, dtype=torch.long)
    d.noise_source = "host"
    torch.manual_seed(5)
    nz = torch.randn(x.shape)   # the draw the host-noise step makes
    torch.manual_seed(5)
    if kind == "ddpm":
        _, a, ab = ref.schedule(1000)
        exp = ref.ddpm_update(x, eps, t, a, ab, nz)
        plan = diff._SamplerPlan("ddpm", tables=d.coef_tables(cuda, clamp_prev=True), compose=to(comp, cuda))
        out = d._step(Foreign(), x.to(cuda), t.to(cuda), plan, True)
    elif kind == "ddim":
        exp = ddim_update(x, eps, pos, d.ddim_tables(5, 0.5, "cpu"), nz)
        plan = diff._SamplerPlan("ddim", sched=d.ddim_tables(5, 0.5, cuda), draws=True, compose=to(comp, cuda))
        out = d._step(Foreign(), x.to(cuda), pos.to(cuda), plan, True)
    else:
        exp, exp_h = dpm_update(x, eps, pos, d.dpm_tables(5, "uniform", "cpu"), hist)
        h = hist.to(cuda)
        plan = diff._SamplerPlan("dpm", sched=d.dpm_tables(5, "uniform", cuda), draws=False, compose=to(comp, cuda))
        out = d._step(Foreign(), x.to(cuda), pos.to(cuda), plan, True, hist=h)
        assert rel(h, exp_h) <= TOL
    assert calls == comp[0].tolist()    # K + 1 calls, one per branch, in branch order
    err = rel(out, exp)
    print(f"[foreign model composed step {kind}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TOL, err


# ---- 10: errors from the C entries -----------------------------------------------------------------------------------
def test_c_entries_reject_bad_compositions(model, cuda):
    """Argument checks on the host: every case returns DMX_E_ARG with a message and launches nothing."""
    import diff
    from dmx import _lib, synth
    from models.unet import Unet
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    lib = nm.lib
    B = 2
    x = torch.zeros((B, 4, 8, 8), device=cuda)
    out = torch.empty_like(x)
    t = torch.full((B,), 5, dtype=torch.long, device=cuda)
    _, _, _, comp = compose_case(d, "plain2", B, 1)
    y_rows, v_rows, m_rows, w = to(comp, cuda)
    tables = d.coef_tables(cuda, True)
    nm.ctx.ensure_time_table(1000)
    a = nm._args(x, out, t, 1, None, 0, None, None, 0.0, tables, x, 0, 0)

    def call(handle, K=2, y=y_rows, vals=v_rows, mask=m_rows, weight=w, gd=None, loop=False):
        c = _lib.Compose(K, y.data_ptr() if y is not None else None, vals.data_ptr() if vals is not None else None,
                         mask.data_ptr() if mask is not None else None, weight.data_ptr() if weight is not None else None)
        gp = ctypes.byref(gd) if gd is not None else None
        with torch.cuda.device(cuda):
            if loop:
                rc = lib.dmx_sample_loop_composed(handle, ctypes.byref(a), None, None, None, gp, ctypes.byref(c), 1, 0, None)
            else:
                rc = lib.dmx_step_composed(handle, ctypes.byref(a), None, None, None, gp, ctypes.byref(c), None)
        return rc, (lib.dmx_last_error() or b"").decode()

    um = Unet(in_ch=4)
    um.load_state_dict(synth.unet_weights(0, in_ch=4))
    unet = um.to(cuda).eval().native()
    bad = dict(K0=dict(K=0), K5=dict(K=5), null_weight=dict(weight=None), null_y=dict(y=None),
               vals_without_mask=dict(mask=None), rescale=dict(gd=_lib.Guidance(0.5)), alias=dict(weight=out))
    for loop in (False, True):
        for name, kw in bad.items():
            rc, msg = call(nm.handle, loop=loop, **kw)
            assert rc == _lib.DMX_E_ARG and msg, (name, loop, rc, msg)
        rc, msg = call(unet.handle, loop=loop)
        assert rc == _lib.DMX_E_ARG and "conditional" in msg, (loop, rc, msg)
    torch.cuda.synchronize()
    # the same struct, well-formed, runs (rescale 0 is no rescale)
    rc, msg = call(nm.handle, gd=_lib.Guidance(0.0))
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    with pytest.raises(ValueError):
        nm.step(x, out, t, None, 0, None, None, 0.0, tables, x, compose=(y_rows, v_rows, m_rows, w), rescale=0.5)
    with pytest.raises(ValueError):
        nm.step(x, out, t, None, 0, None, None, 0.0, tables, x, compose=(y_rows, v_rows, None, w))
    with pytest.raises(ValueError):
        nm.step(x, out, t, None, 0, None, None, 0.0, tables, x, compose=(y_rows, v_rows, m_rows, w[:, :1]))
    assert lib.dmx_compose_eps(x.data_ptr(), w.data_ptr(), 0, B, 4, 8, 8, out.data_ptr(), None) == _lib.DMX_E_ARG
    assert lib.dmx_compose_eps(x.data_ptr(), w.data_ptr(), 5, B, 4, 8, 8, out.data_ptr(), None) == _lib.DMX_E_ARG


# ---- 11: workspace diagnostics ------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys
import torch
sys.path[:0] = [os.path.join(ROOT, "diffusion-model_amd"), ROOT, os.path.join(ROOT, "tests")]
import diff
from dmx import synth
from models.unet_cond_geom import UnetCondWithGeomHead
dev = torch.device("cuda:0")
out = {}
g = torch.Generator().manual_seed(40)
B = 3
y_rows = torch.tensor([[0] * B, [1, 2, 3], [3, 1, 2]], device=dev)
w = torch.tensor([[3.0, -1.0, 0.0], [0.5, 2.0, -0.25]], device=dev)
for in_ch in (4, 3):   # the fused Co = 4 tail, and the three launches of Co < 4
    m = UnetCondWithGeomHead(in_ch=in_ch)
    m.load_state_dict(synth.unet_cond_geom_weights(0, in_ch=in_ch))
    m.to(dev).eval()
    d = diff.Diffuser(4, device=dev)
    tables = d.coef_tables(dev, clamp_prev=True)
    nm = m.native()
    v_rows = torch.rand((3, B, 12), generator=g).to(dev)
    m_rows = (torch.rand((3, B, 12), generator=g) > 0.3).float().to(dev)
    v_rows[0] = 0
    m_rows[0] = 0
    for hw in (16, 28):
        x = torch.randn((B, in_ch, hw, hw), generator=g).to(dev)
        noise = torch.randn((B, in_ch, hw, hw), generator=g).to(dev)
        tt = torch.full((B,), 4, dtype=torch.long, device=dev)
        o = torch.empty_like(x)
        nm.step(x, o, tt, None, 0, None, None, 0.0, tables, noise, compose=(y_rows, v_rows, m_rows, w))
        out[f"step_c{in_ch}_{hw}"] = o.cpu()
        if in_ch == 3:   # the three launches against the model's own per-branch forwards
            from dmx import engine
            es = [nm.forward(x, tt, y_rows[k], v_rows[k], m_rows[k])[0] for k in range(3)]
            out[f"ref_c{in_ch}_{hw}"] = engine.ddpm_update(x, engine.compose_eps(es, w), None, 0.0, tt, tables, noise).cpu()
torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print("[compose-worker] ok", flush=True)
'''


def test_composed_step_reads_no_unwritten_workspace(cuda, tmp_path):
    """One composed step (Co = 4 and Co = 3) in fresh processes, with and without DMX_POISON=1 /
    DMX_CHECK=1: finite and bit-identical.  The Co = 3 step (head, mix, update as three launches)
    equals the model's own per-branch forwards mixed by compose_eps within the step bound."""
    clean = run_worker(tmp_path, "clean", WORKER)
    diag = run_worker(tmp_path, "diag", WORKER, DMX_POISON="1", DMX_CHECK="1")
    bad = [k for k in clean if not torch.isfinite(diag[k]).all() or not torch.equal(clean[k], diag[k])]
    assert bad == [], bad
    for hw in (16, 28):
        err = rel(clean[f"step_c3_{hw}"], clean[f"ref_c3_{hw}"])
        print(f"[composed step Co=3 {hw}x{hw}] rel-L2 vs own forwards + compose_eps = {err:.3e}")
        assert err <= TOL, err
