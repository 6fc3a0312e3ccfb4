"""GPU: the guidance controls — CFG interval with one-forward steps, CFG rescale, and the graph slots
that let a loop alternate between step kinds — against torch-CPU restatements that take eps from the
oracle (oracle.ref.unet_cond_geom_forward) and the tables from the Diffuser.

A step at position p has the network timestep t = tau[p-1]; it uses CFG iff t_lo <= t <= t_hi, else it
is one conditional forward.  In a guided step with phi > 0:
  eg = eu + g (ec - eu) (fp32);  r[n] = 1 + phi (std(ec[n]) / std(eg[n]) - 1) (double, over C h w);
  eps = eg * fp32(r[n]);  r[n] = 1 where std(eg[n]) is not a positive finite number.
Bounds are the project's: TOL for one step, TRAJ_TOL for a trajectory.

Measured on an MI355X (rel-L2 unless said otherwise): cfg_rescale's r 0 or 1 fp32 ulp from the
restatement's on every sample; rescaled steps against the oracle 3.1e-8 (ddpm), 9.0e-7 .. 9.2e-7 (ddim),
9.5e-7 .. 9.6e-7 (dpm), the native r within 2.1e-7 .. 2.2e-7 relative of the oracle's; the unguided step
2.4e-7; trajectories (a) 4.9e-7, (b) 1.3e-6, (c) 3.2e-7 host / 2.8e-7 device, (d) 7.0e-7; foreign models
6.8e-7 (dpm), 6.3e-7 (ddim), 1.8e-7 (ddpm)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref, rules
from oracle.rules import cfg_rescale, ddim_update, dpm_update, rel
from support import cond, device_noise, make_model, make_vae, mode_tables, overflow_sd, ulps

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


@pytest.fixture(scope="module")
def vae(cuda, vae_sd):
    return make_vae(cuda, vae_sd)


@pytest.fixture
def unet_sd_overflow():
    return overflow_sd()


def interval_trajectory(sd, d, mode, x, y, vals, mask, interval, phi, noise_of):
    """rules.trajectory over the mode's schedule, a step guided iff its timestep lies in `interval`."""
    def eps_of(x, t, pos):
        guided = interval is None or interval[0] <= int(t[0]) <= interval[1]
        return rules.guided_eps(sd, x, t, y, vals, mask, guided, phi)[0]
    return rules.trajectory(x, *mode_tables(d, mode), eps_of, noise_of)


# ---- 1: cfg_rescale against the restatement ------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 8, 8), (3, 4, 28, 28), (3, 3, 5, 7)])
def test_cfg_rescale_vs_restatement(cuda, shape):
    from dmx import engine
    gen = torch.Generator().manual_seed(sum(shape))
    B5 = (5,) + shape[1:]
    eu, ec = (torch.randn(B5, generator=gen) for _ in range(2))
    ec[1] = 0.375   # a constant conditional prediction ...
    eu[1] = -1.25   # ... and unconditional one: eg is constant, std 0 after guidance
    phi = 0.7
    eg, r_ref = cfg_rescale(eu, ec, G, phi)
    eps, r = engine.cfg_rescale(eu.to(cuda), ec.to(cuda), G, phi)
    eps, r = eps.cpu(), r.cpu()
    n = shape[0]
    d_ulp = ulps(r, r_ref.float())
    print(f"[cfg_rescale {shape}] r = {r.tolist()}, ulps from fp32(r_ref) = {d_ulp.tolist()}")
    assert int(d_ulp.max()) <= 1
    assert float(r[1]) == 1.0 and float(r_ref[1]) == 1.0
    assert torch.equal(eps, eg * r.view(-1, 1, 1, 1))            # eps = fp32(eg * r_gpu), bit for bit
    eps2, r2 = engine.cfg_rescale(eu.to(cuda), ec.to(cuda), G, phi)
    assert torch.equal(eps2.cpu(), eps) and torch.equal(r2.cpu(), r)   # two runs
    ea, ra = engine.cfg_rescale(eu[:n].to(cuda), ec[:n].to(cuda), G, phi)   # rows of 5 = rows of 3 + 2
    eb, rb = engine.cfg_rescale(eu[n:].to(cuda), ec[n:].to(cuda), G, phi)
    assert torch.equal(torch.cat([ea, eb]).cpu(), eps) and torch.equal(torch.cat([ra, rb]).cpu(), r)
    e0, r0 = engine.cfg_rescale(eu.to(cuda), ec.to(cuda), G, 0.0)            # phi = 0 returns eg
    assert torch.equal(e0.cpu(), eg) and bool((r0 == 1).all())
    e1, r1 = engine.cfg_rescale(eu.to(cuda), ec.to(cuda), G, 1.0)            # phi = 1: std(eps) = std(ec)
    s1, sc = e1.double().flatten(1).std(1).cpu(), ec.double().flatten(1).std(1)
    keep = torch.tensor([i != 1 for i in range(5)])
    assert float(((s1 - sc).abs() / sc)[keep].max()) <= 1e-6
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            engine.cfg_rescale(eu.to(cuda), ec.to(cuda), G, bad)
    with pytest.raises(ValueError):
        engine.cfg_rescale(eu.to(cuda), ec[:2].to(cuda), G, phi)


# ---- 2: one native step with phi = 0.7 -------------------------------------------------------------
_STEP_REF = {}


def step_ref(unet_sd, B, hw):
    """Inputs and the oracle's eu / ec at timestep 600 — position 3 of ddim_timesteps(5), which is also
    dpm_timesteps(5, "uniform") — once per size."""
    if (B, hw) not in _STEP_REF:
        gen = torch.Generator().manual_seed(400 + hw)
        x, hist, nz = (torch.randn((B, 4, hw, hw), generator=gen) for _ in range(3))
        y, vals, mask = cond(B, 401 + hw)
        t = torch.full((B,), 600, dtype=torch.long)
        with torch.no_grad():
            eu, _ = ref.unet_cond_geom_forward(unet_sd, x, t, torch.zeros_like(y), vals, mask)
            ec, _ = ref.unet_cond_geom_forward(unet_sd, x, t, y, vals, mask)
        _STEP_REF[B, hw] = (x, hist, nz, y, vals, mask, t, eu, ec)
    return _STEP_REF[B, hw]


@pytest.mark.parametrize("B,hw", [(2, 8), (3, 28)])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_rescaled_step_vs_oracle(model, cuda, unet_sd, kind, B, hw):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    phi = 0.7
    x, hist, nz, y, vals, mask, t, eu, ec = step_ref(unet_sd, B, hw)
    eg, r_ref = cfg_rescale(eu, ec, G, phi)
    eps = eg * r_ref.float().view(-1, 1, 1, 1)
    pos = torch.full((B,), 3, dtype=torch.long)
    out = torch.empty((B, 4, hw, hw), device=cuda)
    args = (y.to(cuda), 0, vals.to(cuda), mask.to(cuda), G)
    if kind == "ddpm":
        _, a, ab = ref.schedule(1000)
        exp = ref.ddpm_update(x, eps, t, a, ab, nz)
        nm.step(x.to(cuda), out, t.to(cuda), *args, d.coef_tables(cuda, True), nz.to(cuda), rescale=phi)
    elif kind == "ddim":
        exp = ddim_update(x, eps, pos, d.ddim_tables(5, 0.5, "cpu"), nz)
        nm.step(x.to(cuda), out, pos.to(cuda), *args, None, nz.to(cuda), sched=d.ddim_tables(5, 0.5, cuda), rescale=phi)
    else:
        exp, exp_h = dpm_update(x, eps, pos, d.dpm_tables(5, "uniform", "cpu"), hist)
        h = hist.to(cuda)
        nm.step(x.to(cuda), out, pos.to(cuda), *args, None, None, sched=d.dpm_tables(5, "uniform", cuda), hist=h,
                rescale=phi)
        assert rel(h, exp_h) <= TOL
    err = rel(out, exp)
    # the native step's ratio, re-derived from the network's own two predictions
    e2, _ = nm.forward(torch.cat([x, x]).to(cuda), torch.cat([t, t]).to(cuda), torch.cat([torch.zeros_like(y), y]).to(cuda),
                       torch.cat([vals, vals]).to(cuda), torch.cat([mask, mask]).to(cuda))
    _, r = engine.cfg_rescale(e2[:B], e2[B:], G, phi)
    r_err = float(((r.cpu().double() - r_ref) / r_ref).abs().max())
    print(f"[rescaled step {kind} B={B} {hw}x{hw}] rel-L2 vs oracle = {err:.3e}; r = {r.cpu().tolist()}, "
          f"max rel error of r = {r_err:.3e}")
    assert err <= TOL, err
    assert r_err <= 1e-5, r_err
    # the step is deterministic and phi = 0 is the plain step
    out2 = torch.empty_like(out)
    if kind == "ddpm":
        nm.step(x.to(cuda), out2, t.to(cuda), *args, d.coef_tables(cuda, True), nz.to(cuda), rescale=phi)
        assert torch.equal(out2, out)
        plain, zero = torch.empty_like(out), torch.empty_like(out)
        nm.step(x.to(cuda), plain, t.to(cuda), *args, d.coef_tables(cuda, True), nz.to(cuda))
        nm.step(x.to(cuda), zero, t.to(cuda), *args, d.coef_tables(cuda, True), nz.to(cuda), rescale=0.0)
        assert torch.equal(plain, zero) and not torch.equal(plain, out)


def test_rescaled_step_rows_do_not_depend_on_the_batch(model, cuda):
    """B = 5 equals 3 + 2, bit for bit: the per-sample moments see that sample alone (batches below the
    64-sample class, whose conv plans do not depend on the batch either)."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    gen = torch.Generator().manual_seed(77)
    x = torch.randn((5, 4, 16, 16), generator=gen).to(cuda)
    y, vals, mask = (v.to(cuda) for v in cond(5, 78))
    pos = torch.full((5,), 4, dtype=torch.long, device=cuda)
    sched = d.ddim_tables(6, 0.0, cuda)

    def run(s):
        out = torch.empty_like(x[s])
        nm.step(x[s].contiguous(), out, pos[s], y[s], 0, vals[s], mask[s], G, None, None, sched=sched, rescale=0.5)
        return out

    whole = run(slice(0, 5))
    parts = torch.cat([run(slice(0, 3)), run(slice(3, 5))])
    plain = torch.empty_like(x)
    nm.step(x, plain, pos, y, 0, vals, mask, G, None, None, sched=sched)
    plain_parts = torch.empty_like(x[:3])
    nm.step(x[:3].contiguous(), plain_parts, pos[:3], y[:3], 0, vals[:3], mask[:3], G, None, None, sched=sched)
    if torch.equal(plain[:3], plain_parts):  # the network itself is batch-independent at these sizes
        assert torch.equal(whole, parts)
    else:
        assert rel(whole, parts) <= TOL
    assert torch.isfinite(whole).all()


def test_rescale_without_cfg_is_an_error(model, cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    x = torch.zeros((2, 4, 8, 8), device=cuda)
    y, vals, mask = (v.to(cuda) for v in cond(2, 1))
    t = torch.full((2,), 5, device=cuda)
    for g, yy in ((0.0, y), (G, None)):
        with pytest.raises(ValueError):
            nm.step(x, torch.empty_like(x), t, yy, 0, vals, mask, g, d.coef_tables(cuda, True), x, rescale=0.5)
    with pytest.raises(ValueError):
        nm.step(x, torch.empty_like(x), t, y, 0, vals, mask, G, d.coef_tables(cuda, True), x, rescale=1.5)


# ---- 3: defaults untouched -------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("sampler", ["diffuser", "sharded"])
def test_defaults_reproduce_the_plain_calls(model, cuda, source, sampler):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    nm = model.native()
    _, vals, mask = cond(3, 500)
    kw = dict(cond=vals.to(cuda), cond_mask=mask.to(cuda), sampler="ddim", steps=4, eta=1.0)

    def run(**extra):
        torch.manual_seed(501)
        c0 = nm.graph_captures()
        if sampler == "diffuser":
            out = d.sample_latent_cond(model, {1: 2, 3: 1}, z_shape=(4, 8, 8), vae=None, progress=False, **kw, **extra)
        else:
            out = dd.ShardedCondSampler(d, model, None).sample({1: 2, 3: 1}, z_shape=(4, 8, 8), decode=False, **kw,
                                                               **extra)
        return out.cpu(), torch.get_rng_state(), nm.graph_captures() - c0

    most = 1 if source == "device" else 0   # one loop of one kind of step: at most one graph pair
    plain, rng, cap = run()
    assert cap <= most
    for extra in (dict(guidance_interval=(1, 1000)), dict(guidance_rescale=0.0),
                  dict(guidance_interval=(1, 1000), guidance_rescale=0.0), dict(guidance_interval=(200, 1000))):
        out, rng2, cap2 = run(**extra)   # (200, 1000) holds every timestep of ddim_timesteps(4) too
        assert torch.equal(out, plain) and torch.equal(rng2, rng), extra
        assert cap2 <= most, (extra, cap2)   # no extra capture


@pytest.mark.parametrize("source", ["host", "device"])
def test_defaults_reproduce_the_plain_calls_entity_csv(model, vae, cuda, source):
    import diff
    from conftest import GOLDEN
    from entityCsvSampler import EntityCsvSampler
    csv = os.path.join(GOLDEN, "entities.csv")
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    s = EntityCsvSampler(d, model, vae, class_id=1, base_wh=(400, 400), device=cuda)
    kw = dict(count=2, start=1, guidance_scale=3.0, sampler="dpmpp_2m", steps=4)
    torch.manual_seed(510)
    plain = s.sample(csv, **kw)
    torch.manual_seed(510)
    same = s.sample(csv, guidance_interval=(1, 1000), guidance_rescale=0.0, **kw)
    torch.manual_seed(510)
    other = s.sample(csv, guidance_interval=(300, 700), guidance_rescale=0.5, **kw)
    vals, mask = s.load_cond(csv, count=2, start=1)
    torch.manual_seed(510)
    exp = d.sample_latent_cond(model, (1, 2), vae=vae, guidance_scale=3.0, cond=vals, cond_mask=mask,
                               sampler="dpmpp_2m", steps=4, progress=False, guidance_interval=(300, 700),
                               guidance_rescale=0.5)
    for a, b in zip(plain, same):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(other, exp):      # the keywords pass through
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert any(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(other, plain))


# ---- 4: the unguided device loop ---------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 64])
def test_unguided_device_loop(model, model2, cuda, unet_sd, B):
    """guidance 0 with y given: one conditional forward per step.  Ten steps = one launch of the 8-step
    graph + two of the 1-step graph."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    gen = torch.Generator().manual_seed(20 + B)
    x0c = torch.randn((B, 4, 32, 32), generator=gen)
    x0 = x0c.to(cuda)
    yc, valsc, maskc = cond(B, 21 + B)
    y, vals, mask = yc.to(cuda), valsc.to(cuda), maskc.to(cuda)
    sched = d.dpm_tables(25, "logsnr", cuda)

    def loop(mdl, use_graph):
        x, hist = x0.clone(), torch.full_like(x0, float("nan"))
        t = torch.full((1,), 25, dtype=torch.long, device=cuda)
        mdl.native().sample_loop(x, t, y, 0, vals, mask, 0.0, None, 10, seed=7, use_graph=use_graph, sched=sched,
                                 hist=hist)
        torch.cuda.synchronize()
        assert int(t.item()) == 15
        return x.cpu(), hist.cpu()

    graph, eager, again, fresh = loop(model, True), loop(model, False), loop(model, True), loop(model2, True)
    for other in (eager, again, fresh):
        assert torch.equal(graph[0], other[0]) and torch.equal(graph[1], other[1])
    assert torch.isfinite(graph[0]).all()
    nm = model.native()
    a, b, h = x0.clone(), torch.empty_like(x0), torch.full_like(x0, float("nan"))
    first = None
    for p in range(25, 15, -1):
        nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), y, 0, vals, mask, 0.0, None, t_stride=0,
                sched=sched, hist=h)
        a, b = b, a
        first = a.clone() if first is None else first
    assert torch.equal(a.cpu(), graph[0]) and torch.equal(h.cpu(), graph[1])
    if B == 4:  # one position against the oracle's conditional forward + update
        cs = d.dpm_tables(25, "logsnr", "cpu")
        pos = torch.full((B,), 25, dtype=torch.long)
        with torch.no_grad():
            ec, _ = ref.unet_cond_geom_forward(unet_sd, x0c, cs[0][pos - 1], yc, valsc, maskc)
        exp, _ = dpm_update(x0c, ec, pos, cs, torch.zeros_like(x0c))
        err = rel(first, exp)
        print(f"[unguided step B={B}] rel-L2 vs oracle = {err:.3e}")
        assert err <= TOL, err


# ---- 5: interval trajectories against the oracle -------------------------------------------------------
@pytest.mark.parametrize("case,T,kw,ipos,phi,B,hw,source", [
    ("a", 1000, dict(sampler="dpmpp_2m", steps=6), (2, 4), 0.0, 2, 8, "device"),
    ("b", 1000, dict(sampler="ddim", steps=5, eta=1.0), (4, 5), 0.0, 2, 8, "host"),
    ("c-host", 12, dict(), (4, 9), 0.0, 2, 8, "host"),
    ("c-device", 12, dict(), (4, 9), 0.0, 2, 8, "device"),
    # the CFG batch of 64 takes the Winograd path, the unguided batch of 32 the halo path
    ("d", 1000, dict(sampler="dpmpp_2m", steps=4), (2, 3), 0.5, 32, 32, "device"),
])
def test_interval_trajectory_vs_oracle(model, cuda, unet_sd, case, T, kw, ipos, phi, B, hw, source):
    import diff
    d = diff.Diffuser(T, device=cuda)
    d.noise_source = source
    mode = d._sampler_mode(kw.get("sampler", "ddpm"), kw.get("steps"), kw.get("eta", 0.0), None, T)
    tau = d._mode_timesteps(mode)
    interval = (tau[ipos[0] - 1], tau[ipos[1] - 1])   # covers positions ipos[0] .. ipos[1]
    assert d._guided_run(tau, interval) == ipos
    y, vals, mask = cond(B, 600 + B)
    counts = {c: int((y == c).sum()) for c in (1, 2, 3) if int((y == c).sum())}
    y = torch.tensor([c for c, n in counts.items() for _ in range(n)])
    extra = dict(guidance_rescale=phi) if phi > 0 else {}
    torch.manual_seed(601)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=G,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), guidance_interval=interval, **kw, **extra)
    assert d.range_fallbacks == 0
    torch.manual_seed(601)
    x_T = torch.randn((B, 4, hw, hw))
    noisy = mode is None or (mode[0] == "ddim" and mode[2] > 0)
    if not noisy:
        noise_of = lambda p: None  # noqa: E731
    elif source == "host":
        noise_of = lambda p: torch.randn(x_T.shape)  # noqa: E731  (one global draw per step, in step order)
    else:
        seed = d._seed()  # drawn after x_T, as the sampler does
        noise_of = lambda p: device_noise(d, seed, x_T.shape, tau[p - 1], cuda)  # noqa: E731
    exp = interval_trajectory(unet_sd, d, mode, x_T, y, vals, mask, interval, phi, noise_of)
    err = rel(out, exp)
    print(f"[interval trajectory {case}] B={B} {hw}x{hw} interval={interval} phi={phi} {source}: "
          f"rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err


@pytest.mark.parametrize("source", ["host", "device"])
def test_empty_interval_is_a_loop_of_unguided_steps(model, cuda, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    S = 5
    assert d._guided_run(d.dpm_timesteps(S, "uniform"), (401, 599)) is None
    y, vals, mask = (v.to(cuda) for v in cond(3, 610))
    torch.manual_seed(611)
    out = d.sample_latent_cond(model, {1: 1, 2: 1, 3: 1}, z_shape=(4, 8, 8), vae=None, progress=False,
                               guidance_scale=G, cond=vals, cond_mask=mask, sampler="dpmpp_2m", steps=S,
                               spacing="uniform", guidance_interval=(401, 599))
    state = torch.get_rng_state()
    torch.manual_seed(611)
    x = torch.randn((3, 4, 8, 8)).to(cuda)
    assert torch.equal(torch.get_rng_state(), state)  # x_T and nothing else
    hist = torch.empty_like(x)
    for p in range(S, 0, -1):
        x = d.dpm_step(model, x, torch.full((3,), p, device=cuda), hist, S, "uniform", y=y, guidance_scale=0.0,
                       cond_vals=vals, cond_mask=mask)
    assert torch.equal(out, x)


# ---- 6: graph slots ------------------------------------------------------------------------------------
def test_graph_slots(cuda, unet_sd, model2):
    """One model, one x, one position scalar: loops of different kinds keep their captured graphs."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = make_model(cuda, unet_sd).native()   # a fresh arena and empty slots
    ref_nm = model2.native()                  # the same calls without graphs
    gen = torch.Generator().manual_seed(700)
    B = 2
    x0 = torch.randn((B, 4, 16, 16), generator=gen).to(cuda)
    y, vals, mask = (v.to(cuda) for v in cond(B, 701))
    sched = d.dpm_tables(10, "logsnr", cuda)
    x, hist = torch.empty_like(x0), torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(n, g, phi=0.0, use_graph=True):
        x.copy_(x0)
        hist.fill_(float("nan"))
        t.fill_(10)
        c0 = nm.graph_captures()
        kw = dict(rescale=phi) if phi > 0 else {}
        n.sample_loop(x, t, y, 0, vals, mask, g, None, 10, use_graph=use_graph, sched=sched, hist=hist, **kw)
        torch.cuda.synchronize()
        assert int(t.item()) == 0
        return x.clone(), nm.graph_captures() - c0

    kinds = {"guided": (G, 0.0), "unguided": (0.0, 0.0), "rescaled": (G, 0.5), "rescaled25": (G, 0.25),
             "guided2": (2.0, 0.0)}
    want = {k: loop(ref_nm, *v, use_graph=False)[0] for k, v in kinds.items()}
    assert len({tuple(v.flatten().tolist()) for v in want.values()}) == len(want)  # five different results

    def check(kind, captures):
        out, cap = loop(nm, *kinds[kind])
        assert cap == captures, (kind, cap, captures)
        assert torch.equal(out, want[kind]), kind
        eager, cap = loop(nm, *kinds[kind], use_graph=False)
        assert cap == 0 and torch.equal(eager, want[kind]), kind

    loop(nm, G, 0.5, use_graph=False)  # the largest plan of this shape: the arena will not grow below
    c0 = nm.graph_captures()
    for kind, captures in (("guided", 1), ("unguided", 1), ("guided", 0), ("rescaled", 1)):
        check(kind, captures)
    assert nm.graph_captures() - c0 == 3
    # another precision and back: every slot was dropped, the results are not changed
    before = nm.graph_captures()
    nm.set_precision("fp32")
    nm.set_precision("x3")
    check("guided", 1)
    check("unguided", 1)
    assert nm.graph_captures() > before
    # a larger batch grows the arena under the slots: they are dropped, not replayed on freed memory
    xb = torch.randn((8, 4, 32, 32), generator=gen).to(cuda)
    yb, vb, mb = (v.to(cuda) for v in cond(8, 702))
    tb = torch.full((1,), 10, dtype=torch.long, device=cuda)
    ws0 = nm.workspace_bytes()
    nm.sample_loop(xb, tb, yb, 0, vb, mb, G, None, 2, use_graph=True, sched=sched, hist=torch.empty_like(xb))
    torch.cuda.synchronize()
    assert nm.workspace_bytes() > ws0 and torch.isfinite(xb).all()
    check("guided", 1)
    check("unguided", 1)
    check("rescaled", 1)
    check("rescaled25", 1)    # four slots live
    check("guided", 0)
    check("unguided", 0)
    check("rescaled", 0)
    check("rescaled25", 0)
    check("guided2", 1)       # a fifth key: the least recently used slot (guided) goes
    check("rescaled25", 0)
    check("guided", 1)        # evicted above, captured again (unguided goes)
    check("rescaled", 0)
    check("guided2", 0)


# ---- 7: range guard ------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
def test_range_guard_replays_chunks_with_their_segments(cuda, unet_sd_overflow, source):
    import diff
    m = make_model(cuda, unet_sd_overflow)
    _, vals, mask = cond(2, 800)
    S = 9
    tau = diff.Diffuser(1000).dpm_timesteps(S)
    interval = (tau[4], tau[7])  # positions 5..8: boundaries inside the chunks 9..7 and 6..4

    def run():
        d = diff.Diffuser(1000, device=cuda)
        d.noise_source = source
        d.GUARD_CHUNK = 3
        assert d._guidance_segments(9, 6, d._guided_run(tau, interval)) == [(9, 8, False), (8, 6, True)]
        assert d._guidance_segments(6, 3, d._guided_run(tau, interval)) == [(6, 4, True), (4, 3, False)]
        torch.manual_seed(801)
        lat = d.sample_latent_cond(m, {1: 1, 2: 1}, z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=G,
                                   cond=vals.to(cuda), cond_mask=mask.to(cuda), sampler="dpmpp_2m", steps=S,
                                   guidance_interval=interval, guidance_rescale=0.5)
        return d, lat

    d, lat = run()
    assert d.range_fallbacks == 3   # every chunk
    assert torch.isfinite(lat).all() and m.native().precision == "x3"
    with m.native().precision_override("fp32"):
        d32, lat32 = run()
    assert d32.range_fallbacks == 0
    assert torch.equal(lat, lat32)


# ---- 8: public paths -----------------------------------------------------------------------------------
@pytest.mark.parametrize("source,kw", [
    ("device", dict(sampler="dpmpp_2m", steps=6, guidance_interval=(150, 800), guidance_rescale=0.5)),
    ("host", dict(sampler="ddim", steps=5, eta=1.0, guidance_interval=(400, 1000), guidance_rescale=0.7)),
])
def test_sharded_world1_equals_diffuser(model, cuda, source, kw):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    _, vals, mask = cond(5, 900)
    vals, mask = vals.to(cuda), mask.to(cuda)
    torch.manual_seed(901)
    lat = dd.ShardedCondSampler(d, model, None).sample({1: 3, 3: 2}, z_shape=(4, 8, 8), cond=vals, cond_mask=mask,
                                                       decode=False, **kw)
    s_sharded = torch.get_rng_state()
    torch.manual_seed(901)
    single = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals,
                                  cond_mask=mask, **kw)
    assert torch.equal(lat.cpu(), single.cpu()) and torch.isfinite(single).all()
    assert torch.equal(s_sharded, torch.get_rng_state())
    torch.manual_seed(901)
    plain = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals,
                                 cond_mask=mask, **{k: v for k, v in kw.items() if not k.startswith("guidance_")})
    assert not torch.equal(plain, single)
    assert torch.equal(s_sharded, torch.get_rng_state())   # the draw order does not depend on the step kinds


@pytest.mark.parametrize("name,kw", [("dpm", dict(sampler="dpmpp_2m", steps=4)),
                                     ("ddim", dict(sampler="ddim", steps=4, eta=0.0)), ("ddpm", dict())])
def test_foreign_model_interval_and_rescale(model, cuda, unet_sd, name, kw):
    import diff
    T = 6 if name == "ddpm" else 1000
    d = diff.Diffuser(T, device=cuda)
    mode = d._sampler_mode(kw.get("sampler", "ddpm"), kw.get("steps"), kw.get("eta", 0.0), None, T)
    tau = d._mode_timesteps(mode)
    interval = (tau[1], tau[2])
    phi = 0.5
    calls = []

    class Foreign(torch.nn.Module):  # not a dmx network: no .native()
        def forward(self, x, t, y, cond_vals=None, cond_mask=None):
            calls.append(int(y[0]))
            return model(x, t, y, cond_vals=cond_vals, cond_mask=cond_mask)

    y, vals, mask = cond(2, 910)
    y = torch.tensor([2, 2])
    torch.manual_seed(911)
    out = d.sample_latent_cond(Foreign(), {2: 2}, z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=G,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), guidance_interval=interval,
                               guidance_rescale=phi, **kw)
    S = len(tau)
    assert len(calls) == S + 2          # one call per unguided step, two per guided one
    assert calls.count(0) == 2          # the null label only inside the interval
    torch.manual_seed(911)
    x_T = torch.randn((2, 4, 8, 8))
    noise_of = (lambda p: torch.randn(x_T.shape)) if mode is None else (lambda p: torch.zeros_like(x_T))
    exp = interval_trajectory(unet_sd, d, mode, x_T, y, vals, mask, interval, phi, noise_of)
    err = rel(out, exp)
    print(f"[foreign model {name}, interval + rescale] rel-L2 vs restatement = {err:.3e}")
    assert err <= TRAJ_TOL, err


@pytest.mark.parametrize("source", ["host", "device"])
def test_known_region_with_both_keywords(model, cuda, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    gen = torch.Generator().manual_seed(920)
    B = 2
    z0 = torch.randn((B, 4, 8, 8), generator=gen)
    m = torch.ones((B, 1, 8, 8))
    m[:, :, :, :4] = 0.0          # keep the left half
    _, vals, mask = cond(B, 921)
    kw = dict(z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=G, cond=vals.to(cuda),
              cond_mask=mask.to(cuda), sampler="dpmpp_2m", steps=6, init_latent=z0.to(cuda), mask=m.to(cuda),
              strength=0.7)
    torch.manual_seed(922)
    out = d.sample_latent_cond(model, {1: 1, 3: 1}, guidance_interval=(150, 800), guidance_rescale=0.5, **kw).cpu()
    torch.manual_seed(922)
    plain = d.sample_latent_cond(model, {1: 1, 3: 1}, **kw).cpu()
    keep = (m == 0).expand_as(z0)
    assert torch.equal(out[keep], z0[keep]) and torch.equal(plain[keep], z0[keep])
    assert torch.isfinite(out).all() and not torch.equal(out[~keep], plain[~keep])
