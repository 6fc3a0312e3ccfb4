"""GPU: perturbed-attention guidance — one more branch per step whose self-attention is replaced by the
identity in chosen blocks, mixed as eps = e_u + g (e_c - e_u) + s (e_c - e_p) by the composed tail.

The oracle is oracle.ref.unet_cond_geom_forward, once per branch; for a perturbed branch ref.attention
is replaced, for the duration of the call, by a restatement that sets a = qkv[..., 2c:] (softmax = I) in
the named blocks and calls the original otherwise.  Bounds are the project's: TOL for one forward or
step, TRAJ_TOL for a trajectory, TOL_FWD in f16 mode.

Measured on an MI355X (rel-L2): perturbed forward rows against the patched oracle 1.3e-6 .. 1.9e-6 (x3 and
fp32), 1.04e-3 (f16); the perturbation itself moves eps by 0.080 (sa3) .. 0.47 (all six); PAG steps 6.7e-8 ..
7.2e-8 (ddpm), 2.1e-6 .. 3.0e-6 (ddim, dpm); B = 22 with three branches 2.6e-6; trajectories 5.7e-7 .. 2.0e-6;
the bit-equalities hold."""
import ctypes
import os

import pytest
import torch

from oracle import ref, rules
from oracle.rules import ALL6, composed_eps, ddim_update, dpm_update, perturbed_forward, rel
from support import cond, device_noise, make_model, make_vae, mode_tables, run_worker

pytestmark = pytest.mark.gpu

TOL = 2e-5        # one forward or step (the project's step bound)
TRAJ_TOL = 1e-4   # a trajectory (the project's trajectory bound)
TOL_FWD = 2e-3    # one forward in f16 mode (the project's config-4 bound)
G = 3.0
S = 3.0


def bits(names):
    return sum(1 << ALL6.index(n) for n in names)


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    return make_model(cuda, unet_sd)


@pytest.fixture(scope="module")
def model2(cuda, unet_sd):
    """A second network with the same weights: its own arena and its own graph slots."""
    return make_model(cuda, unet_sd)


def to(comp, dev):
    return tuple(c.to(dev).contiguous() for c in comp)


def pag_case(d, name, B, seed):
    """The tables of a named PAG call on the CPU, built by the sampler's own _compose_args / _pag_args:
    (branch tables, (blocks, branches))."""
    y, vals, mask = cond(B, seed)
    _, v2, m2 = cond(B, seed + 1)
    if name == "pag33":          # CFG + PAG, both scales 3, the default block
        return d._pag_args(S, ("sa3",), y.tolist(), vals, mask, G)
    if name == "all6":
        return d._pag_args(S, ALL6, y.tolist(), vals, mask, G)
    if name == "persample":      # a per-sample scale with a zero
        s = [0.0 if i == 1 else 1.0 + 0.5 * i for i in range(B)]
        return d._pag_args(s, ("sa2", "sa5"), y.tolist(), vals, mask, G)
    if name == "dropped_also":   # over the true unconditional base, with one more condition
        also = [dict(classes=[1 + (i + 1) % 3 for i in range(B)], cond=v2, cond_mask=m2, weight=1.5)]
        comp = d._compose_args(y.tolist(), vals, mask, G, "dropped", also)
        return d._pag_args(2.0, ("sa1", "sa6"), y.tolist(), vals, mask, G, comp)
    if name == "g0":             # no CFG: K = 1 over the main condition
        return d._pag_args(S, ("sa3", "sa4"), y.tolist(), vals, mask, 0.0)
    if name == "sa13":
        return d._pag_args(S, ("sa1", "sa3"), y.tolist(), vals, mask, G)
    raise KeyError(name)


# ---- 1: the identity kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("L", [9, 49, 1024])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_attn_identity_is_v_bit_for_bit(cuda, C, L, n):
    from dmx import engine
    gen = torch.Generator().manual_seed(C + L + n)
    qkv = torch.randn((n, L, 3 * C), generator=gen)
    qkv[0, 0, 2 * C] = float("inf")      # a copy: specials pass through
    qkv[-1, -1, -1] = -0.0
    out = engine.attn_identity(qkv.to(cuda), C)
    assert out.shape == (n, L, C)
    exp = qkv[..., 2 * C:].contiguous()
    assert torch.equal(out.cpu().view(torch.int32), exp.view(torch.int32))
    with pytest.raises(ValueError):
        engine.attn_identity(qkv.to(cuda), 32)
    with pytest.raises(ValueError):
        engine.attn_identity(qkv[..., :-4].to(cuda), C)


# ---- 2: the forward with perturbed rows ----------------------------------------------------------------------
_FWD_REF = {}


def fwd_inputs(hw):
    B = 2
    gen = torch.Generator().manual_seed(200 + hw)
    x = torch.randn((2 * B, 4, hw, hw), generator=gen)
    t = torch.full((2 * B,), 500, dtype=torch.long)
    y, vals, mask = cond(2 * B, 201 + hw)
    return B, x, t, y, vals, mask


def fwd_ref(sd, hw, names):
    """The oracle's eps of rows [B, 2B), perturbed in `names` (() = unperturbed), once per size and set."""
    key = (hw, tuple(names))
    if key not in _FWD_REF:
        B, x, t, y, vals, mask = fwd_inputs(hw)
        _FWD_REF[key] = perturbed_forward(sd, x[B:], t[B:], y[B:], vals[B:], mask[B:], names)
    return _FWD_REF[key]


FWD_CASES = [(hw, names, prec, TOL) for hw in (32, 28) for names in (("sa3",), ("sa6",), ALL6)
             for prec in ("x3", "fp32")] + [(32, ALL6, "f16", TOL_FWD)]


@pytest.mark.parametrize("hw,names,prec,tol", FWD_CASES)
def test_forward_perturbed_rows(model, cuda, unet_sd, hw, names, prec, tol):
    nm = model.native()
    B, x, t, y, vals, mask = fwd_inputs(hw)
    args = (x.to(cuda), t.to(cuda), y.to(cuda), vals.to(cuda), mask.to(cuda))
    with nm.precision_override(prec):
        plain, _ = nm.forward(*args)
        pert, _ = nm.forward(*args, perturb=(bits(names), B, 2 * B))
    assert torch.isfinite(pert).all()
    assert torch.equal(pert[:B], plain[:B])               # the sub-range guarantee
    exp, unperturbed = fwd_ref(unet_sd, hw, names), fwd_ref(unet_sd, hw, ())
    moved = rel(exp, unperturbed)
    err = rel(pert[B:], exp)
    print(f"[forward {prec} {hw}x{hw} {'+'.join(names)}] rel-L2 vs patched oracle = {err:.3e}; "
          f"the perturbation moves eps by {moved:.3e}")
    assert moved > 1e-2, moved                           # the test cannot pass on an unperturbed network
    assert err <= tol, err
    # the first rows perturbed instead: the trailing rows keep their bits
    with nm.precision_override(prec):
        head, _ = nm.forward(*args, perturb=(bits(names), 0, B))
    assert torch.equal(head[B:], plain[B:]) and not torch.equal(head[:B], plain[:B])


def test_forward_rejects_bad_perturb(model, cuda):
    nm = model.native()
    _, x, t, y, vals, mask = fwd_inputs(32)
    args = (x.to(cuda), t.to(cuda), y.to(cuda), vals.to(cuda), mask.to(cuda))
    for bad in ((0, 0, 2), (64, 0, 2), (4, 2, 2), (4, -1, 2), (4, 0, 5)):
        with pytest.raises(ValueError):
            nm.forward(*args, perturb=bad)


# ---- 3: unperturbed branches keep their bits --------------------------------------------------------------------
def step_call(nm, d, cuda, kind, x, out, nz, hist, pos, t, **kw):
    args = (None, 0, None, None, 0.0)
    if kind == "ddpm":
        nm.step(x, out, t, *args, d.coef_tables(cuda, True), nz, **kw)
    elif kind == "ddim":
        nm.step(x, out, pos, *args, None, nz, sched=d.ddim_tables(5, 0.5, cuda), **kw)
    else:
        nm.step(x, out, pos, *args, None, None, sched=d.dpm_tables(5, "uniform", cuda), hist=hist, **kw)


@pytest.mark.parametrize("B,hw", [(3, 32), (2, 28)])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_unperturbed_branches_untouched(model, cuda, kind, B, hw):
    """K = 2 with the weights (g, 0): the perturbed branch 2 does not enter eps, so the step equals the
    one without perturb — the rows of branches 0 and 1 have the bits of the full-batch attention."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    gen = torch.Generator().manual_seed(300 + hw)
    x, h0, nz = (torch.randn((B, 4, hw, hw), generator=gen).to(cuda) for _ in range(3))
    comp, pt = pag_case(d, "all6", B, 301 + hw)
    y_rows, v_rows, m_rows, w = comp
    w = torch.stack([torch.full((B,), G), torch.zeros(B)])
    comp = to((y_rows, v_rows, m_rows, w), cuda)
    pos = torch.full((B,), 3, dtype=torch.long, device=cuda)
    t = torch.full((B,), 600, dtype=torch.long, device=cuda)
    a, b = torch.empty_like(x), torch.empty_like(x)
    ha, hb = h0.clone(), h0.clone()
    step_call(nm, d, cuda, kind, x, a, nz, ha, pos, t, compose=comp)
    step_call(nm, d, cuda, kind, x, b, nz, hb, pos, t, compose=comp, perturb=pt)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(ha, hb)


# ---- 4: steps against the oracle -----------------------------------------------------------------------------------
_STEP_REF = {}


def step_ref(unet_sd, d, name, B, hw):
    """Inputs and the oracle's mixed eps at timestep 600 — position 3 of ddim_timesteps(5), which is also
    dpm_timesteps(5, "uniform") — once per case and size."""
    key = (name, B, hw)
    if key not in _STEP_REF:
        gen = torch.Generator().manual_seed(400 + hw + B)
        x, hist, nz = (torch.randn((B, 4, hw, hw), generator=gen) for _ in range(3))
        comp, pt = pag_case(d, name, B, 401 + hw)
        t = torch.full((B,), 600, dtype=torch.long)
        _STEP_REF[key] = (x, hist, nz, comp, pt, t, composed_eps(unet_sd, x, t, comp, pt))
    return _STEP_REF[key]


def pag_step_vs_oracle(nm, d, cuda, unet_sd, kind, name, B, hw, philox=False):
    x, hist, nz, comp, pt, t, eps = step_ref(unet_sd, d, name, B, hw)
    pos = torch.full((B,), 3, dtype=torch.long)
    out = torch.empty((B, 4, hw, hw), device=cuda)
    kw = {}
    if philox:   # the step draws its own noise, keyed by (seed, timestep, sample)
        nz, kw = device_noise(d, 77, x.shape, 600, cuda), dict(seed=77)
    if kind == "ddpm":
        _, a, ab = ref.schedule(1000)
        exp = ref.ddpm_update(x, eps, t, a, ab, nz)
    elif kind == "ddim":
        exp = ddim_update(x, eps, pos, d.ddim_tables(5, 0.5, "cpu"), nz)
    else:
        exp, exp_h = dpm_update(x, eps, pos, d.dpm_tables(5, "uniform", "cpu"), hist)
    h = hist.to(cuda)
    step_call(nm, d, cuda, kind, x.to(cuda), out, None if philox else nz.to(cuda), h, pos.to(cuda), t.to(cuda),
              compose=to(comp, cuda), perturb=pt, **kw)
    if kind == "dpm":
        assert rel(h, exp_h) <= TOL
    return rel(out, exp)


@pytest.mark.parametrize("B,hw", [(3, 32), (2, 28)])
@pytest.mark.parametrize("kind,philox", [("ddpm", False), ("ddpm", True), ("ddim", False), ("ddim", True),
                                         ("dpm", False)])
def test_pag_step_vs_oracle(model, cuda, unet_sd, kind, philox, B, hw):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    comp, pt = step_ref(unet_sd, d, "pag33", B, hw)[3:5]
    assert comp[0].shape[0] == 3 and pt == (4, 4)
    assert torch.equal(comp[3], torch.tensor([[G + S] * B, [-S] * B]))
    err = pag_step_vs_oracle(model.native(), d, cuda, unet_sd, kind, "pag33", B, hw, philox)
    print(f"[pag step {kind} {'philox' if philox else 'given'} g=3 s=3 B={B} {hw}x{hw}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TOL, err


@pytest.mark.parametrize("B,hw", [(3, 32), (2, 28)])
@pytest.mark.parametrize("name,kind,rows", [("persample", "ddpm", 3), ("dropped_also", "ddim", 4), ("g0", "dpm", 2)])
def test_pag_step_forms_vs_oracle(model, cuda, unet_sd, name, kind, rows, B, hw):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    comp, pt = step_ref(unet_sd, d, name, B, hw)[3:5]
    assert comp[0].shape[0] == rows and pt[1] == 1 << (rows - 1)
    if name == "persample":
        assert bool((comp[3][1] == 0).any()) and bool((comp[3][1] < 0).any())
    if name == "g0":
        assert torch.equal(comp[0][0], comp[0][1]) and torch.equal(comp[3], torch.full((1, B), -S))
    err = pag_step_vs_oracle(model.native(), d, cuda, unet_sd, kind, name, B, hw)
    print(f"[pag step {kind} {name} B={B} {hw}x{hw}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TOL, err


# ---- 5: the Winograd batch class ---------------------------------------------------------------------------------
def test_winograd_batch_class_vs_oracle(model, cuda, unet_sd):
    """B = 22 with three branches: N = 66 rows run in the 128-sample class; sa1 + sa3 perturbed."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    err = pag_step_vs_oracle(model.native(), d, cuda, unet_sd, "ddim", "sa13", 22, 32)
    print(f"[pag step ddim sa1+sa3 B=22 32x32] rel-L2 vs oracle = {err:.3e}")
    assert err <= TOL, err


# ---- 6: trajectories through sample_latent_cond -----------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("case,T,kw", [
    ("ddpm", 12, dict()),
    ("ddim", 1000, dict(sampler="ddim", steps=10, eta=0.5)),
    ("dpmpp_2m", 1000, dict(sampler="dpmpp_2m", steps=8)),
])
def test_pag_trajectory_vs_oracle(model, cuda, unet_sd, case, T, kw, source):
    import diff
    d = diff.Diffuser(T, device=cuda)
    d.noise_source = source
    B, hw = 3, 16
    counts = {1: 2, 3: 1}
    y = torch.tensor([1, 1, 3])
    _, vals, mask = cond(B, 600)
    s = [2.0, 0.0, 1.0] if case == "dpmpp_2m" else 2.0   # (the dpmpp_2m case carries a per-sample scale)
    blocks = ("sa2", "sa3", "sa5") if case != "ddim" else ("sa3",)
    comp, pt = d._pag_args(s, blocks, y.tolist(), vals, mask, G)
    mode = d._sampler_mode(kw.get("sampler", "ddpm"), kw.get("steps"), kw.get("eta", 0.0), None, T)
    tau = d._mode_timesteps(mode)
    torch.manual_seed(602)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=G,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), pag_scale=s, pag_blocks=blocks, **kw)
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
    x = rules.trajectory(x, *mode_tables(d, mode), lambda x, t, pos: composed_eps(unet_sd, x, t, comp, pt), noise_of)
    assert torch.isfinite(x).all()
    err = rel(out, x)
    print(f"[pag trajectory {case} {source}] B={B} {hw}x{hw}: rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err


# ---- 7: the loop and its graphs ---------------------------------------------------------------------------------
def test_pag_device_loop_graph_eager_steps_fresh(model, model2, cuda):
    """Ten steps = one launch of the 8-step graph + two of the 1-step graph."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    B = 4
    gen = torch.Generator().manual_seed(700)
    x0 = torch.randn((B, 4, 32, 32), generator=gen).to(cuda)
    comp, pt = pag_case(d, "dropped_also", B, 701)
    comp = to(comp, cuda)
    sched = d.ddim_tables(25, 1.0, cuda)

    def loop(mdl, use_graph):
        x = x0.clone()
        t = torch.full((1,), 25, dtype=torch.long, device=cuda)
        mdl.native().sample_loop(x, t, None, 0, None, None, 0.0, None, 10, seed=7, use_graph=use_graph, sched=sched,
                                 compose=comp, perturb=pt)
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
                t_stride=0, sched=sched, compose=comp, perturb=pt)
        a, b = b, a
    assert torch.equal(a.cpu(), graph)
    # the composition alone is another loop
    x = x0.clone()
    t = torch.full((1,), 25, dtype=torch.long, device=cuda)
    nm.sample_loop(x, t, None, 0, None, None, 0.0, None, 10, seed=7, sched=sched, compose=comp)
    assert not torch.equal(x.cpu(), graph)


def test_pag_and_plain_loops_keep_their_graphs(cuda, unet_sd):
    """PAG, plain, PAG loops on one model, one x and one scalar capture 1, 1, 0 graph pairs; the composed
    loop over the same tables without perturb is a third key."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = make_model(cuda, unet_sd).native()   # a fresh arena and empty slots
    B = 2
    gen = torch.Generator().manual_seed(710)
    x0 = torch.randn((B, 4, 16, 16), generator=gen).to(cuda)
    y, vals, mask = cond(B, 711)
    comp, pt = d._pag_args(S, ("sa2", "sa3"), y.tolist(), vals, mask, G)
    y, vals, mask, comp = y.to(cuda), vals.to(cuda), mask.to(cuda), to(comp, cuda)
    sched = d.dpm_tables(10, "logsnr", cuda)
    x, hist = torch.empty_like(x0), torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(kind, use_graph=True):
        x.copy_(x0)
        hist.fill_(float("nan"))
        t.fill_(10)
        c0 = nm.graph_captures()
        if kind == "plain":
            nm.sample_loop(x, t, y, 0, vals, mask, G, None, 10, use_graph=use_graph, sched=sched, hist=hist)
        else:
            nm.sample_loop(x, t, None, 0, None, None, 0.0, None, 10, use_graph=use_graph, sched=sched, hist=hist,
                           compose=comp, **(dict(perturb=pt) if kind == "pag" else {}))
        torch.cuda.synchronize()
        assert int(t.item()) == 0
        return x.clone(), nm.graph_captures() - c0

    want = {k: loop(k, use_graph=False)[0] for k in ("pag", "plain", "composed")}   # (the larger plan first)
    assert not torch.equal(want["pag"], want["plain"]) and not torch.equal(want["pag"], want["composed"])
    for kind, captures in (("pag", 1), ("plain", 1), ("pag", 0), ("composed", 1), ("pag", 0)):
        out, cap = loop(kind)
        assert cap == captures, (kind, cap, captures)
        assert torch.equal(out, want[kind])


def test_zero_scale_is_the_call_without_the_keywords(model, cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = "device"
    _, vals, mask = cond(3, 720)
    kw = dict(z_shape=(4, 16, 16), vae=None, progress=False, guidance_scale=G, cond=vals.to(cuda),
              cond_mask=mask.to(cuda), sampler="ddim", steps=6, eta=1.0)
    nm = model.native()
    outs = []
    for extra in (dict(), dict(pag_scale=0.0, pag_blocks=("sa1", "sa2")), dict(pag_scale=[0.0, 0.0, 0.0])):
        torch.manual_seed(721)
        outs.append(d.sample_latent_cond(model, {1: 2, 3: 1}, **kw, **extra))
        state = torch.get_rng_state()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    torch.manual_seed(721)
    pag = d.sample_latent_cond(model, {1: 2, 3: 1}, **kw, pag_scale=1.0, pag_blocks=("sa1", "sa2"))
    assert torch.isfinite(pag).all() and not torch.equal(pag, outs[0])
    assert torch.equal(state, torch.get_rng_state())     # the draw order does not depend on the keywords
    assert nm.precision == "x3"


# ---- 8: with the existing features ----------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(model, cuda):
    """B = 5 equals the shards 3 + 2 (sample_offset keeps the Philox rows), bit for bit."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    gen = torch.Generator().manual_seed(77)
    x = torch.randn((5, 4, 16, 16), generator=gen).to(cuda)
    comp, pt = pag_case(d, "persample", 5, 78)
    comp = to(comp, cuda)
    pos = torch.full((5,), 4, dtype=torch.long, device=cuda)
    sched = d.ddim_tables(6, 1.0, cuda)

    def run(s, e):
        out = torch.empty_like(x[s:e])
        nm.step(x[s:e].contiguous(), out, pos[s:e], None, 0, None, None, 0.0, None, None, seed=11, sample_offset=s,
                sched=sched, compose=tuple(c[:, s:e].contiguous() for c in comp), perturb=pt)
        return out

    whole = run(0, 5)
    parts = torch.cat([run(0, 3), run(3, 5)])
    assert torch.isfinite(whole).all()
    assert torch.equal(whole, parts)


@pytest.mark.parametrize("source", ["host", "device"])
def test_known_region_with_pag(model, cuda, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    gen = torch.Generator().manual_seed(920)
    B = 2
    z0 = torch.randn((B, 4, 16, 16), generator=gen)
    m = torch.ones((B, 1, 16, 16))
    m[:, :, :, :8] = 0.0          # keep the left half
    _, vals, mask = cond(B, 921)
    kw = dict(z_shape=(4, 16, 16), vae=None, progress=False, guidance_scale=G, cond=vals.to(cuda),
              cond_mask=mask.to(cuda), sampler="dpmpp_2m", steps=6, init_latent=z0.to(cuda), mask=m.to(cuda),
              strength=0.7)
    torch.manual_seed(923)
    out = d.sample_latent_cond(model, {1: 1, 3: 1}, pag_scale=[2.0, 0.5], pag_blocks=("sa2", "sa3"), **kw).cpu()
    torch.manual_seed(923)
    plain = d.sample_latent_cond(model, {1: 1, 3: 1}, **kw).cpu()
    keep = (m == 0).expand_as(z0)
    assert torch.equal(out[keep], z0[keep]) and torch.equal(plain[keep], z0[keep])
    assert torch.isfinite(out).all() and not torch.equal(out, plain)


@pytest.mark.parametrize("source,kw", [("device", dict(sampler="dpmpp_2m", steps=6)),
                                       ("host", dict(sampler="ddim", steps=5, eta=1.0))])
def test_sharded_world1_equals_diffuser(model, cuda, source, kw):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    _, vals, mask = cond(5, 900)
    vals, mask = vals.to(cuda), mask.to(cuda)
    pkw = dict(guidance_scale=G, pag_scale=[3.0, 2.0, 0.0, 1.0, 4.0], pag_blocks=("sa2", "sa3", "sa4"))
    torch.manual_seed(902)
    lat = dd.ShardedCondSampler(d, model, None).sample({1: 3, 3: 2}, z_shape=(4, 16, 16), cond=vals, cond_mask=mask,
                                                       decode=False, **kw, **pkw)
    s_sharded = torch.get_rng_state()
    torch.manual_seed(902)
    single = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals,
                                  cond_mask=mask, **kw, **pkw)
    assert torch.equal(lat.cpu(), single.cpu()) and torch.isfinite(single).all()
    assert torch.equal(s_sharded, torch.get_rng_state())
    torch.manual_seed(902)
    plain = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals,
                                 cond_mask=mask, guidance_scale=G, **kw)
    assert not torch.equal(plain, single)
    assert torch.equal(s_sharded, torch.get_rng_state())   # the draw order does not depend on the keywords


def test_entity_csv_sampler_passes_pag(model, cuda, vae_sd):
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
    same = s.sample(csv, pag_scale=0.0, pag_blocks=("sa1",), **kw)
    torch.manual_seed(510)
    other = s.sample(csv, pag_scale=2.0, pag_blocks=("sa2", "sa3"), **kw)
    vals, mask = s.load_cond(csv, count=2, start=1)
    torch.manual_seed(510)
    exp = d.sample_latent_cond(model, (1, 2), vae=vae, guidance_scale=3.0, cond=vals, cond_mask=mask,
                               sampler="dpmpp_2m", steps=4, progress=False, pag_scale=2.0, pag_blocks=("sa2", "sa3"))
    for a, b in zip(plain, same):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(other, exp):      # the keywords pass through
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert any(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(other, plain))


# ---- the C entries' argument rules ----------------------------------------------------------------------------------
def test_c_entries_reject_bad_perturbations(model, cuda):
    """Argument checks on the host: every case returns DMX_E_ARG with a message and launches nothing."""
    import diff
    from dmx import _lib
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    lib = nm.lib
    B = 2
    x = torch.zeros((B, 4, 8, 8), device=cuda)
    out = torch.empty_like(x)
    t = torch.full((B,), 5, dtype=torch.long, device=cuda)
    y, vals, mask = cond(B, 1)
    comp, pt = d._pag_args(S, ("sa1",), y.tolist(), vals, mask, G)
    y_rows, v_rows, m_rows, w = to(comp, cuda)
    tables = d.coef_tables(cuda, True)
    nm.ctx.ensure_time_table(1000)
    y, vals, mask = y.to(cuda), vals.to(cuda), mask.to(cuda)
    a = nm._args(x, out, t, 1, y, 0, vals, mask, G, tables, x, 0, 0)
    c = _lib.Compose(2, y_rows.data_ptr(), v_rows.data_ptr(), m_rows.data_ptr(), w.data_ptr())

    def call(blocks=1, branches=4, comp=c, gd=None, loop=False):
        p = _lib.Perturb(blocks, branches)
        cp = ctypes.byref(comp) if comp is not None else None
        gp = ctypes.byref(gd) if gd is not None else None
        with torch.cuda.device(cuda):
            if loop:
                rc = lib.dmx_sample_loop_perturbed(nm.handle, ctypes.byref(a), None, None, None, gp, cp, ctypes.byref(p),
                                                   1, 0, None)
            else:
                rc = lib.dmx_step_perturbed(nm.handle, ctypes.byref(a), None, None, None, gp, cp, ctypes.byref(p), None)
        return rc, (lib.dmx_last_error() or b"").decode()

    bad = dict(blocks0=dict(blocks=0), blocks64=dict(blocks=64), none=dict(branches=0), middle=dict(branches=2),
               gap=dict(branches=5), beyond=dict(branches=8), past=dict(branches=12), no_compose=dict(comp=None),
               rescale=dict(gd=_lib.Guidance(0.5)))
    for loop in (False, True):
        for name, kw in bad.items():
            rc, msg = call(loop=loop, **kw)
            assert rc == _lib.DMX_E_ARG and msg, (name, loop, rc, msg)
    torch.cuda.synchronize()
    for branches in (4, 6, 7):   # trailing runs of 0..2, well-formed, run
        rc, msg = call(branches=branches)
        assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    with pytest.raises(_lib.DmxError):
        nm.step(x, out, t, None, 0, None, None, 0.0, tables, x, compose=(y_rows, v_rows, m_rows, w), perturb=(1, 2))
    with pytest.raises(ValueError):
        nm.step(x, out, t, y, 0, vals, mask, G, tables, x, perturb=(1, 4))


@pytest.mark.parametrize("composed", [False, True])
def test_perturbed_entry_without_perturb_is_the_narrower_entry(cuda, unet_sd, composed):
    """dmx_step_perturbed / dmx_sample_loop_perturbed with perturb = NULL: the bits of dmx_*_composed
    (compose given) or dmx_*_guided (compose NULL too), and the loop replays that entry's graph."""
    import diff
    from dmx import _lib, engine
    d = diff.Diffuser(1000, device=cuda)
    nm = make_model(cuda, unet_sd).native()   # its own graph slots
    lib, h = nm.lib, nm.handle
    nm.ctx.ensure_time_table(1000)
    B, n_steps = 2, 3
    gen = torch.Generator().manual_seed(950)
    x0 = torch.randn((B, 4, 8, 8), generator=gen).to(cuda)
    x, out, hist = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
    t = torch.zeros((B,), dtype=torch.long, device=cuda)
    y, vals, mask = (v.to(cuda) for v in cond(B, 951))
    comp, _ = d._pag_args(S, ("sa1",), y.tolist(), vals.cpu(), mask.cpu(), G)
    y_rows, v_rows, m_rows, w = to(comp, cuda)
    c = _lib.Compose(2, y_rows.data_ptr(), v_rows.data_ptr(), m_rows.data_ptr(), w.data_ptr()) if composed else None
    cp = ctypes.byref(c) if c is not None else None
    dpm = engine._dpm_struct(d.dpm_tables(n_steps, "uniform", cuda), cuda, hist, x)
    gd = _lib.Guidance(0.0)
    side = nm.side_stream()

    def run(general, loop):
        x.copy_(x0)
        out.fill_(float("nan"))
        hist.fill_(float("nan"))
        t.fill_(n_steps)
        torch.cuda.synchronize()
        c0 = nm.graph_captures()
        a = nm._args(x, x if loop else out, t[:1] if loop else t, 0 if loop else 1, y, 0, vals, mask, G, None, None, 0, 0)
        head = (h, ctypes.byref(a), None, ctypes.byref(dpm), None, ctypes.byref(gd))
        with torch.cuda.device(cuda):
            st = ctypes.c_void_p(side.cuda_stream if loop else torch.cuda.current_stream(cuda).cuda_stream)
            if loop:
                fn = lib.dmx_sample_loop_perturbed if general else (
                    lib.dmx_sample_loop_composed if composed else lib.dmx_sample_loop_guided)
                tail = (n_steps, 1, st)
            else:
                fn = lib.dmx_step_perturbed if general else (lib.dmx_step_composed if composed else lib.dmx_step_guided)
                tail = (st,)
            mid = ((cp, None) if general else (cp,) if composed else ())
            _lib.check(fn(*head, *mid, *tail))
        torch.cuda.synchronize()
        return (x if loop else out).clone(), hist.clone(), nm.graph_captures() - c0

    for loop in (False, True):
        general, narrow = run(True, loop), run(False, loop)
        assert torch.isfinite(general[0]).all() and not torch.equal(general[0], x0)
        assert torch.equal(general[0], narrow[0]) and torch.equal(general[1], narrow[1])
        if loop:
            assert (general[2], narrow[2]) == (1, 0)   # the narrower entry replayed the general entry's graph


# ---- 9: workspace diagnostics -----------------------------------------------------------------------------------------
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
m = UnetCondWithGeomHead()
m.load_state_dict(synth.unet_cond_geom_weights(0))
m.to(dev).eval()
d = diff.Diffuser(4, device=dev)
tables = d.coef_tables(dev, clamp_prev=True)
nm = m.native()
y = [1, 2, 3]
vals = torch.rand((B, 12), generator=g)
mask = (torch.rand((B, 12), generator=g) > 0.3).float()
comp, pt = d._pag_args([3.0, 0.0, 1.5], ("sa1", "sa2", "sa3", "sa4", "sa5", "sa6"), y, vals, mask, 3.0)
comp = tuple(c.to(dev).contiguous() for c in comp)
for prec in ("x3", "fp32"):   # the fused token kernels, and the unfused attention block
    nm.set_precision(prec)
    for hw in (16, 28):
        x = torch.randn((B, 4, hw, hw), generator=g).to(dev)
        noise = torch.randn((B, 4, hw, hw), generator=g).to(dev)
        tt = torch.full((B,), 4, dtype=torch.long, device=dev)
        o = torch.empty_like(x)
        nm.step(x, o, tt, None, 0, None, None, 0.0, tables, noise, compose=comp, perturb=pt)
        out[f"step_{prec}_{hw}"] = o.cpu()
        yy = torch.tensor(y * 2, device=dev)
        e, _ = nm.forward(torch.cat([x, x]), torch.cat([tt, tt]), yy, torch.cat([vals, vals]).to(dev),
                          torch.cat([mask, mask]).to(dev), perturb=(0b101010, 2, 5))
        out[f"fwd_{prec}_{hw}"] = e.cpu()
torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print("[pag-worker] ok", flush=True)
'''


def test_pag_step_reads_no_unwritten_workspace(cuda, tmp_path):
    """PAG steps and perturbed forwards (a range in the middle of the batch) in fresh processes, with
    and without DMX_POISON=1 / DMX_CHECK=1: finite and bit-identical."""
    clean = run_worker(tmp_path, "clean", WORKER)
    diag = run_worker(tmp_path, "diag", WORKER, DMX_POISON="1", DMX_CHECK="1")
    assert len(clean) == 8
    bad = [k for k in clean if not torch.isfinite(diag[k]).all() or not torch.equal(clean[k], diag[k])]
    assert bad == [], bad
