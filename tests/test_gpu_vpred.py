"""GPU: v-prediction — the standalone conversion and the training target bit for bit, one native step per
rule, trajectories, graphs, the combinations with every guidance form, training and the range guard —
against a torch-CPU restatement on top of the oracle's forwards (oracle.ref / oracle.train_ref).

The v-rule of every step: oracle forward(s) -> the mix in output space (CFG, composition,
perturbed branch, CFG rescale, geometry guidance) -> the conversion, once,
    eps = p_o[t-1] out + p_x[t-1] x_net      p_o = sqrt(ab), p_x = sqrt(1-ab), t the network timestep,
                                             x_net the latent the network was evaluated at
-> the eps-form update, all restated in oracle/rules.py.  Bounds are the project's: 2e-5 for one
step, 1e-4 for a trajectory and for a gradient tensor, 2e-5 for the loss, rel-L2 against the fp32 oracle."""
import os

import pytest
import torch

from oracle import ref, rules, train_ref
from oracle.rules import (Foreign, cfg_eps, cfg_rescaled, composed_eps, ddim_update, dpm_update, invert_update,
                          known_blend, rel, row)
from support import cond, device_noise, make_model, mode_tables, on, overflow_sd

pytestmark = pytest.mark.gpu

TOL = 2e-5        # one step (the project's step bound)
TRAJ_TOL = 1e-4   # a trajectory (the project's trajectory bound)
GRAD_TOL = 1e-4   # a gradient tensor (the project's bound for the native backward)
LOSS_TOL = 2e-5
G = 3.0
T = 1000


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return make_model(cuda, unet_sd)


@pytest.fixture(scope="module")
def unet3_sd():
    from dmx import synth
    return synth.unet_weights(0, in_ch=3)


@pytest.fixture(scope="module")
def unet3(cuda, unet3_sd):
    from models.unet import Unet
    m = Unet(in_ch=3)
    m.load_state_dict(unet3_sd)
    return m.to(cuda).eval()


def dv(dev, T=T):
    import diff
    return diff.Diffuser(T, device=dev, prediction="v")


def de(dev, T=T):
    import diff
    return diff.Diffuser(T, device=dev)


def to_eps_of(d, out, x_net, t):
    """rules.to_eps at the network timesteps t (B,) with d's tables."""
    return rules.to_eps(out, x_net, t, *d.pred_tables("cpu"))


# ---- 1: the standalone conversion, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 4, 16, 16), (6, 3, 16, 16), (5, 3, 9, 7)])
def test_pred_to_eps_bit_exact(cuda, shape):
    from dmx import engine
    d = dv(cuda)
    B = shape[0]
    g = torch.Generator().manual_seed(11 + shape[1] + shape[2])
    out, x = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    t = torch.tensor(([1, 2, 500, 999, 1000, 37] * 2)[:B])
    exp = to_eps_of(d, out, x, t)
    tabs = d.pred_tables(cuda)
    assert torch.equal(tabs[0].cpu(), d.noise_tables("cpu")[0]) and torch.equal(tabs[1].cpu(), d.noise_tables("cpu")[1])
    got = engine.pred_to_eps(out.to(cuda), x.to(cuda), t.to(cuda), *tabs)
    assert torch.equal(got.cpu(), exp)
    # aliased: the result lands in `out`
    o = out.to(cuda)
    res = engine.pred_to_eps(o, x.to(cuda), t.to(cuda), *tabs, inplace=True)
    assert res.data_ptr() == o.data_ptr() and torch.equal(o.cpu(), exp)
    # a strided t (every other entry of a longer tensor), and one value for every sample
    wide = torch.full((2 * B,), 777, dtype=torch.long)
    wide[::2] = t
    ts = wide.to(cuda)[::2]
    assert ts.stride(0) == 2
    assert torch.equal(engine.pred_to_eps(out.to(cuda), x.to(cuda), ts, *tabs).cpu(), exp)
    one = engine.pred_to_eps(out.to(cuda), x.to(cuda), torch.tensor([500], device=cuda), *tabs)
    assert torch.equal(one.cpu(), to_eps_of(d, out, x, torch.full((B,), 500)))
    # timesteps outside [1, T] are clamped for the table reads
    far = engine.pred_to_eps(out.to(cuda), x.to(cuda), torch.tensor([-3, 5000] * 3, device=cuda)[:B], *tabs)
    assert torch.equal(far.cpu(), to_eps_of(d, out, x, torch.tensor([1, T] * 3)[:B]))
    with pytest.raises(ValueError):
        engine.pred_to_eps(out.to(cuda), x.to(cuda)[:, :1], t.to(cuda), *tabs)
    with pytest.raises(ValueError):
        engine.pred_to_eps(out.to(cuda), x.to(cuda), t.to(cuda)[:2], *tabs)
    xa = x.to(cuda)
    with pytest.raises(ValueError):
        engine.pred_to_eps(xa, xa, t.to(cuda), *tabs, inplace=True)


# ---- 2: the training target, bit for bit ---------------------------------------------------------------
def front_inputs(shape, seed=0, gd=12):
    B = shape[0]
    g = torch.Generator().manual_seed(seed)
    z, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    t = torch.randint(1, T + 1, (B,), generator=g)
    t[0], t[-1] = 1, T
    y = torch.randint(1, 4, (B,), generator=g)
    vals = torch.rand((B, gd), generator=g) - 0.25
    mask = (torch.rand((B, gd), generator=g) > 0.3).float()
    drop = torch.zeros(B, dtype=torch.bool)
    drop[B // 2] = True
    return z, noise, t, y, vals, mask, drop


@pytest.mark.parametrize("shape", [(3, 4, 8, 8), (1, 4, 28, 28), (5, 3, 9, 7)])  # (the last: the element path)
def test_train_noise_target_bit_exact(cuda, shape):
    from dmx import engine
    d = dv(cuda)
    sa, s1 = d.noise_tables(cuda)
    z, noise, t, y, vals, mask, drop = on(cuda, *front_inputs(shape))
    for tt in ([t] if shape[0] > 1 else [torch.full_like(t, 1), torch.full_like(t, T)]):
        plain = engine.train_noise(z, sa, s1, tt, noise, drop, y, 7, vals, mask)
        full = engine.train_noise(z, sa, s1, tt, noise, drop, y, 7, vals, mask, target=True)
        assert len(plain) == 7 and len(full) == 8
        for a, b in zip(plain, full[:7]):
            assert torch.equal(a, b)
        exp = row(sa.cpu(), tt.cpu()) * noise.cpu() - row(s1.cpu(), tt.cpu()) * z.cpu()
        assert torch.equal(full[7].cpu(), exp)
        buf = torch.full_like(z, float("nan"))
        again = engine.train_noise(z, sa, s1, tt, noise, drop, y, 7, vals, mask, target=buf)
        assert again[7] is buf and torch.equal(buf.cpu(), exp)
    # drawn noise: the target is the formula on the noise the same launch stored
    dr = engine.train_noise(z, sa, s1, None, None, None, y, 0, vals, mask, 0.5, seed=99, target=True)
    pl = engine.train_noise(z, sa, s1, None, None, None, y, 0, vals, mask, 0.5, seed=99)
    for a, b in zip(pl, dr[:7]):
        assert torch.equal(a, b)
    assert torch.equal(dr[7].cpu(), row(sa.cpu(), dr[2].cpu()) * dr[1].cpu() - row(s1.cpu(), dr[2].cpu()) * z.cpu())
    for bad in (torch.empty(shape, device=cuda, dtype=torch.float64), torch.empty(shape),
                torch.empty((1,), device=cuda)):
        with pytest.raises(ValueError):
            engine.train_noise(z, sa, s1, t, noise, target=bad)


# ---- 3: one native step per rule against the oracle ------------------------------------------------------
B3, HW3, S3 = 3, 16, 50
POS3 = [1, 25, 50]
_STEP = {}


def step_inputs():
    g = torch.Generator().manual_seed(31)
    x = torch.randn((B3, 4, HW3, HW3), generator=g)
    other = 0.8 * torch.randn((B3, 4, HW3, HW3), generator=g)  # the DPM history / the inversion's source latent
    y = torch.tensor([1, 3, 2])
    vals = torch.rand((B3, 12), generator=g)
    mask = (torch.rand((B3, 12), generator=g) > 0.4).float()
    return x, other, y, vals, mask, seeded_noise(x.shape)


NOISE_SEED = 78


def seeded_noise(shape):
    """The one randn(shape) a host-noise step draws after torch.manual_seed(NOISE_SEED); the global
    generator is left as it was."""
    state = torch.get_rng_state()
    torch.manual_seed(NOISE_SEED)
    nz = torch.randn(tuple(shape))
    torch.set_rng_state(state)
    return nz


def rule_case(d, rule):
    """-> (pos as the rule counts it, the network timesteps, the CPU tables)."""
    if rule == "ddpm":
        t = torch.tensor([1, 500, 1000])
        return t, t, None
    if rule == "ddim":
        sched = d.ddim_tables(S3, 0.5, "cpu")
    elif rule == "dpm":
        sched = d.dpm_tables(S3, "logsnr", "cpu")
    else:  # inversion, R = 1: 100 rows in countdown order; (p, k) = (1, 0), (25, 1) and (50, 1)
        sched = d.invert_tables(S3, None, 1, "cpu")
        c = torch.tensor([100, 51, 1])
        assert sched[3][c - 1].tolist() == [0, 1, 1]
        return c, sched[0][c - 1], sched
    pos = torch.tensor(POS3)
    return pos, sched[0][pos - 1], sched


def step_ref(sd, rule, g=G):
    """The v-rule of one step on the CPU, once per rule and guidance -> (x', hist or src afterwards)."""
    key = (rule, g)
    if key not in _STEP:
        d = dv("cpu")
        x, other, y, vals, mask, nz = step_inputs()
        pos, t, sched = rule_case(d, rule)
        assert pos.tolist() != t.tolist() or rule == "ddpm"  # position differs from timestep
        eps = to_eps_of(d, cfg_eps(sd, x, t, y, vals, mask, g), x, t)
        if rule == "ddpm":
            _, a, ab = ref.schedule(T)
            _STEP[key] = (ref.ddpm_update(x, eps, t, a, ab, nz), None)
        elif rule == "ddim":
            _STEP[key] = (ddim_update(x, eps, pos, sched, nz), None)
        elif rule == "dpm":
            _STEP[key] = dpm_update(x, eps, pos, sched, other)
        else:
            _STEP[key] = invert_update(other, eps, pos, sched)
    return _STEP[key]


def run_step(d, mdl, cuda, rule, g=G):
    """One public step of `rule` on the GPU -> (x', hist or src afterwards)."""
    x, other, y, vals, mask, nz = step_inputs()
    pos = rule_case(d, rule)[0]
    xd, yd, vd, md, pd = on(cuda, x, y, vals, mask, pos)
    kw = dict(y=yd, guidance_scale=g, cond_vals=vd, cond_mask=md)
    if rule in ("ddpm", "ddim"):  # host noise: the step draws one randn(x.shape), nz under this seed
        torch.manual_seed(NOISE_SEED)
        if rule == "ddpm":
            return d.denoise_cond(mdl, xd, pd, **kw), None
        return d.ddim_step(mdl, xd, pd, S3, eta=0.5, **kw), None
    h = other.to(cuda)
    if rule == "dpm":
        return d.dpm_step(mdl, xd, pd, h, S3, **kw), h
    plan = d._plan(xd, ("invert", S3, None, 1), g)
    return d._step(mdl, xd, pd, plan, True, yd, 0, vd, md, hist=h), h


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("rule", ["ddpm", "ddim", "dpm", "invert"])
def test_step_vs_oracle(model, cuda, unet_sd, rule, prec):
    d = dv(cuda)
    exp, exp_h = step_ref(unet_sd, rule)
    with model.native().precision_override(prec):
        out, h = run_step(d, model, cuda, rule)
    assert model.native().prediction == "v"
    err = rel(out, exp)
    print(f"[v step {rule} {prec}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TOL, err
    if exp_h is not None:
        eh = rel(h, exp_h)
        print(f"[v step {rule} {prec}] history / source rel-L2 = {eh:.3e}")
        assert eh <= TOL, eh
    # the eps-reading of the same network is another number: the conversion is not a no-op here
    eps_out, _ = run_step(de(cuda), model, cuda, rule)
    assert rel(eps_out, exp) > 1e-2
    assert model.native().prediction == "eps"


@pytest.mark.parametrize("rule", ["ddpm", "ddim", "dpm", "invert"])
def test_foreign_model_lands_on_the_native_step(model, cuda, unet_sd, rule):
    d = dv(cuda)
    # (a ddpm step with y and guidance 0 is the reference's own error path: denoise_cond mirrors it)
    for g in ((G,) if rule == "ddpm" else (G, 0.0)):
        exp, exp_h = step_ref(unet_sd, rule, g)
        nat, nat_h = run_step(d, model, cuda, rule, g)
        out, h = run_step(d, Foreign(model), cuda, rule, g)
        e_o, e_n = rel(out, exp), rel(out, nat)
        print(f"[v step {rule} g={g} foreign] rel-L2 vs oracle = {e_o:.3e}, vs native = {e_n:.3e}")
        assert e_o <= TOL and e_n <= TOL, (e_o, e_n)
        if exp_h is not None:
            assert rel(h, exp_h) <= TOL and rel(h, nat_h) <= TOL


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_unconditional_unet_denoise(unet3, unet3_sd, cuda, prec):
    """The 3-channel Unet through denoise: the generic tail on a feature map (and a foreign wrapper of it)."""
    d = dv(cuda)
    g = torch.Generator().manual_seed(33)
    x = torch.randn((3, 3, HW3, HW3), generator=g)
    nz = seeded_noise(x.shape)
    t = torch.tensor([1, 500, 1000])
    with torch.no_grad():
        out_ref = ref.unet_forward(unet3_sd, x, t)
    _, a, ab = ref.schedule(T)
    exp = ref.ddpm_update(x, to_eps_of(d, out_ref, x, t), t, a, ab, nz, clamp_prev=False)

    class Wrapped(torch.nn.Module):
        def forward(self, x, t):
            return unet3(x, t)

    for name, mdl in (("native", unet3), ("foreign", Wrapped())):
        torch.manual_seed(NOISE_SEED)
        with unet3.native().precision_override(prec):
            out = d.denoise(mdl, x.to(cuda), t.to(cuda))
        err = rel(out, exp)
        print(f"[v denoise unet3 {name} {prec}] rel-L2 vs oracle = {err:.3e}")
        assert err <= TOL, err


# ---- 4: trajectories -----------------------------------------------------------------------------------
def sample_vs_oracle(model, cuda, sd, Tn, hw, kw, source, seed, extra=None, out_of=None, tag=""):
    d = dv(cuda, Tn)
    d.noise_source = source
    B, counts = 2, {1: 1, 3: 1}
    y = torch.tensor([1, 3])
    _, vals, mask = cond(B, seed)
    mode = d._sampler_mode(kw.get("sampler", "ddpm"), kw.get("steps"), kw.get("eta", 0.0), None, Tn)
    tau = d._mode_timesteps(mode)
    torch.manual_seed(seed + 1)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=G,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), **kw, **(extra or {}))
    assert d.range_fallbacks == 0
    torch.manual_seed(seed + 1)
    x = torch.randn((B, 4, hw, hw))
    noisy = mode is None or (mode[0] == "ddim" and mode[2] > 0)
    if not noisy:
        noise_of = lambda p: torch.zeros_like(x)  # noqa: E731
    elif source == "host":
        noise_of = lambda p: torch.randn(x.shape)  # noqa: E731  (one global draw per step, in step order)
    else:
        s = d._seed()  # drawn after x_T, as the sampler does
        noise_of = lambda p: device_noise(d, s, x.shape, tau[p - 1], cuda)  # noqa: E731
    out_of = out_of(d, y, vals, mask) if out_of is not None else (lambda x, t: cfg_eps(sd, x, t, y, vals, mask))
    exp = rules.trajectory(x, *mode_tables(d, mode), lambda x, t, pos: to_eps_of(d, out_of(x, t), x, t), noise_of)
    err = rel(out, exp)
    print(f"[v trajectory {tag or kw} {hw}x{hw} {source}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err
    return out


@pytest.mark.parametrize("case,Tn,hw,kw,source", [
    ("ddim8", T, 16, dict(sampler="ddim", steps=8, eta=0.0), "device"),
    ("dpm6", T, 16, dict(sampler="dpmpp_2m", steps=6), "device"),
    ("dpm6", T, 16, dict(sampler="dpmpp_2m", steps=6), "host"),
    ("ddpm12", 12, 16, dict(), "host"),
    ("ddpm12", 12, 16, dict(), "device"),
    ("ddim4-28", T, 28, dict(sampler="ddim", steps=4, eta=0.5), "host"),
    ("ddim4-28", T, 28, dict(sampler="ddim", steps=4, eta=0.5), "device"),
])
def test_trajectory_vs_oracle(model, cuda, unet_sd, case, Tn, hw, kw, source):
    sample_vs_oracle(model, cuda, unet_sd, Tn, hw, kw, source, 60 + hw + len(case), tag=case)


# ---- 5: graphs ------------------------------------------------------------------------------------------
def test_graph_loop_equals_eager_and_follows_the_prediction(cuda, unet_sd):
    model = make_model(cuda, unet_sd)  # graph slots of its own
    nm = model.native()
    d_v, d_e = dv(cuda), de(cuda)
    B, steps = 4, 11  # one 8-step graph launch and three one-step launches
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn((B, 4, 16, 16), generator=g).to(cuda)
    y, vals, mask = on(cuda, *cond(B, 3))
    sched = d_e.ddim_tables(25, 1.0, cuda)
    x = torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(d, use_graph):
        d._set_prediction(nm)
        x.copy_(x0)
        t.fill_(25)
        nm.sample_loop(x, t, y, 0, vals, mask, G, None, steps, seed=1234, use_graph=use_graph, sched=sched)
        torch.cuda.synchronize()
        assert int(t.item()) == 25 - steps
        return x.cpu()

    c0 = nm.graph_captures()
    e1 = loop(d_e, True)
    c1 = nm.graph_captures()
    v2 = loop(d_v, True)
    c2 = nm.graph_captures()
    e3 = loop(d_e, True)
    c3 = nm.graph_captures()
    assert c0 < c1 < c2 < c3, (c0, c1, c2, c3)  # every switch drops the graphs
    assert torch.equal(e1, e3)
    v_eager = loop(d_v, False)
    assert torch.equal(v2, v_eager) and not torch.equal(v2, e1) and torch.isfinite(v2).all()
    assert torch.equal(loop(d_v, True), v2)
    c4 = nm.graph_captures()
    assert torch.equal(loop(d_v, True), v2) and nm.graph_captures() == c4  # the same setting again: a replay
    # eager one-step calls walk the same numbers
    a, b = x0.clone(), torch.empty_like(x0)
    for p in range(25, 25 - steps, -1):
        nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), y, 0, vals, mask, G, None, seed=1234,
                t_stride=0, sched=sched)
        a, b = b, a
    assert torch.equal(a.cpu(), v2)
    # a schedule that names a timestep above the stored T is refused before anything runs
    from dmx._lib import DMX_E_ARG, DmxError
    d12 = dv(cuda, 12)
    d12._set_prediction(nm)
    x.copy_(x0)
    t.fill_(25)
    with pytest.raises(DmxError) as why:
        nm.sample_loop(x, t, y, 0, vals, mask, G, None, 2, seed=1234, sched=sched)
    assert why.value.code == DMX_E_ARG
    with pytest.raises(DmxError):
        nm.step(x0, torch.empty_like(x0), torch.full((1,), 25, dtype=torch.long, device=cuda), y, 0, vals, mask, G,
                None, seed=1234, t_stride=0, sched=sched)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and int(t.item()) == 25


# ---- 6: combinations ---------------------------------------------------------------------------------------
def test_rescale_measures_v(model, cuda, unet_sd):
    def out_of(d, y, vals, mask):
        def f(x, t):
            with torch.no_grad():
                ec, _ = ref.unet_cond_geom_forward(unet_sd, x, t, y, vals, mask)
                eu, _ = ref.unet_cond_geom_forward(unet_sd, x, t, torch.zeros_like(y), vals, mask)
            return cfg_rescaled(eu, ec, G, 0.7)
        return f
    for kw in (dict(sampler="dpmpp_2m", steps=3), dict(sampler="ddim", steps=2, eta=0.0)):
        sample_vs_oracle(model, cuda, unet_sd, T, 16, kw, "device", 71, dict(guidance_rescale=0.7), out_of, "rescale")
    # and one host-stepped step through a foreign model: the same rule
    sample_vs_oracle(Foreign(model), cuda, unet_sd, T, 16, dict(sampler="ddim", steps=2, eta=0.0), "host", 71,
                     dict(guidance_rescale=0.7), out_of, "rescale foreign")


def test_composed_k2(model, cuda, unet_sd):
    _, v2, m2 = cond(2, 81)
    also = [dict(classes=[2, 1], cond=v2, cond_mask=m2, weight=[1.5, -0.5])]

    def out_of(d, y, vals, mask):
        comp = d._compose_args(y.tolist(), vals, mask, G, "null", also, device="cpu")
        assert comp[0].shape[0] == 3  # K = 2
        return lambda x, t: composed_eps(unet_sd, x, t, comp)
    sample_vs_oracle(model, cuda, unet_sd, T, 16, dict(sampler="ddim", steps=3, eta=0.0), "device", 82,
                     dict(also=also), out_of, "also K=2")
    sample_vs_oracle(model, cuda, unet_sd, 4, 16, dict(), "host", 82, dict(also=also), out_of, "also K=2 ddpm")
    sample_vs_oracle(Foreign(model), cuda, unet_sd, T, 16, dict(sampler="dpmpp_2m", steps=2), "host", 82,
                     dict(also=also), out_of, "also K=2 foreign")


def test_pag(model, cuda, unet_sd):
    def out_of(d, y, vals, mask):
        comp, pt = d._pag_args(2.0, ("sa3",), y.tolist(), vals, mask, G)
        return lambda x, t: composed_eps(unet_sd, x, t, comp, pt)
    sample_vs_oracle(model, cuda, unet_sd, T, 16, dict(sampler="ddim", steps=2, eta=0.0), "device", 91,
                     dict(pag_scale=2.0), out_of, "pag")


@pytest.mark.parametrize("rule", ["ddpm", "ddim"])
def test_geom_step_shows_the_divided_sig(model, cuda, unet_sd, rule):
    """The step's own arithmetic: eu / ec from the oracle, dL/dx from the GPU's own geom_grad (whose own bound,
    1e-4, is test_gpu_geom.py's business), so the bound here is the step's: v += s (sig / sqrt(ab)) dL/dx, then
    the conversion, then the update."""
    d = dv(cuda)
    x, other, y, vals, mask, nz = step_inputs()
    pos, t, sched = rule_case(d, rule)
    # (a DDPM step moves x by c1 eps, c1 = beta / sqrt(1 - ab) <= 0.02: it takes a larger scale to show)
    scale = torch.full((B3,), 2000.0 if rule == "ddim" else 40000.0)
    grad = model.geom_grad(*on(cuda, x, t, y, vals, mask))[1].cpu()
    plan = d._plan(x.to(cuda), None if rule == "ddpm" else ("ddim", S3, 0.5), G, geom=scale)
    sig = plan.geom[1].cpu()
    p_o = d.pred_tables("cpu")[0]
    e_sig = de(cuda)._plan(x.to(cuda), None if rule == "ddpm" else ("ddim", S3, 0.5), G, geom=scale).geom[1].cpu()
    # the eps-mode table over sqrt(ab): the tables' own roots (the strided rules': k_e over k_a)
    assert torch.equal(sig, e_sig / (p_o if rule == "ddpm" else sched[2]))
    out_g = cfg_eps(unet_sd, x, t, y, vals, mask)
    mixed = out_g + (scale * sig[pos - 1]).view(-1, 1, 1, 1) * grad
    _, a, ab = ref.schedule(T)

    def upd(o):
        eps = to_eps_of(d, o, x, t)
        return ref.ddpm_update(x, eps, t, a, ab, nz) if rule == "ddpm" else ddim_update(x, eps, pos, sched, nz)

    exp, plain = upd(mixed), upd(out_g)
    share = float((exp - plain).norm() / exp.norm())
    assert share >= 0.05, share
    out = torch.empty(x.shape, device=cuda)
    nm = d._native(model)
    nm.step(x.to(cuda), out, pos.to(cuda), y.to(cuda), 0, vals.to(cuda), mask.to(cuda), G, plan.tables, nz.to(cuda),
            **plan.kwargs(True))
    err = rel(out, exp)
    print(f"[v geom step {rule}] rel-L2 vs restatement = {err:.3e}, share = {share:.3f}")
    assert err <= TOL, err
    # the undivided table would be off by the share of the gradient
    wrong = out_g + (scale * e_sig[pos - 1]).view(-1, 1, 1, 1) * grad
    assert rel(out, upd(wrong)) > 10 * TOL


def test_init_latent_and_mask(model, cuda, unet_sd):
    d = dv(cuda)
    d.noise_source = "device"
    B, hw, S, p0 = 2, 16, 4, 2
    y = torch.tensor([1, 3])
    _, vals, mask = cond(B, 101)
    g = torch.Generator().manual_seed(102)
    z0 = 0.8 * torch.randn((B, 4, hw, hw), generator=g)
    m = torch.zeros((B, 1, hw, hw))
    m[0, :, 3:11, 4:12] = 1.0
    m[1, :, 5:13, 2:9] = 1.0
    m[1, :, 4, :] = 0.25
    torch.manual_seed(103)
    out = d.sample_latent_cond(model, {1: 1, 3: 1}, vae=None, progress=False, guidance_scale=G, cond=vals.to(cuda),
                               cond_mask=mask.to(cuda), sampler="ddim", steps=S, init_latent=z0, mask=m, strength=0.5)
    keep = (m == 0).expand_as(z0)
    assert torch.equal(out.cpu()[keep], z0[keep])  # kept pixels: z0's bits
    torch.manual_seed(103)
    e0 = torch.randn((B, 4, hw, hw))
    mode = ("ddim", S, 0.0)
    tau = d._mode_timesteps(mode)
    tabs, sched = d.known_tables(tau, "cpu"), d.ddim_tables(S, 0.0, "cpu")
    x = known_blend(None, z0, e0, None, torch.full((B,), p0 + 1), tabs)
    for p in range(p0, 0, -1):
        pos = torch.full((B,), p, dtype=torch.long)
        t = sched[0][pos - 1]
        eps = to_eps_of(d, cfg_eps(unet_sd, x, t, y, vals, mask), x, t)
        x = known_blend(ddim_update(x, eps, pos, sched, torch.zeros_like(x)), z0, e0, m, pos, tabs)
    err = rel(out, x)
    print(f"[v inpaint ddim S={S} p0={p0}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err


def test_cache_refresh_steps_are_plain_v_steps(model, cuda, unet_sd):
    d = dv(cuda)
    nm = d._native(model)
    x, other, y, vals, mask, nz = on(cuda, *step_inputs())
    sched = d.ddim_tables(S3, 0.5, cuda)
    pos = torch.full((B3,), 25, dtype=torch.long, device=cuda)
    outs = []
    for cache in (None, (2, 0), (2, 2)):
        out = torch.empty_like(x)
        nm.step(x, out, pos, y, 0, vals, mask, G, None, nz, sched=sched, **({} if cache is None else dict(cache=cache)))
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    t = sched[0][pos - 1].cpu()
    xc, yc, vc, mc = x.cpu(), y.cpu(), vals.cpu(), mask.cpu()
    exp = ddim_update(xc, to_eps_of(d, cfg_eps(unet_sd, xc, t, yc, vc, mc), xc, t), pos.cpu(),
                          d.ddim_tables(S3, 0.5, "cpu"), nz.cpu())
    assert rel(outs[1], exp) <= TOL
    # a reuse step converts too: it runs, is finite and differs from the eps reading of the same step
    reuse = torch.empty_like(x)
    nm.step(x, reuse, pos - 1, y, 0, vals, mask, G, None, nz, sched=sched, cache=(2, 1))
    assert torch.isfinite(reuse).all()
    # the sampler's keyword: whole loop, refreshes at even offsets
    d.noise_source = "device"
    torch.manual_seed(7)
    lat = d.sample_latent_cond(model, {1: 1, 2: 1}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals[:2],
                               cond_mask=mask[:2], sampler="ddim", steps=4, cache_interval=2)
    assert torch.isfinite(lat).all() and nm.prediction == "v"


def test_invert_then_start_latent_round_trip(model, cuda, unet_sd):
    d = dv(cuda)
    B, hw, S, R = 2, 16, 4, 1
    counts = {1: 1, 3: 1}
    y = torch.tensor([1, 3])
    _, vals, mask = cond(B, 111)
    g = torch.Generator().manual_seed(112)
    z0 = 0.8 * torch.randn((B, 4, hw, hw), generator=g)
    kw = dict(guidance_scale=G, cond=vals.to(cuda), cond_mask=mask.to(cuda))
    state = torch.get_rng_state()
    lat = d.invert_latent_cond(model, z0, counts, steps=S, refine=R, **kw)
    back = d.sample_latent_cond(model, counts, vae=None, progress=False, sampler="ddim", steps=S, start_latent=lat,
                                **kw)
    assert torch.equal(torch.get_rng_state(), state)  # nothing is drawn
    tables, sched = d.invert_tables(S, None, R, "cpu"), d.ddim_tables(S, 0.0, "cpu")
    N = int(tables[0].numel())
    x, src = z0, z0
    for c in range(N, 0, -1):  # the conversion reads the latent the network saw: x, not src
        pos = torch.full((B,), c, dtype=torch.long)
        t = tables[0][pos - 1]
        x, src = invert_update(src, to_eps_of(d, cfg_eps(unet_sd, x, t, y, vals, mask), x, t), pos, tables)
    e_inv = rel(lat, x)
    xb = x
    for p in range(S, 0, -1):
        pos = torch.full((B,), p, dtype=torch.long)
        t = sched[0][pos - 1]
        eps = to_eps_of(d, cfg_eps(unet_sd, xb, t, y, vals, mask), xb, t)
        xb = ddim_update(xb, eps, pos, sched, torch.zeros_like(xb))
    e_back = rel(back, xb)
    print(f"[v invert S={S} R={R}] rel-L2 vs restatement: inverted {e_inv:.3e}, sampled back {e_back:.3e}; "
          f"round trip vs z0 {rel(back, z0):.3e} (restatement {rel(xb, z0):.3e})")
    assert e_inv <= TRAJ_TOL and e_back <= TRAJ_TOL, (e_inv, e_back)


# ---- 7: training ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_model(cuda, unet_sd):
    return make_model(cuda, unet_sd).train()


def e2e_inputs(B, hw, seed=31):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, 4, hw, hw), generator=g)
    noise = torch.randn((B, 4, hw, hw), generator=g)
    classes = torch.randint(1, 4, (B,), generator=g)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    t = torch.tensor([1000, 40, 1][:B])
    drop = torch.zeros(B, dtype=torch.bool)
    drop[B - 1] = True
    return z, noise, classes, vals, mask, t, drop


def native_grads(d, model, inputs, cuda, lam, weighting):
    z, noise, classes, vals, mask, t, drop = on(cuda, *inputs)
    model.zero_grad(set_to_none=True)
    res = d.training_loss(model, z, classes, vals, mask, geom_lambda=lam, weighting=weighting, t=t, noise=noise,
                          drop=drop)
    res.loss.backward()
    return res, {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()}


@pytest.mark.parametrize("B,hw,weighting", [(3, 8, "uniform"), (3, 8, "min_snr"), (2, 28, "uniform")])
def test_training_loss_vs_oracle(cuda, train_model, unet_sd, B, hw, weighting):
    from dmx import engine
    d_v, d_e = dv(cuda), de(cuda)
    lam = 0.5
    inputs = e2e_inputs(B, hw)
    z, noise, classes, vals, mask, t, drop = inputs
    before, g_before = native_grads(d_e, train_model, inputs, cuda, lam, weighting)
    res, grads = native_grads(d_v, train_model, inputs, cuda, lam, weighting)
    after, g_after = native_grads(d_e, train_model, inputs, cuda, lam, weighting)
    # eps-mode is untouched by a v-mode iteration in between
    for f in ("loss", "noise_loss", "geom_loss", "per_sample", "eps", "target"):
        assert torch.equal(getattr(before, f).detach(), getattr(after, f).detach()), f
    assert torch.equal(before.target, noise.to(cuda))
    for n in g_before:
        assert (g_before[n] is None) == (g_after[n] is None), n
        assert g_before[n] is None or torch.equal(g_before[n], g_after[n]), n
    # the target: the formula with the tables' bits, and what train_noise stores
    sa, s1 = d_v.noise_tables(cuda)
    exp_t = row(sa.cpu(), t) * noise - row(s1.cpu(), t) * z
    assert torch.equal(res.target.cpu(), exp_t)
    front = engine.train_noise(z.to(cuda), sa, s1, t.to(cuda), noise.to(cuda), drop.to(cuda), target=True)
    assert torch.equal(front[7], res.target) and torch.equal(res.eps, before.eps)  # (the same network input)
    # the oracle: autograd through train_ref.forward on the v-target written out here
    ab = d_v._host[1][t - 1].view(-1, 1, 1, 1)
    z_noisy = torch.sqrt(ab) * z + torch.sqrt(1 - ab) * noise
    target = torch.sqrt(ab) * noise - torch.sqrt(1 - ab) * z
    keep = (~drop).float().unsqueeze(1)
    y_used, vals_used, mask_used = torch.where(drop, torch.zeros_like(classes), classes), vals * keep, mask * keep
    w = d_v.loss_weights(weighting, device="cpu")
    if weighting == "min_snr":
        assert float(w[t - 1].max()) < 1.0  # below 1 at small and at large t
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in unet_sd.items()}
    eps, gp = train_ref.forward(leaves, z_noisy, t, y_used, vals_used, mask_used)
    rloss = (w[t - 1] * ((eps - target) ** 2).mean(dim=(1, 2, 3))).mean() \
        + lam * train_ref.masked_geom_mse(gp, vals, mask_used)
    rloss.backward()
    e_loss = abs(float(res.loss.detach()) - float(rloss)) / float(rloss)
    worst = []
    for n in grads:
        gr = leaves[n].grad
        assert (grads[n] is None) == (gr is None), n
        if gr is not None:
            worst.append((rel(grads[n], gr), n))
    worst.sort(reverse=True)
    print(f"[v objective B={B} {hw}x{hw} {weighting}] loss rel = {e_loss:.3e}; worst gradient rel-L2:", worst[:3])
    assert e_loss <= LOSS_TOL, e_loss
    assert worst[0][0] <= GRAD_TOL, worst[:5]
    assert rel(res.loss.detach(), before.loss.detach()) > 1e-3  # another objective than eps-mode's


# ---- 8: the range guard -----------------------------------------------------------------------------------
@pytest.fixture
def unet_sd_overflow():
    return overflow_sd()


@pytest.mark.parametrize("source", ["host", "device"])
def test_range_guard_replays_in_fp32(cuda, unet_sd_overflow, source):
    m = make_model(cuda, unet_sd_overflow)
    d = dv(cuda, 8)
    d.noise_source = source
    g = torch.Generator().manual_seed(35)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    mask = torch.ones((2, 12), device=cuda)
    torch.manual_seed(36)
    lat = d.sample_latent_cond(m, {1: 1, 2: 1}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals,
                               cond_mask=mask, sampler="ddim", steps=4, eta=0.5)
    assert d.range_fallbacks == 1
    assert torch.isfinite(lat).all() and m.native().precision == "x3" and m.native().prediction == "v"
