"""GPU: zero-terminal-SNR schedules and the x0-form of a v-model — the standalone conversion bit
for bit, one native step per rule (the terminal row included), the x0-form against the eps-form on an
ordinary schedule, trajectories, graphs, the combinations with every guidance form, training at t = T —
against the torch-CPU restatement of tests/rules_x0.py on top of the oracle's forwards.

The x0-rule of every step: oracle forward(s) -> the mix in output space -> the conversion, once,
    x0 = p_o[t-1] x_net - p_x[t-1] out,  eps = p_o[t-1] out + p_x[t-1] x_net
-> the update on (x0, eps), without a division.  Bounds are the project's (tests/test_gpu_vpred.py): 2e-5 for
one step, 1e-4 for a trajectory and for a gradient tensor, 2e-5 for the loss, rel-L2 against the fp32 oracle."""
import os

import pytest
import torch

import rules_x0
from oracle import ref, rules, train_ref
from oracle.rules import Foreign, cfg_eps, cfg_rescaled, composed_eps, invert_update, rel, row
from support import cond, device_noise, make_model, on

pytestmark = pytest.mark.gpu

TOL = 2e-5        # one step, and the two forms of one step against each other
TRAJ_TOL = 1e-4   # a trajectory
GRAD_TOL = 1e-4   # a gradient tensor
LOSS_TOL = 2e-5
G = 3.0
T = 50
S = 5
HW = 8


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


def dz(dev, n=T):
    """A v-diffuser on the rescaled schedule (x0-form follows)."""
    import diff
    return diff.Diffuser(n, device=dev, prediction="v", zero_terminal_snr=True)


def dv(dev, n=T, x0_form=False):
    import diff
    return diff.Diffuser(n, device=dev, prediction="v", x0_form=x0_form)


def split_of(d, out, x_net, t):
    return rules_x0.x0_split(out, x_net, t, *d.pred_tables("cpu"))


def x0_rules_of(d):
    return rules_x0.x0_rules(*d.pred_tables("cpu"), *d.x0_tables("cpu"))


# ---- 1: the standalone conversion, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 4, 16, 16), (6, 3, 16, 16), (5, 3, 9, 7)])
def test_pred_split_bit_exact(cuda, shape):
    from dmx import engine
    d = dz(cuda)
    B = shape[0]
    g = torch.Generator().manual_seed(13 + shape[1] + shape[2])
    out, x = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    t = torch.tensor([1, 2, T // 2, T - 1, T, 37][:B])
    assert 1 in t.tolist() and T in t.tolist()
    e_x0, e_eps = split_of(d, out, x, t)
    assert torch.equal(e_x0[t == T], -out[t == T]) and torch.equal(e_eps[t == T], x[t == T])  # pure noise: x0 = -v
    tabs = d.pred_tables(cuda)
    x0, eps = engine.pred_split(out.to(cuda), x.to(cuda), t.to(cuda), *tabs)
    assert torch.equal(x0.cpu(), e_x0) and torch.equal(eps.cpu(), e_eps)
    assert torch.equal(eps, engine.pred_to_eps(out.to(cuda), x.to(cuda), t.to(cuda), *tabs))
    # eps_out aliased onto out
    o = out.to(cuda)
    x0a, res = engine.pred_split(o, x.to(cuda), t.to(cuda), *tabs, inplace=True)
    assert res.data_ptr() == o.data_ptr() and torch.equal(o.cpu(), e_eps) and torch.equal(x0a.cpu(), e_x0)
    # a strided t, one value for every sample, and the clamp of the table reads
    wide = torch.full((2 * B,), 7, dtype=torch.long)
    wide[::2] = t
    ts = wide.to(cuda)[::2]
    assert ts.stride(0) == 2
    assert torch.equal(engine.pred_split(out.to(cuda), x.to(cuda), ts, *tabs)[0].cpu(), e_x0)
    one = engine.pred_split(out.to(cuda), x.to(cuda), torch.tensor([T], device=cuda), *tabs)
    assert torch.equal(one[0].cpu(), -out) and torch.equal(one[1].cpu(), x)
    far = engine.pred_split(out.to(cuda), x.to(cuda), torch.tensor([-3, 5000] * 3, device=cuda)[:B], *tabs)
    exp_far = split_of(d, out, x, torch.tensor([1, T] * 3)[:B])
    assert torch.equal(far[0].cpu(), exp_far[0]) and torch.equal(far[1].cpu(), exp_far[1])
    with pytest.raises(ValueError):
        engine.pred_split(out.to(cuda), x.to(cuda)[:, :1], t.to(cuda), *tabs)
    xa = x.to(cuda)
    with pytest.raises(ValueError):
        engine.pred_split(xa, xa, t.to(cuda), *tabs, inplace=True)


# ---- 2: one native step per rule against the oracle ------------------------------------------------------
B3 = 3
POS = [1, 3, S]
NOISE_SEED = 78
_REF = {}


def seeded_noise(shape):
    """The one randn(shape) a host-noise step draws after torch.manual_seed(NOISE_SEED)."""
    state = torch.get_rng_state()
    torch.manual_seed(NOISE_SEED)
    nz = torch.randn(tuple(shape))
    torch.set_rng_state(state)
    return nz


def step_inputs():
    g = torch.Generator().manual_seed(41)
    x = torch.randn((B3, 4, HW, HW), generator=g)
    other = 0.8 * torch.randn((B3, 4, HW, HW), generator=g)  # the DPM history
    y = torch.tensor([1, 3, 2])
    vals = torch.rand((B3, 12), generator=g)
    mask = (torch.rand((B3, 12), generator=g) > 0.4).float()
    return x, other, y, vals, mask, seeded_noise(x.shape)


RULES = ["ddpm", "ddim0", "ddim1", "dpm"]


def rule_case(d, rule):
    """-> (pos as the rule counts it, the network timesteps, the CPU tables)."""
    n = int(d.num_timesteps)
    if rule == "ddpm":
        t = torch.tensor([1, n // 2, n])
        return t, t, None
    sched = d.dpm_tables(S, "logsnr", "cpu") if rule == "dpm" else d.ddim_tables(S, float(rule[-1]), "cpu")
    pos = torch.tensor(POS)
    assert int(sched[0][S - 1]) == n  # position S is the terminal row
    return pos, sched[0][pos - 1], sched


def mixed_out(sd, d, rule):
    """The oracle's CFG-mixed output at the rule's three rows, once per (schedule, rule)."""
    key = ("out", int(d.num_timesteps), d.zero_terminal_snr, rule)
    if key not in _REF:
        x, other, y, vals, mask, nz = step_inputs()
        _, t, _ = rule_case(d, rule)
        _REF[key] = cfg_eps(sd, x, t, y, vals, mask, G)
    return _REF[key]


def step_ref(sd, d, rule):
    """The x0-rule of one step on the CPU -> (x', history afterwards or None, x0)."""
    x, other, y, vals, mask, nz = step_inputs()
    pos, t, sched = rule_case(d, rule)
    x0, eps = split_of(d, mixed_out(sd, d, rule), x, t)
    if rule == "ddpm":
        return rules_x0.ddpm_x0_update(x0, eps, t, *d.x0_tables("cpu"), d.coef_tables("cpu")[2], nz), None, x0
    if rule == "dpm":
        out, h = rules_x0.dpm_x0_update(x, x0, pos, sched, other)
        return out, h, x0
    return rules_x0.ddim_x0_update(x0, eps, pos, sched, nz), None, x0


def run_step(d, mdl, cuda, rule):
    """One public step of `rule` on the GPU -> (x', history afterwards or None)."""
    x, other, y, vals, mask, nz = step_inputs()
    pos = rule_case(d, rule)[0]
    xd, yd, vd, md, pd = on(cuda, x, y, vals, mask, pos)
    kw = dict(y=yd, guidance_scale=G, cond_vals=vd, cond_mask=md)
    if rule == "dpm":
        h = other.to(cuda)
        return d.dpm_step(mdl, xd, pd, h, S, **kw), h
    torch.manual_seed(NOISE_SEED)  # host noise: the step draws one randn(x.shape) where it draws at all
    if rule == "ddpm":
        return d.denoise_cond(mdl, xd, pd, **kw), None
    return d.ddim_step(mdl, xd, pd, S, eta=float(rule[-1]), **kw), None


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("rule", RULES)
def test_step_vs_oracle(model, cuda, unet_sd, rule, prec):
    """A wrong row, a wrong x_net, or d_s and d_d swapped is an O(1) error here; the terminal row (t = T,
    ab = 0) is among the three and is finite."""
    d = dz(cuda)
    exp, exp_h, _ = step_ref(unet_sd, d, rule)
    assert torch.isfinite(exp).all()
    with model.native().precision_override(prec):
        out, h = run_step(d, model, cuda, rule)
    nm = model.native()
    assert nm.prediction == "v" and nm.x0_form
    assert torch.isfinite(out).all()
    err = rel(out, exp)
    per_row = [rel(out[i], exp[i]) for i in range(B3)]
    print(f"[x0 step {rule} {prec}] rel-L2 vs oracle = {err:.3e}, per row {['%.2e' % e for e in per_row]}")
    assert err <= TOL and max(per_row) <= TOL, (err, per_row)
    if exp_h is not None:  # the history after the step is the restated x0
        eh = rel(h, exp_h)
        print(f"[x0 step {rule} {prec}] history rel-L2 = {eh:.3e}")
        assert torch.isfinite(h).all() and eh <= TOL, eh


@pytest.mark.parametrize("rule", RULES)
def test_x0_form_agrees_with_eps_form_on_an_ordinary_schedule(model, cuda, rule):
    """Same weights, same noise, one step of each rule at the three positions: the two forms are the same map
    of (x, v) up to their fp32 rounding (each within 1.1e-5 of float64: DESIGN §6u, §6x)."""
    d_e, d_x = dv(cuda), dv(cuda, x0_form=True)
    a, ha = run_step(d_e, model, cuda, rule)
    assert not model.native().x0_form
    b, hb = run_step(d_x, model, cuda, rule)
    assert model.native().x0_form
    err = rel(b, a)
    print(f"[x0-form vs eps-form {rule}] rel-L2 = {err:.3e}")
    assert 0.0 < err <= TOL or torch.equal(a, b), err
    if ha is not None:
        assert rel(hb, ha) <= TOL
    c, _ = run_step(d_e, model, cuda, rule)
    assert torch.equal(a, c) and not model.native().x0_form  # and back: the eps-form's bits


def test_foreign_model_is_refused(model, cuda):
    d = dz(cuda)
    x, other, y, vals, mask, nz = on(cuda, *step_inputs())
    pos = torch.tensor(POS, device=cuda)
    with pytest.raises(TypeError):
        d.ddim_step(Foreign(model), x, pos, S, y=y, guidance_scale=G, cond_vals=vals, cond_mask=mask)
    with pytest.raises(TypeError):
        d.denoise_cond(Foreign(model), x, pos, y=y, guidance_scale=G, cond_vals=vals, cond_mask=mask)


# ---- 3: trajectories -----------------------------------------------------------------------------------
def traj_tables(d, mode):
    if mode is None:
        return "ddpm", (d._host[0] * 0, d._host[0], d._host[1])  # (betas unused, alphas, alpha_bars: the Diffuser's own)
    if mode[0] == "ddim":
        return "ddim", d.ddim_tables(mode[1], mode[2], "cpu")
    return "dpm", d.dpm_tables(mode[1], mode[2], "cpu")


def sample_vs_oracle(model, cuda, sd, n, hw, kw, source, seed, extra=None, out_of=None, tag=""):
    d = dz(cuda, n)
    d.noise_source = source
    B, counts = 2, {1: 1, 3: 1}
    y = torch.tensor([1, 3])
    _, vals, mask = cond(B, seed)
    mode = d._sampler_mode(kw.get("sampler", "ddpm"), kw.get("steps"), kw.get("eta", 0.0), kw.get("spacing"), n)
    tau = d._mode_timesteps(mode)
    assert tau[-1] == n  # every sampler starts at the pure-noise step
    torch.manual_seed(seed + 1)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=G,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), **kw, **(extra or {}))
    assert d.range_fallbacks == 0 and torch.isfinite(out).all()
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
    with x0_rules_of(d):
        exp = rules.trajectory(x, *traj_tables(d, mode), lambda x, t, pos: out_of(x, t), noise_of)
    err = rel(out, exp)
    print(f"[x0 trajectory {tag or kw} {hw}x{hw} {source}] rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err
    return out


@pytest.mark.parametrize("case,n,hw,kw,source", [
    ("ddpm20", 20, HW, dict(), "host"),
    ("ddpm20", 20, HW, dict(), "device"),
    ("ddim5-eta0", T, HW, dict(sampler="ddim", steps=S, eta=0.0), "device"),
    ("ddim5-eta1", T, HW, dict(sampler="ddim", steps=S, eta=1.0), "host"),
    ("dpm5-logsnr", T, HW, dict(sampler="dpmpp_2m", steps=S, spacing="logsnr"), "device"),
    ("dpm5-uniform", T, HW, dict(sampler="dpmpp_2m", steps=S, spacing="uniform"), "host"),
    ("ddim3-28", T, 28, dict(sampler="ddim", steps=3, eta=1.0), "device"),
])
def test_trajectory_vs_oracle(model, cuda, unet_sd, case, n, hw, kw, source):
    sample_vs_oracle(model, cuda, unet_sd, n, hw, kw, source, 160 + hw + len(case), tag=case)


def test_unconditional_unet_sample_latent(unet3, unet3_sd, cuda):
    """The 3-channel Unet through sample_latent / denoise: the generic tail on a feature map, every step of a
    short schedule, alpha_bar_prev clamped at t = 1 (no wrap-around in x0-form)."""
    n, shape = 6, (2, 3, HW, HW)
    d = dz(cuda, n)
    torch.manual_seed(171)
    out = d.sample_latent(unet3, z_shape=shape, vae=None, progress=False)
    torch.manual_seed(171)
    x = torch.randn(shape)
    with x0_rules_of(d):
        exp = rules.trajectory(x, *traj_tables(d, None), lambda x, t, pos: ref.unet_forward(unet3_sd, x, t),
                               lambda p: torch.randn(shape))
    err = rel(out, exp)
    print(f"[x0 sample_latent unet3 T={n}] rel-L2 vs oracle = {err:.3e}")
    assert torch.isfinite(out).all() and err <= TRAJ_TOL, err
    # one denoise step at t = T and t = 1 alone
    t = torch.tensor([n, 1])
    torch.manual_seed(NOISE_SEED)
    got = d.denoise(unet3, x.to(cuda), t.to(cuda))
    with torch.no_grad():
        x0, eps = split_of(d, ref.unet_forward(unet3_sd, x, t), x, t)
    one = rules_x0.ddpm_x0_update(x0, eps, t, *d.x0_tables("cpu"), d.coef_tables("cpu")[2], seeded_noise(shape))
    assert rel(got, one) <= TOL

    class Wrapped(torch.nn.Module):
        def forward(self, x, t):
            return unet3(x, t)
    with pytest.raises(TypeError):
        d.denoise(Wrapped(), x.to(cuda), t.to(cuda))


# ---- 4: graphs ------------------------------------------------------------------------------------------
def test_graph_loop_equals_eager_and_follows_the_form(cuda, unet_sd):
    from dmx._lib import DMX_E_ARG, DmxError
    model = make_model(cuda, unet_sd)  # graph slots of its own
    nm = model.native()
    d_v, d_x = dv(cuda), dz(cuda)
    B, P, steps = 4, 25, 11  # one 8-step graph launch and three one-step launches
    g = torch.Generator().manual_seed(2)
    x_start = torch.randn((B, 4, 16, 16), generator=g).to(cuda)
    y, vals, mask = on(cuda, *cond(B, 3))
    sched = {id(d_v): d_v.ddim_tables(P, 1.0, cuda), id(d_x): d_x.ddim_tables(P, 1.0, cuda)}
    x = torch.empty_like(x_start)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(d, use_graph):
        d._set_prediction(nm)
        x.copy_(x_start)
        t.fill_(P)  # (position P: the terminal row of the rescaled schedule)
        nm.sample_loop(x, t, y, 0, vals, mask, G, None, steps, seed=1234, use_graph=use_graph, sched=sched[id(d)])
        torch.cuda.synchronize()
        assert int(t.item()) == P - steps
        return x.cpu()

    c0 = nm.graph_captures()
    v1 = loop(d_v, True)
    c1 = nm.graph_captures()
    z2 = loop(d_x, True)
    c2 = nm.graph_captures()
    assert nm.x0_form and nm.prediction == "v"
    v3 = loop(d_v, True)
    c3 = nm.graph_captures()
    assert not nm.x0_form and nm.prediction == "v"
    assert c0 < c1 < c2 < c3, (c0, c1, c2, c3)  # every switch drops the graphs
    assert torch.equal(v1, v3) and torch.isfinite(v1).all()
    z_eager = loop(d_x, False)
    assert torch.equal(z2, z_eager) and torch.isfinite(z2).all() and not torch.equal(z2, v1)
    assert torch.equal(loop(d_x, True), z2)
    c4 = nm.graph_captures()
    assert torch.equal(loop(d_x, True), z2) and nm.graph_captures() == c4  # the same setting again: a replay
    # eager one-step calls walk the same numbers
    a, b = x_start.clone(), torch.empty_like(x_start)
    for p in range(P, P - steps, -1):
        nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), y, 0, vals, mask, G, None, seed=1234,
                t_stride=0, sched=sched[id(d_x)])
        a, b = b, a
    assert torch.equal(a.cpu(), z2)
    # an x0-form schedule that names a timestep above the stored T is refused before anything runs
    dz(cuda, 12)._set_prediction(nm)
    assert nm.x0_form
    x.copy_(x_start)
    t.fill_(P)
    with pytest.raises(DmxError) as why:
        nm.sample_loop(x, t, y, 0, vals, mask, G, None, 2, seed=1234, sched=sched[id(d_x)])
    assert why.value.code == DMX_E_ARG
    with pytest.raises(DmxError):
        nm.step(x_start, torch.empty_like(x_start), torch.full((1,), P, dtype=torch.long, device=cuda), y, 0, vals,
                mask, G, None, seed=1234, t_stride=0, sched=sched[id(d_x)])
    torch.cuda.synchronize()
    assert torch.equal(x, x_start) and int(t.item()) == P


# ---- 5: combinations ---------------------------------------------------------------------------------------
def test_rescale_also_and_pag(model, cuda, unet_sd):
    """The precomputed-output tail (CFG rescale, the paper's companion setting) and the composed tail (K = 2; the
    perturbed branch), each from the pure-noise step."""
    def rescaled(d, y, vals, mask):
        def f(x, t):
            with torch.no_grad():
                ec, _ = ref.unet_cond_geom_forward(unet_sd, x, t, y, vals, mask)
                eu, _ = ref.unet_cond_geom_forward(unet_sd, x, t, torch.zeros_like(y), vals, mask)
            return cfg_rescaled(eu, ec, G, 0.7)
        return f
    sample_vs_oracle(model, cuda, unet_sd, T, HW, dict(sampler="dpmpp_2m", steps=3), "device", 71,
                     dict(guidance_rescale=0.7), rescaled, "rescale dpm")
    sample_vs_oracle(model, cuda, unet_sd, T, HW, dict(sampler="ddim", steps=2, eta=0.0), "device", 71,
                     dict(guidance_rescale=0.7), rescaled, "rescale ddim")
    _, v2, m2 = cond(2, 81)
    also = [dict(classes=[2, 1], cond=v2, cond_mask=m2, weight=[1.5, -0.5])]

    def composed(d, y, vals, mask):
        comp = d._compose_args(y.tolist(), vals, mask, G, "null", also, device="cpu")
        assert comp[0].shape[0] == 3  # K = 2
        return lambda x, t: composed_eps(unet_sd, x, t, comp)
    sample_vs_oracle(model, cuda, unet_sd, T, HW, dict(sampler="ddim", steps=3, eta=1.0), "device", 82,
                     dict(also=also), composed, "also K=2 ddim")
    sample_vs_oracle(model, cuda, unet_sd, 4, HW, dict(), "host", 82, dict(also=also), composed, "also K=2 ddpm")
    sample_vs_oracle(model, cuda, unet_sd, T, HW, dict(sampler="dpmpp_2m", steps=2), "host", 82, dict(also=also),
                     composed, "also K=2 dpm")

    def pag(d, y, vals, mask):
        comp, pt = d._pag_args(2.0, ("sa3",), y.tolist(), vals, mask, G)
        return lambda x, t: composed_eps(unet_sd, x, t, comp, pt)
    sample_vs_oracle(model, cuda, unet_sd, T, HW, dict(sampler="ddim", steps=2, eta=0.0), "device", 91,
                     dict(pag_scale=2.0), pag, "pag")


def test_geom_step_is_unsteered_at_pure_noise(model, cuda, unet_sd):
    """eu / ec from the oracle, dL/dx from the GPU's own geom_grad (test_gpu_geom.py bounds it): the terminal row
    has sig = 0 and is the unguided step; the position below it shows v += s (k_e / k_a) dL/dx."""
    d = dz(cuda)
    x, other, y, vals, mask, nz = step_inputs()
    pos = torch.tensor([S, S - 1, 1])
    sched = d.ddim_tables(S, 0.0, "cpu")
    t = sched[0][pos - 1]
    scale = torch.full((B3,), 400.0)  # (large enough for the gradient's share of the second row's step to show)
    plan = d._plan(x.to(cuda), ("ddim", S, 0.0), G, geom=scale)
    sig = plan.geom[1].cpu()
    assert torch.isfinite(sig).all() and float(sig[S - 1]) == 0.0
    assert torch.equal(sig[:S - 1], (sched[1] / sched[2])[:S - 1]) and float(sig[S - 2]) > 1.0
    grad = model.geom_grad(*on(cuda, x, t, y, vals, mask))[1].cpu()
    out_g = cfg_eps(unet_sd, x, t, y, vals, mask)
    mixed = out_g + (scale * sig[pos - 1]).view(-1, 1, 1, 1) * grad

    def upd(o):
        x0, eps = split_of(d, o, x, t)
        return rules_x0.ddim_x0_update(x0, eps, pos, sched, None)

    exp, plain = upd(mixed), upd(out_g)
    assert torch.equal(exp[0], plain[0])  # the terminal row is not steered
    share = float((exp[1] - plain[1]).norm() / exp[1].norm())
    assert share >= 0.05, share
    out = torch.empty(x.shape, device=cuda)
    nm = d._native(model)
    nm.step(x.to(cuda), out, pos.to(cuda), y.to(cuda), 0, vals.to(cuda), mask.to(cuda), G, plan.tables, nz.to(cuda),
            **plan.kwargs(True))
    err = rel(out, exp)
    print(f"[x0 geom step] rel-L2 vs restatement = {err:.3e}, share at the second position = {share:.3f}")
    assert torch.isfinite(out).all() and err <= TOL, err
    assert rel(out[1], plain[1]) > 10 * TOL  # the second position is steered
    # the sampler's keyword, from the pure-noise step
    d.noise_source = "device"
    torch.manual_seed(5)
    lat = d.sample_latent_cond(model, {1: 1, 2: 1}, z_shape=(4, HW, HW), vae=None, progress=False, guidance_scale=G,
                               cond=vals[:2].to(cuda), cond_mask=mask[:2].to(cuda), sampler="dpmpp_2m", steps=3,
                               geom_scale=5.0)
    assert torch.isfinite(lat).all()


def test_init_latent_and_mask_at_full_strength(model, cuda):
    d = dz(cuda)
    d.noise_source = "device"
    B = 2
    _, vals, mask = cond(B, 101)
    g = torch.Generator().manual_seed(102)
    z0 = 0.8 * torch.randn((B, 4, HW, HW), generator=g)
    m = torch.zeros((B, 1, HW, HW))
    m[0, :, 2:6, 1:5] = 1.0
    m[1, :, 3:7, 2:8] = 1.0
    m[1, :, 1, :] = 0.25
    for kw in (dict(sampler="ddim", steps=4), dict(sampler="dpmpp_2m", steps=4), dict()):
        dd = d if kw else dz(cuda, 6)
        dd.noise_source = "device"
        torch.manual_seed(103)
        out = dd.sample_latent_cond(model, {1: 1, 3: 1}, vae=None, progress=False, guidance_scale=G,
                                    cond=vals.to(cuda), cond_mask=mask.to(cuda), init_latent=z0, mask=m, strength=1.0,
                                    **kw)
        keep = (m == 0).expand_as(z0)
        assert torch.isfinite(out).all()
        assert torch.equal(out.cpu()[keep], z0[keep])  # kept pixels: z0's bits
        assert not torch.equal(out.cpu()[~keep], z0[~keep])


def test_cache_interval(model, cuda, unet_sd):
    d = dz(cuda)
    nm = d._native(model)
    x, other, y, vals, mask, nz = on(cuda, *step_inputs())
    sched = d.ddim_tables(S, 1.0, cuda)
    pos = torch.tensor([S, 3, 2], device=cuda)
    outs = []
    for cache in (None, (2, 0), (2, 2)):  # a refresh step is the plain x0-form step
        out = torch.empty_like(x)
        nm.step(x, out, pos, y, 0, vals, mask, G, None, nz, sched=sched, **({} if cache is None else dict(cache=cache)))
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.isfinite(outs[0]).all()
    reuse = torch.empty_like(x)
    nm.step(x, reuse, pos - 1, y, 0, vals, mask, G, None, nz, sched=sched, cache=(2, 1))
    assert torch.isfinite(reuse).all()
    d.noise_source = "device"
    torch.manual_seed(7)
    lat = d.sample_latent_cond(model, {1: 1, 2: 1}, z_shape=(4, HW, HW), vae=None, progress=False, cond=vals[:2],
                               cond_mask=mask[:2], sampler="ddim", steps=4, cache_interval=2)
    assert torch.isfinite(lat).all() and nm.x0_form


def test_invert_then_start_latent(model, cuda, unet_sd):
    """Inversion has no x0 and no division: it converts as a v-model does, up to the pure-noise step (where
    y = eps); sampling back from there is the x0-form's."""
    d = dz(cuda)
    B, Si, R = 2, 3, 1
    counts = {1: 1, 3: 1}
    y = torch.tensor([1, 3])
    _, vals, mask = cond(B, 111)
    g = torch.Generator().manual_seed(112)
    z0 = 0.8 * torch.randn((B, 4, HW, HW), generator=g)
    kw = dict(guidance_scale=G, cond=vals.to(cuda), cond_mask=mask.to(cuda))
    lat = d.invert_latent_cond(model, z0, counts, steps=Si, refine=R, **kw)
    assert not model.native().x0_form or model.native().prediction == "v"
    back = d.sample_latent_cond(model, counts, vae=None, progress=False, sampler="ddim", steps=Si, start_latent=lat, **kw)
    assert torch.isfinite(lat).all() and torch.isfinite(back).all()
    tables, sched = d.invert_tables(Si, None, R, "cpu"), d.ddim_tables(Si, 0.0, "cpu")
    p_o, p_x = d.pred_tables("cpu")
    x, src = z0, z0
    for c in range(int(tables[0].numel()), 0, -1):
        pos = torch.full((B,), c, dtype=torch.long)
        t = tables[0][pos - 1]
        x, src = invert_update(src, rules.to_eps(cfg_eps(unet_sd, x, t, y, vals, mask), x, t, p_o, p_x), pos, tables)
    e_inv = rel(lat, x)
    with x0_rules_of(d):
        xb = rules.trajectory(x, "ddim", sched, lambda x, t, pos: cfg_eps(unet_sd, x, t, y, vals, mask))
    e_back = rel(back, xb)
    print(f"[x0 invert S={Si} R={R}] rel-L2 vs restatement: inverted {e_inv:.3e}, sampled back {e_back:.3e}")
    assert e_inv <= TRAJ_TOL and e_back <= TRAJ_TOL, (e_inv, e_back)


# ---- 6: training ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", ["uniform", "min_snr"])
def test_training_loss_at_pure_noise(cuda, unet_sd, weighting):
    """No kernel changes: at t = T the noising gives z_t = noise and the target is v = -z."""
    model = make_model(cuda, unet_sd).train()
    d = dz(cuda)
    B, lam = 3, 0.5
    g = torch.Generator().manual_seed(31)
    z, noise = torch.randn((B, 4, HW, HW), generator=g), torch.randn((B, 4, HW, HW), generator=g)
    classes = torch.randint(1, 4, (B,), generator=g)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    t = torch.tensor([T, 20, 1])
    drop = torch.tensor([False, False, True])
    zc, nc, cc, vc, mc, tc, dc = on(cuda, z, noise, classes, vals, mask, t, drop)
    model.zero_grad(set_to_none=True)
    res = d.training_loss(model, zc, cc, vc, mc, geom_lambda=lam, weighting=weighting, t=tc, noise=nc, drop=dc)
    res.loss.backward()
    grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()}
    sa, s1 = (k.cpu() for k in d.noise_tables(cuda))  # (the noising's tables: torch's roots on the device)
    assert float(sa[T - 1]) == 0.0 and float(s1[T - 1]) == 1.0
    exp_t = row(sa, t) * noise - row(s1, t) * z
    assert torch.equal(res.target.cpu(), exp_t) and torch.equal(res.target[0].cpu(), -z[0])
    z_noisy = row(sa, t) * z + row(s1, t) * noise
    assert torch.equal(z_noisy[0], noise[0])
    keep = (~drop).float().unsqueeze(1)
    y_used, vals_used, mask_used = torch.where(drop, torch.zeros_like(classes), classes), vals * keep, mask * keep
    w = d.loss_weights(weighting, device="cpu")
    assert float(w[T - 1]) == (1.0 if weighting == "uniform" else 0.0)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in unet_sd.items()}
    eps, gp = train_ref.forward(leaves, z_noisy, t, y_used, vals_used, mask_used)
    rloss = (w[t - 1] * ((eps - exp_t) ** 2).mean(dim=(1, 2, 3))).mean() + lam * train_ref.masked_geom_mse(gp, vals, mask_used)
    rloss.backward()
    e_loss = abs(float(res.loss.detach()) - float(rloss)) / float(rloss)
    worst = []
    for n in grads:
        gr = leaves[n].grad
        assert (grads[n] is None) == (gr is None), n
        if gr is not None:
            worst.append((rel(grads[n], gr), n))
    worst.sort(reverse=True)
    print(f"[x0 objective {weighting}] loss rel = {e_loss:.3e}; worst gradient rel-L2:", worst[:3])
    assert torch.isfinite(res.loss) and e_loss <= LOSS_TOL, e_loss
    assert worst[0][0] <= GRAD_TOL, worst[:5]
