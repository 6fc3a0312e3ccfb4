"""GPU: DPM-Solver++(2M) sampling — the fused update, one network step, trajectories, the graph loop,
solver accuracy and the public samplers — against a torch-CPU restatement of the update that takes
eps from the oracle (oracle.ref.unet_cond_geom_forward) and the tables from Diffuser.dpm_tables.

Position p = 1..S of a schedule stands for the timestep t_map[p-1]; the step at p uses table row p-1:
  x0 = (x - k_e eps)/k_a;  y = k_x x + k_c x0;  x' = y + k_p hist where k_p != 0, else y;  hist <- x0
(torch's evaluation order, fp32).  Bounds as in test_gpu_ddim.py.

Measured on an MI355X (rel-L2): steps against the oracle 1.2e-6 .. 1.8e-6; trajectories (a) 1.1e-6,
(b) 2.2e-6, (c) 1.9e-6; solver accuracy at S = 20 against the float64 full-stride solution:
dpmpp_2m/logsnr 1.805e-2, ddim 6.999e-2 (ratio 0.258), GPU against its fp32 CPU restatement 1.6e-7."""
import math

import numpy as np
import pytest
import torch

from oracle import ref, rules
from oracle.rules import Foreign, cfg_eps, ddim_update, dpm_update, rel
from support import make_model, make_vae, overflow_sd

pytestmark = pytest.mark.gpu

TOL = 2e-5        # one step (the project's step bound)
TRAJ_TOL = 1e-4   # a trajectory (the project's trajectory bound)


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    return make_model(cuda, unet_sd)


@pytest.fixture(scope="module")
def vae(cuda, vae_sd):
    return make_vae(cuda, vae_sd)


@pytest.fixture
def unet_sd_overflow():
    return overflow_sd()


# ---- 4: the update, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["logsnr", "uniform"])
def test_dpm_update_bit_exact(cuda, spacing):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    S = 7
    sched = d.dpm_tables(S, spacing, "cpu")
    dsched = d.dpm_tables(S, spacing, cuda)
    g = torch.Generator().manual_seed(9)
    B = 3
    pos = torch.tensor([S, 4, 1])  # first-order (no history yet), second-order, first-order (s = 0)
    for C in (4, 3):  # both go through the generic tail; 3 channels: the Co < 4 indexing
        x, eu, ec, hist = (torch.randn((B, C, 16, 16), generator=g) for _ in range(4))
        exp, exp_h = dpm_update(x, eu + 3.0 * (ec - eu), pos, sched, hist)
        h = hist.to(cuda)
        out = engine.dpm_update(x.to(cuda), eu.to(cuda), ec.to(cuda), 3.0, pos.to(cuda), dsched, h).cpu()
        assert torch.equal(out, exp) and torch.equal(h.cpu(), exp_h)
        # no CFG operand: eps = eu
        exp1, exp1_h = dpm_update(x, eu, pos, sched, hist)
        h = hist.to(cuda)
        out1 = engine.dpm_update(x.to(cuda), eu.to(cuda), None, 0.0, pos.to(cuda), dsched, h).cpu()
        assert torch.equal(out1, exp1) and torch.equal(h.cpu(), exp1_h)
        # hist is not read where k_p == 0: NaN there changes nothing at positions S and 1
        h = torch.full_like(x, float("nan")).to(cuda)
        outn = engine.dpm_update(x.to(cuda), eu.to(cuda), ec.to(cuda), 3.0, pos.to(cuda), dsched, h).cpu()
        assert torch.isfinite(outn[[0, 2]]).all() and torch.equal(outn[[0, 2]], exp[[0, 2]])
        assert torch.equal(h.cpu(), exp_h)  # always written
        # x_out may alias x
        xa, h = x.to(cuda), hist.to(cuda)
        res = engine.dpm_update(xa, eu.to(cuda), ec.to(cuda), 3.0, pos.to(cuda), dsched, h, out=xa)
        assert res.data_ptr() == xa.data_ptr()
        assert torch.equal(xa.cpu(), exp) and torch.equal(h.cpu(), exp_h)


def test_dpm_update_rejects_bad_history(cuda):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    sched = d.dpm_tables(7, "logsnr", cuda)
    x = torch.zeros((2, 4, 8, 8), device=cuda)
    pos = torch.tensor([7, 7], device=cuda)
    for bad in (None, x, torch.zeros((2, 4, 8, 4), device=cuda), torch.zeros((2, 4, 8, 8), device=cuda).double()):
        with pytest.raises(ValueError):
            engine.dpm_update(x, x, None, 0.0, pos, sched, bad)
    with pytest.raises(ValueError):  # a plain 6-tuple is a DDIM schedule
        engine.dpm_update(x, x, None, 0.0, pos, tuple(sched), torch.zeros_like(x))


# ---- 5: first-order rows are DDIM ------------------------------------------------------------------
def test_dpm_first_order_rows_are_ddim(cuda):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(50)
    B = 2
    x, eps = (torch.randn((B, 4, 16, 16), generator=g) for _ in range(2))
    nan = torch.full_like(x, float("nan"))
    pos = torch.tensor([2, 1])  # S = 2, "uniform": 1000 -> 500 and 500 -> 0
    got = engine.dpm_update(x.to(cuda), eps.to(cuda), None, 0.0, pos.to(cuda), d.dpm_tables(2, "uniform", cuda),
                            nan.to(cuda))
    ddim = engine.ddim_update(x.to(cuda), eps.to(cuda), None, 0.0, pos.to(cuda), d.ddim_tables(2, 0.0, cuda))
    err = rel(got, ddim)
    print(f"[dpm first-order rows vs ddim, GPU] rel-L2 = {err:.3e}")
    assert err <= 1e-6, err
    # The two formulas' fp32 CPU restatements differ by rounding only and are identical at s = 0.
    # (1000 -> 500), the row used above, stays within 8e-8.  (1000 -> 980) reads 8.1e-8 .. 8.6e-8 for
    # unit-normal draws (x0 is about 150 |eps| there and DDIM cancels two rounded products of that
    # size), so it is held to the 1e-6 of the GPU comparison; both figures are printed.
    for S, p, bound in ((2, 2, 8e-8), (50, 50, 1e-6)):
        pp = torch.full((B,), p)
        a, _ = dpm_update(x, eps, pp, d.dpm_tables(S, "uniform", "cpu"), nan)
        b = ddim_update(x, eps, pp, d.ddim_tables(S, 0.0, "cpu"))
        err = rel(a, b)
        print(f"[dpm first-order row vs ddim, CPU restatements, S={S} p={p}] rel-L2 = {err:.3e}")
        assert err <= bound, err
    for S in (2, 50):
        pp = torch.full((B,), 1)
        a, a0 = dpm_update(x, eps, pp, d.dpm_tables(S, "uniform", "cpu"), nan)
        assert torch.equal(a, ddim_update(x, eps, pp, d.ddim_tables(S, 0.0, "cpu"))) and torch.equal(a, a0)


# ---- 6: one network step against the oracle -----------------------------------------------------
_STEP_REF = {}


def step_ref(unet_sd, d, hw):
    """Inputs and the restatement of positions 4 then 3 (S = 7, "logsnr") fed oracle eps; once per size."""
    if hw not in _STEP_REF:
        g = torch.Generator().manual_seed(31 + hw)
        B = 2
        x = torch.randn((B, 4, hw, hw), generator=g)
        hist = torch.randn((B, 4, hw, hw), generator=g)  # stands for the x0 of position 5
        y = torch.tensor([1, 3])
        vals = torch.rand((B, 12), generator=g)
        mask = (torch.rand((B, 12), generator=g) > 0.4).float()
        sched = d.dpm_tables(7, "logsnr", "cpu")
        exp = []
        xr, hr = x, hist
        with torch.no_grad():
            for p in (4, 3):
                pos = torch.full((B,), p)
                xr, hr = dpm_update(xr, cfg_eps(unet_sd, xr, sched[0][pos - 1], y, vals, mask), pos, sched, hr)
                exp.append((xr, hr))
        _STEP_REF[hw] = (x, hist, y, vals, mask, exp)
    return _STEP_REF[hw]


@pytest.mark.parametrize("hw", [32, 28])
@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_dpm_step_vs_oracle(model, cuda, unet_sd, prec, hw):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    x, hist, y, vals, mask, exp = step_ref(unet_sd, d, hw)
    xs, h = x.to(cuda), hist.to(cuda)
    state = torch.get_rng_state()
    with model.native().precision_override(prec):
        for p, (ex, eh) in zip((4, 3), exp):  # position 3 reads the history that position 4 wrote
            pos = torch.full((x.shape[0],), p, device=cuda)
            xs = d.dpm_step(model, xs, pos, h, 7, "logsnr", y=y.to(cuda), guidance_scale=3.0,
                            cond_vals=vals.to(cuda), cond_mask=mask.to(cuda))
            ex_err, eh_err = rel(xs, ex), rel(h, eh)
            print(f"[dpm step {prec} {hw}x{hw} p={p}] rel-L2 vs oracle: x' {ex_err:.3e}, hist {eh_err:.3e}")
            assert ex_err <= TOL and eh_err <= TOL, (ex_err, eh_err)
    assert torch.equal(torch.get_rng_state(), state)  # nothing is drawn


def test_dpm_step_without_cfg_and_foreign_model(model, cuda, unet_sd):
    """guidance 0: one conditional forward; a duck-typed model takes the model-call + dmx_dpm_update
    path and lands on the same numbers."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(32)
    B = 2
    x, hist = (torch.randn((B, 4, 16, 16), generator=g) for _ in range(2))
    y = torch.tensor([2, 1])
    pos = torch.tensor([4, 6])
    sched = d.dpm_tables(7, "logsnr", "cpu")
    t = sched[0][pos - 1]

    with torch.no_grad():
        e_y, _ = ref.unet_cond_geom_forward(unet_sd, x, t, y)
        e_0, _ = ref.unet_cond_geom_forward(unet_sd, x, t, torch.zeros_like(y))
        e_cfg = e_0 + 3.0 * (e_y - e_0)
    outs = {}
    for name, mdl in (("native", model), ("foreign", Foreign(model))):
        for case, eps, kw in (("y", e_y, dict(y=y.to(cuda))), ("cfg", e_cfg, dict(y=y.to(cuda), guidance_scale=3.0))):
            h = hist.to(cuda)
            out = d.dpm_step(mdl, x.to(cuda), pos.to(cuda), h, 7, **kw)
            ex, eh = dpm_update(x, eps, pos, sched, hist)
            assert rel(out, ex) <= TOL and rel(h, eh) <= TOL, (name, case)
            outs[name, case] = (out, h)
    for case in ("y", "cfg"):
        assert rel(outs["foreign", case][0], outs["native", case][0]) <= TOL
        assert rel(outs["foreign", case][1], outs["native", case][1]) <= TOL


# ---- 7: trajectories against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("case,counts,hw,S,spacing,source", [
    ("a", {1: 1, 2: 1}, 16, 11, "logsnr", "device"),          # one 8-step graph launch + three one-step launches
    ("b", {1: 1, 3: 1}, 16, 8, "uniform", "host"),
    ("c", {1: 11, 2: 11, 3: 10}, 32, 4, "logsnr", "device"),  # the 64-sample batch class: Winograd convs
])
def test_dpm_trajectory_vs_oracle(model, cuda, unet_sd, case, counts, hw, S, spacing, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    B = sum(counts.values())
    y = torch.tensor([c for c, n in counts.items() for _ in range(n)])
    g = torch.Generator().manual_seed(60 + S)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    torch.manual_seed(61)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=3.0,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), sampler="dpmpp_2m", steps=S,
                               spacing=spacing)
    assert d.range_fallbacks == 0
    torch.manual_seed(61)
    x_T = torch.randn((B, 4, hw, hw))
    sched = d.dpm_tables(S, spacing, "cpu")
    exp = rules.trajectory(x_T, "dpm", sched, lambda x, t, pos: cfg_eps(unet_sd, x, t, y, vals, mask))
    err = rel(out, exp)
    print(f"[dpm trajectory {case}] B={B} {hw}x{hw} S={S} {spacing} {source}: rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err


# ---- 8: graph == eager, determinism, schedule and history are part of the graph key ---------------
@pytest.mark.parametrize("B", [4, 64])
def test_dpm_graph_loop_equals_eager_and_is_deterministic(model, cuda, B):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn((B, 4, 32, 32), generator=g).to(cuda)
    y = torch.tensor([1 + i % 3 for i in range(B)], device=cuda)
    vals = torch.rand((B, 12), generator=g).to(cuda)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(cuda) if B > 4 else torch.ones((B, 12), device=cuda)
    sched = d.dpm_tables(25, "logsnr", cuda)
    x = torch.empty_like(x0)  # ONE state buffer, ONE history and ONE position scalar for every loop below
    hist = torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(sched, start, steps, use_graph, hist=hist, tables=None):
        x.copy_(x0)
        t.fill_(start)
        kw = dict(sched=sched) if sched is not None else {}
        if hist is not None:
            hist.fill_(float("nan"))  # every DPM loop below starts at its position S: not read
            kw["hist"] = hist
        nm.sample_loop(x, t, y, 0, vals, mask, 3.0, tables, steps, seed=1234, use_graph=use_graph, **kw)
        torch.cuda.synchronize()
        assert int(t.item()) == start - steps
        return x.cpu(), (hist.cpu() if hist is not None else None)

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    outs = [loop(sched, 25, 19, ug) for ug in (True, False, True)]  # position 25 -> 6
    assert same(outs[0], outs[1]) and same(outs[0], outs[2])
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    if B == 4:
        a, b, h = x0.clone(), torch.empty_like(x0), torch.full_like(x0, float("nan"))
        for p in range(25, 6, -1):
            nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), y, 0, vals, mask, 3.0, None,
                    t_stride=0, sched=sched, hist=h)
            a, b = b, a
        assert torch.equal(a.cpu(), outs[0][0]) and torch.equal(h.cpu(), outs[0][1])
    # another DPM schedule on the same buffers: only the schedule tells its graphs from the ones above
    sched10 = d.dpm_tables(10, "logsnr", cuda)
    graph10 = loop(sched10, 10, 10, True)
    eager10 = loop(sched10, 10, 10, False)
    assert same(graph10, eager10) and not torch.equal(graph10[0], outs[0][0])
    # a DDIM loop and the DDPM loop on the same x and scalar are not confused with either
    ddim10 = d.ddim_tables(10, 0.0, cuda)
    assert torch.equal(loop(ddim10, 10, 10, True, hist=None)[0], loop(ddim10, 10, 10, False, hist=None)[0])
    tables = d.coef_tables(cuda, True)
    assert torch.equal(loop(None, 10, 10, True, hist=None, tables=tables)[0],
                       loop(None, 10, 10, False, hist=None, tables=tables)[0])
    assert same(loop(sched10, 10, 10, True), eager10)
    # another history buffer with the same tables: its own graphs; the first buffer is not touched
    before = hist.clone()
    hist2 = torch.empty_like(x0)
    other = loop(sched10, 10, 10, True, hist=hist2)
    assert same(other, eager10)
    assert torch.equal(hist.cpu(), before.cpu())


# ---- 9: solver accuracy on a closed-form problem (foreign-model path, no network) -----------------
MIX_W, MIX_MU, MIX_STD = (0.4, 0.6), (-1.0, 0.6), 0.25


def mixture_eps(x, ab_t):
    """eps of the per-element two-component Gaussian mixture at alpha = sqrt(ab_t), sigma = sqrt(1 - ab_t):
    sigma * sum_k r_k (x - alpha mu_k) / (alpha^2 std^2 + sigma^2), r = softmax responsibilities."""
    a, s = torch.sqrt(ab_t).view(-1, 1, 1, 1), torch.sqrt(1 - ab_t).view(-1, 1, 1, 1)
    var = a * a * MIX_STD ** 2 + s * s
    dk = torch.stack([x - a * mu for mu in MIX_MU])
    logit = torch.stack([math.log(w) - dk[k] ** 2 / (2 * var) for k, w in enumerate(MIX_W)])
    r = torch.softmax(logit, dim=0)
    return s * (r * dk).sum(0) / var


class MixtureModel(torch.nn.Module):  # duck-typed: no .native()
    def __init__(self, alpha_bars):
        super().__init__()
        self.ab = alpha_bars

    def forward(self, x, t, y, cond_vals=None, cond_mask=None):
        return mixture_eps(x, self.ab[t - 1])


def tables64(d, tau):
    """float64 DPM-Solver++(2M) tables of the ascending timesteps tau (the definitions, unrounded)."""
    S = len(tau)
    ab = torch.cat([torch.ones(1, dtype=torch.float64), d._host[1].double()])
    t = torch.tensor(tau)
    s = torch.tensor([0] + tau[:-1])
    k_e, k_a = torch.sqrt(1 - ab[t]), torch.sqrt(ab[t])
    k_x = torch.sqrt(1 - ab[s]) / k_e
    m = torch.sqrt(ab[s]) - k_x * k_a
    k_c, k_p = m.clone(), torch.zeros_like(m)
    lam = 0.5 * torch.log(ab / (1 - ab))  # lam[0] = inf, not used below
    for i in range(1, S - 1):
        r = (lam[t[i]] - lam[t[i + 1]]) / (lam[s[i]] - lam[t[i]])
        k_c[i], k_p[i] = m[i] * (1 + 1 / (2 * r)), -m[i] / (2 * r)
    return (t, k_e, k_a, k_x, k_c, k_p)


def solver_accuracy_cpu(d, x_T, S=20):
    """-> (float64 full-stride 2M reference, fp32 restatement of 2M/logsnr at S, fp32 restatement of DDIM at S)."""
    ab = d._host[1]
    fine = tables64(d, list(range(1, d.num_timesteps + 1)))
    ref64 = rules.trajectory(x_T.double(), "dpm", fine, lambda x, t, pos: mixture_eps(x, ab.double()[t - 1]))
    def eps32(x, t, pos):
        return mixture_eps(x, ab[t - 1])
    dpm32 = rules.trajectory(x_T, "dpm", d.dpm_tables(S, "logsnr", "cpu"), eps32)
    return ref64, dpm32, rules.trajectory(x_T, "ddim", d.ddim_tables(S, 0.0, "cpu"), eps32)


def test_dpm_solver_accuracy(cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    torch.manual_seed(9)
    x_T = torch.randn((4, 4, 8, 8))
    ref64, dpm32, ddim32 = solver_accuracy_cpu(d, x_T)
    cpu_dpm, cpu_ddim = rel(dpm32, ref64), rel(ddim32, ref64)
    print(f"[solver accuracy, CPU restatements S=20] dpmpp_2m/logsnr {cpu_dpm:.3e}, ddim {cpu_ddim:.3e}")
    assert cpu_dpm <= 0.5 * cpu_ddim  # the restatement alone meets the bar on this draw
    mdl = MixtureModel(d.alpha_bars)
    kw = dict(z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=0.0)
    torch.manual_seed(9)
    got = d.sample_latent_cond(mdl, {1: 4}, sampler="dpmpp_2m", steps=20, spacing="logsnr", **kw)
    torch.manual_seed(9)
    got_ddim = d.sample_latent_cond(mdl, {1: 4}, sampler="ddim", steps=20, eta=0.0, **kw)
    e_same, e_dpm, e_ddim = rel(got, dpm32), rel(got, ref64), rel(got_ddim, ref64)
    print(f"[solver accuracy, GPU S=20] dpmpp_2m/logsnr {e_dpm:.3e}, ddim {e_ddim:.3e}, ratio {e_dpm / e_ddim:.3f}; "
          f"GPU vs fp32 CPU restatement {e_same:.3e}")
    assert e_same <= TRAJ_TOL, e_same
    assert e_dpm <= 0.5 * e_ddim, (e_dpm, e_ddim)


# ---- 10: only x_T is drawn -------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
def test_dpm_draws_only_x_T(model, cuda, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    g = torch.Generator().manual_seed(90)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    mask = torch.ones((2, 12), device=cuda)
    outs = []
    for _ in range(2):
        torch.manual_seed(91)
        outs.append(d.sample_latent_cond(model, {2: 1, 3: 1}, z_shape=(4, 16, 16), vae=None, progress=False,
                                         cond=vals, cond_mask=mask, sampler="dpmpp_2m", steps=5).cpu())
        after = torch.get_rng_state()
        torch.manual_seed(91)
        torch.randn((2, 4, 16, 16))
        assert torch.equal(after, torch.get_rng_state())
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()


# ---- 11: the range guard's replay restores the history ---------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
def test_dpm_range_guard_replay_restores_history(cuda, unet_sd_overflow, source):
    import diff
    m = make_model(cuda, unet_sd_overflow)
    g = torch.Generator().manual_seed(35)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    mask = torch.ones((2, 12), device=cuda)

    def run():
        d = diff.Diffuser(8, device=cuda)
        d.noise_source = source
        d.GUARD_CHUNK = 3  # chunks 7..5, 4..2, 1: the second starts on a row that reads the history
        torch.manual_seed(36)
        lat = d.sample_latent_cond(m, {1: 1, 2: 1}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals,
                                   cond_mask=mask, sampler="dpmpp_2m", steps=7)
        return d, lat

    d, lat = run()
    assert d.range_fallbacks >= 1
    assert torch.isfinite(lat).all() and m.native().precision == "x3"
    with m.native().precision_override("fp32"):
        d32, lat32 = run()
    assert d32.range_fallbacks == 0
    err = rel(lat, lat32)
    print(f"[dpm range guard {source}] fallbacks {d.range_fallbacks}, rel-L2 vs the fp32 run = {err:.3e}")
    assert err <= TRAJ_TOL, err


# ---- 12: public paths ------------------------------------------------------------------------------
def test_dpm_sample_to_pil(model, vae, cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    torch.manual_seed(100)
    imgs = d.sample_latent_cond(model, {1: 1, 2: 1, 3: 1}, z_shape=(4, 16, 16), vae=vae, to_pil=True,
                                progress=False, sampler="dpmpp_2m", steps=4)
    assert len(imgs) == 3 and all(im.size == (128, 128) for im in imgs)


@pytest.mark.parametrize("source,spacing", [("host", None), ("device", "uniform")])
def test_dpm_sharded_world1_equals_diffuser(model, cuda, source, spacing):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    g = torch.Generator().manual_seed(101)
    vals = torch.rand((5, 12), generator=g).to(cuda)
    mask = (torch.rand((5, 12), generator=g) > 0.3).float().to(cuda)
    torch.manual_seed(102)
    lat = dd.ShardedCondSampler(d, model, None).sample({1: 3, 3: 2}, z_shape=(4, 16, 16), cond=vals, cond_mask=mask,
                                                       decode=False, sampler="dpmpp_2m", steps=8, spacing=spacing)
    s_sharded = torch.get_rng_state()
    torch.manual_seed(102)
    single = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals,
                                  cond_mask=mask, sampler="dpmpp_2m", steps=8, spacing=spacing)
    assert torch.equal(lat.cpu(), single.cpu()) and torch.isfinite(single).all()
    assert torch.equal(s_sharded, torch.get_rng_state())  # x_T and nothing else, in both


def test_dpm_entity_csv_sampler(model, vae, cuda):
    import os

    import diff
    from conftest import GOLDEN
    from entityCsvSampler import EntityCsvSampler
    csv = os.path.join(GOLDEN, "entities.csv")
    d = diff.Diffuser(1000, device=cuda)
    s = EntityCsvSampler(d, model, vae, class_id=1, base_wh=(400, 400), device=cuda)
    torch.manual_seed(110)
    imgs = s.sample(csv, count=2, start=1, guidance_scale=3.0, sampler="dpmpp_2m", steps=4)
    vals, mask = s.load_cond(csv, count=2, start=1)
    torch.manual_seed(110)
    exp = d.sample_latent_cond(model, (1, 2), vae=vae, guidance_scale=3.0, cond=vals, cond_mask=mask,
                               sampler="dpmpp_2m", steps=4, progress=False)
    assert len(imgs) == len(exp) == 2
    for a, b in zip(imgs, exp):
        assert a.size == b.size and np.array_equal(np.asarray(a), np.asarray(b))
