"""GPU: strided (DDIM) sampling — the fused update, one network step, trajectories, the graph
loop and the public samplers — against a torch-CPU restatement of the update that takes eps from
the oracle (oracle.ref.unet_cond_geom_forward) and the tables from Diffuser.ddim_tables.

Position p = 1..S of a schedule stands for the timestep t_map[p-1]; the step at p uses table row
p-1:  x0 = (x - k_e eps)/k_a;  x' = k_s x0 + k_d eps + k_n noise  (torch's evaluation order, fp32)."""
import pytest
import torch

from oracle import ref, rules
from oracle.rules import Foreign, cfg_eps, ddim_update, rel
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


# ---- 4: the update, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_update_bit_exact(cuda, eta):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    sched = d.ddim_tables(50, eta, "cpu")
    dsched = d.ddim_tables(50, eta, cuda)
    g = torch.Generator().manual_seed(9)
    B = 6
    pos = torch.tensor([1, 2, 3, 25, 49, 50])
    for C in (4, 3):  # both go through the generic tail; 3 channels: the Co < 4 indexing
        x, eu, ec, nz = (torch.randn((B, C, 16, 16), generator=g) for _ in range(4))
        out = engine.ddim_update(x.to(cuda), eu.to(cuda), ec.to(cuda), 3.0, pos.to(cuda), dsched, nz.to(cuda)).cpu()
        assert torch.equal(out, ddim_update(x, eu + 3.0 * (ec - eu), pos, sched, nz))
        out = engine.ddim_update(x.to(cuda), eu.to(cuda), None, 0.0, pos.to(cuda), dsched, nz.to(cuda)).cpu()
        assert torch.equal(out, ddim_update(x, eu, pos, sched, nz))
    if eta == 0.0:  # no noise anywhere: nothing is read or drawn, given or not
        out2 = engine.ddim_update(x.to(cuda), eu.to(cuda), None, 0.0, pos.to(cuda), dsched, None, seed=5).cpu()
        assert torch.equal(out2, out)


def test_ddim_update_device_noise_keyed_by_timestep(cuda):
    """Philox noise of the strided update: absent at position 1, keyed by the network timestep (the
    DDPM update at t = tau draws the same normals) and shard-invariant through sample_offset."""
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    sched = d.ddim_tables(50, 1.0, cuda)
    B = 8
    x = torch.zeros((B, 4, 32, 32), device=cuda)
    pos = torch.tensor([1, 2, 2, 7, 7, 50, 50, 50], device=cuda)
    full = engine.ddim_update(x, x, None, 0.0, pos, sched, None, seed=99)
    part = engine.ddim_update(x[4:], x[4:], None, 0.0, pos[4:], sched, None, seed=99, sample_offset=4)
    assert torch.equal(full[4:], part)
    assert float(full[0].abs().max()) == 0.0 and float(full[1].abs().max()) > 0.0
    tab = d.coef_tables(cuda, True)
    t = sched[0][pos - 1]
    ddpm = engine.ddpm_update(x, x, None, 0.0, t, tab, None, seed=99)  # x = eps = 0: noise * sd[t-1]
    z_ddim = full[1:] / sched[5][pos[1:] - 1].view(-1, 1, 1, 1)
    z_ddpm = ddpm[1:] / tab[2][t[1:] - 1].view(-1, 1, 1, 1)
    assert rel(z_ddim, z_ddpm) < 1e-6  # the same normals up to the two roundings of * k / k


# ---- 5: one network step against the oracle -----------------------------------------------------
@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_ddim_step_vs_oracle(model, cuda, unet_sd, prec):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(31)
    B = 3
    x = torch.randn((B, 4, 32, 32), generator=g)
    y = torch.tensor([1, 3, 2])
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.4).float()
    pos = torch.tensor([1, 25, 50])
    with model.native().precision_override(prec):
        torch.manual_seed(78)
        out = d.ddim_step(model, x.to(cuda), pos.to(cuda), 50, eta=0.5, y=y.to(cuda), guidance_scale=3.0,
                          cond_vals=vals.to(cuda), cond_mask=mask.to(cuda))
        after = torch.get_rng_state()
    torch.manual_seed(78)
    noise = torch.randn(x.shape)
    assert torch.equal(after, torch.get_rng_state())  # one randn(x.shape) per call
    sched = d.ddim_tables(50, 0.5, "cpu")
    with torch.no_grad():
        exp = ddim_update(x, cfg_eps(unet_sd, x, sched[0][pos - 1], y, vals, mask), pos, sched, noise)
    err = rel(out, exp)
    print(f"[ddim step {prec}] rel-L2 vs oracle = {err:.3e}")
    assert err < TOL, err


def test_ddim_step_without_cfg_and_foreign_model(model, cuda, unet_sd):
    """guidance 0: one conditional forward (y defaults to null_label); a duck-typed model takes the
    model-call + dmx_ddim_update path and lands on the same numbers."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(32)
    B = 2
    x = torch.randn((B, 4, 16, 16), generator=g)
    y = torch.tensor([2, 1])
    pos = torch.tensor([4, 7])
    sched = d.ddim_tables(7, 0.0, "cpu")
    t = sched[0][pos - 1]

    with torch.no_grad():
        e_y, _ = ref.unet_cond_geom_forward(unet_sd, x, t, y)
        e_0, _ = ref.unet_cond_geom_forward(unet_sd, x, t, torch.zeros_like(y))
        e_cfg = e_0 + 3.0 * (e_y - e_0)
    zero = torch.zeros_like(x)
    for mdl in (model, Foreign(model)):
        out = d.ddim_step(mdl, x.to(cuda), pos.to(cuda), 7, y=y.to(cuda))
        assert rel(out, ddim_update(x, e_y, pos, sched, zero)) < TOL
        out = d.ddim_step(mdl, x.to(cuda), pos.to(cuda), 7)
        assert rel(out, ddim_update(x, e_0, pos, sched, zero)) < TOL
        out = d.ddim_step(mdl, x.to(cuda), pos.to(cuda), 7, y=y.to(cuda), guidance_scale=3.0)
        assert rel(out, ddim_update(x, e_cfg, pos, sched, zero)) < TOL


# ---- 6: trajectories against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("case,counts,hw,S,eta,source", [
    ("a", {1: 1, 2: 1}, 16, 11, 0.0, "device"),            # one 8-step graph launch + three one-step launches
    ("b", {1: 1, 3: 1}, 16, 8, 0.5, "host"),
    ("c", {1: 11, 2: 11, 3: 10}, 32, 4, 0.0, "device"),    # the 64-sample batch class: Winograd convs
])
def test_ddim_trajectory_vs_oracle(model, cuda, unet_sd, case, counts, hw, S, eta, source):
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
                               cond=vals.to(cuda), cond_mask=mask.to(cuda), sampler="ddim", steps=S, eta=eta)
    assert d.range_fallbacks == 0
    torch.manual_seed(61)
    x_T = torch.randn((B, 4, hw, hw))
    # one global randn per step when eta > 0 (the DDPM sampler's draw order)
    noise_of = (lambda p: torch.randn(x_T.shape)) if eta > 0 else (lambda p: torch.zeros_like(x_T))
    exp = rules.trajectory(x_T, "ddim", d.ddim_tables(S, eta, "cpu"),
                           lambda x, t, pos: cfg_eps(unet_sd, x, t, y, vals, mask), noise_of)
    err = rel(out, exp)
    print(f"[ddim trajectory {case}] B={B} {hw}x{hw} S={S} eta={eta} {source}: rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err


# ---- 7: graph == eager, determinism, the schedule is part of the graph key -----------------------
@pytest.mark.parametrize("B", [4, 64])
def test_ddim_graph_loop_equals_eager_and_is_deterministic(model, cuda, B):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn((B, 4, 32, 32), generator=g).to(cuda)
    y = torch.tensor([1 + i % 3 for i in range(B)], device=cuda)
    vals = torch.rand((B, 12), generator=g).to(cuda)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(cuda) if B > 4 else torch.ones((B, 12), device=cuda)
    sched = d.ddim_tables(25, 1.0, cuda)
    x = torch.empty_like(x0)  # ONE state buffer and ONE position scalar for every loop below
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(sched, start, steps, use_graph):
        x.copy_(x0)
        t.fill_(start)
        nm.sample_loop(x, t, y, 0, vals, mask, 3.0, None, steps, seed=1234, use_graph=use_graph, sched=sched)
        torch.cuda.synchronize()
        assert int(t.item()) == start - steps
        return x.cpu()

    outs = [loop(sched, 25, 19, ug) for ug in (True, False, True)]  # position 25 -> 6
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.isfinite(outs[0]).all()
    if B == 4:
        a, b = x0.clone(), torch.empty_like(x0)
        for p in range(25, 6, -1):
            nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), y, 0, vals, mask, 3.0, None,
                    seed=1234, t_stride=0, sched=sched)
            a, b = b, a
        assert torch.equal(a.cpu(), outs[0])
    # another schedule on the same buffers: only the schedule tells its graphs from the ones above
    sched10 = d.ddim_tables(10, 1.0, cuda)
    graph10 = loop(sched10, 10, 10, True)
    eager10 = loop(sched10, 10, 10, False)
    assert torch.equal(graph10, eager10) and not torch.equal(graph10, outs[0])
    # and the DDPM loop on the same buffers is not confused with either
    tables = d.coef_tables(cuda, True)

    def ddpm(use_graph):
        x.copy_(x0)
        t.fill_(10)
        nm.sample_loop(x, t, y, 0, vals, mask, 3.0, tables, 10, seed=1234, use_graph=use_graph)
        torch.cuda.synchronize()
        return x.cpu()

    assert torch.equal(ddpm(True), ddpm(False))
    assert torch.equal(loop(sched10, 10, 10, True), eager10)


# ---- 8: full stride with eta = 1 is the DDPM sampler -----------------------------------------------
def test_ddim_full_stride_eta1_is_ddpm(model, cuda):
    import diff
    d = diff.Diffuser(40, device=cuda)
    g = torch.Generator().manual_seed(80)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    mask = torch.ones((2, 12), device=cuda)
    kw = dict(z_shape=(4, 16, 16), vae=None, progress=False, guidance_scale=3.0, cond=vals, cond_mask=mask)
    torch.manual_seed(81)
    ddpm = d.sample_latent_cond(model, {1: 1, 2: 1}, **kw)
    s_ddpm = torch.get_rng_state()
    torch.manual_seed(81)
    ddim = d.sample_latent_cond(model, {1: 1, 2: 1}, sampler="ddim", steps=40, eta=1.0, **kw)
    s_ddim = torch.get_rng_state()
    err = rel(ddim, ddpm)
    print(f"[ddim full stride eta=1 vs ddpm] rel-L2 = {err:.3e}")
    assert err <= TRAJ_TOL, err
    assert torch.equal(s_ddpm, s_ddim)  # x_T, then one global draw per step, in both


# ---- 9: eta = 0 draws no step noise ----------------------------------------------------------------
def test_ddim_eta0_draws_only_x_T(model, cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(90)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    mask = torch.ones((2, 12), device=cuda)
    outs = []
    for _ in range(2):
        torch.manual_seed(91)
        outs.append(d.sample_latent_cond(model, {2: 1, 3: 1}, z_shape=(4, 16, 16), vae=None, progress=False,
                                         cond=vals, cond_mask=mask, sampler="ddim", steps=6).cpu())
        after = torch.get_rng_state()
        torch.manual_seed(91)
        torch.randn((2, 4, 16, 16))
        assert torch.equal(after, torch.get_rng_state())
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()


# ---- 10: public paths ------------------------------------------------------------------------------
def test_ddim_sample_to_pil(model, vae, cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    torch.manual_seed(100)
    imgs = d.sample_latent_cond(model, {1: 1, 2: 1, 3: 1}, z_shape=(4, 16, 16), vae=vae, to_pil=True,
                                progress=False, sampler="ddim", steps=5)
    assert len(imgs) == 3 and all(im.size == (128, 128) for im in imgs)


@pytest.mark.parametrize("source,eta", [("host", 0.5), ("host", 0.0), ("device", 1.0)])
def test_ddim_sharded_world1_equals_diffuser(model, cuda, source, eta):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    g = torch.Generator().manual_seed(101)
    vals = torch.rand((5, 12), generator=g).to(cuda)
    mask = (torch.rand((5, 12), generator=g) > 0.3).float().to(cuda)
    torch.manual_seed(102)
    lat = dd.ShardedCondSampler(d, model, None).sample({1: 3, 3: 2}, z_shape=(4, 16, 16), cond=vals, cond_mask=mask,
                                                       decode=False, sampler="ddim", steps=8, eta=eta)
    s_sharded = torch.get_rng_state()
    torch.manual_seed(102)
    single = d.sample_latent_cond(model, {1: 3, 3: 2}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals,
                                  cond_mask=mask, sampler="ddim", steps=8, eta=eta)
    assert torch.equal(lat.cpu(), single.cpu()) and torch.isfinite(single).all()
    assert torch.equal(s_sharded, torch.get_rng_state())


@pytest.fixture
def unet_sd_overflow():
    return overflow_sd()


@pytest.mark.parametrize("source", ["host", "device"])
def test_ddim_range_guard_replays_in_fp32(cuda, unet_sd_overflow, source):
    import diff
    m = make_model(cuda, unet_sd_overflow)
    d = diff.Diffuser(8, device=cuda)
    d.noise_source = source
    g = torch.Generator().manual_seed(35)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    mask = torch.ones((2, 12), device=cuda)
    torch.manual_seed(36)
    lat = d.sample_latent_cond(m, {1: 1, 2: 1}, z_shape=(4, 16, 16), vae=None, progress=False, cond=vals,
                               cond_mask=mask, sampler="ddim", steps=4, eta=0.5)
    assert d.range_fallbacks == 1
    assert torch.isfinite(lat).all() and m.native().precision == "x3"
