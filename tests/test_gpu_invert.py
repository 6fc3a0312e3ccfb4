"""GPU: DDIM inversion — the fused update, one network row, trajectories, the graph loop, the round trip
through sample_latent_cond(start_latent=...), the range guard and the poison check — against the torch
restatement of tests/test_invert_host.py, which takes eps from the oracle
(oracle.ref.unet_cond_geom_forward) and the tables from Diffuser.invert_tables.

A row c (countdown, N..1) of the tables computes y = i_x src + i_e eps(x, t_eval); x <- y; src <- y
where adv != 0.  Bounds as in test_gpu_ddim.py: 2e-5 for one step, 1e-4 for a trajectory.
Every trajectory case is first checked on the CPU to pass on less than 2x a 1e-5 relative perturbation
of z0, so that parity at those bounds is a statement about the kernels and not about the problem.

Measured on an MI355X (rel-L2): one row against the oracle 1.4e-7 .. 5.4e-7 (native and foreign paths);
trajectories (a) 1.6e-6, (b) 1.0e-6, (c) 2.6e-6, (d) 1.2e-6 with CPU perturbation gains 0.20 / 0.80 / 0.69 /
0.21; round trip R = 0 2.399e-1, R = 3 1.587e-3 (the CPU restatement: the same to four digits)."""
import pytest
import torch

from oracle.rules import Foreign, cfg_eps, invert_update, rel
from support import make_model, on, overflow_sd, run_worker
from test_invert_host import invert_ref, perturbation_gain, round_trip_inputs

pytestmark = pytest.mark.gpu

TOL = 2e-5        # one step (the project's step bound)
TRAJ_TOL = 1e-4   # a trajectory (the project's trajectory bound)


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    return make_model(cuda, unet_sd)


@pytest.fixture
def unet_sd_overflow():
    return overflow_sd()


# ---- 1: the update, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 3, 5])  # (5: the update takes any channel count)
def test_invert_update_bit_exact(cuda, C):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    tables = d.invert_tables(20, 0.3, 2, "cpu")  # 18 rows
    dtab = d.invert_tables(20, 0.3, 2, cuda)
    g = torch.Generator().manual_seed(9 + C)
    B = 6
    pos = torch.tensor([18, 16, 12, 10, 2, 1])  # (p, k) = (1,0) (1,2) (3,0) (3,2) (6,1) (6,2): adv 0 1 0 1 0 1
    assert tables[3][pos - 1].tolist() == [0, 1, 0, 1, 0, 1]
    x, eu, ec, src = (torch.randn((B, C, 16, 16), generator=g) for _ in range(4))
    for guided in (True, False):
        eps = eu + 3.0 * (ec - eu) if guided else eu
        exp, exp_src = invert_update(src, eps, pos, tables)
        s = src.to(cuda)
        out = engine.invert_update(x.to(cuda), eu.to(cuda), ec.to(cuda) if guided else None, 3.0 if guided else 0.0,
                                   pos.to(cuda), dtab, s)
        assert torch.equal(out.cpu(), exp) and torch.equal(s.cpu(), exp_src)
        assert not torch.equal(exp_src, src) and torch.equal(exp_src[0], src[0])  # (the rows do mix)
    # out may alias x: x's values are not an operand
    xa, s = x.to(cuda), src.to(cuda)
    res = engine.invert_update(xa, eu.to(cuda), ec.to(cuda), 3.0, pos.to(cuda), dtab, s, out=xa)
    exp, exp_src = invert_update(src, eu + 3.0 * (ec - eu), pos, tables)
    assert res.data_ptr() == xa.data_ptr()
    assert torch.equal(xa.cpu(), exp) and torch.equal(s.cpu(), exp_src)


def test_invert_update_and_step_reject_bad_operands(model, cuda):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    tab = d.invert_tables(7, None, 1, cuda)
    x = torch.zeros((2, 4, 8, 8), device=cuda)
    pos = torch.tensor([7, 7], device=cuda)
    for bad in (None, torch.zeros((2, 4, 8, 4), device=cuda), torch.zeros((2, 4, 8, 8), device=cuda).double()):
        with pytest.raises(ValueError):
            engine.invert_update(x, x, None, 0.0, pos, tab, bad)
    src = torch.zeros_like(x)
    with pytest.raises(ValueError):  # y may not land in src
        engine.invert_update(x, x, None, 0.0, pos, tab, src, out=src)
    with pytest.raises(ValueError):  # a DDIM schedule is no inversion table
        engine.invert_update(x, x, None, 0.0, pos, d.ddim_tables(7, 0.0, cuda), src)
    with pytest.raises(ValueError):
        engine.invert_update(x, x, None, 0.0, pos, d.invert_tables(7, None, 1, "cpu"), src)
    nm = model.native()
    y = torch.tensor([1, 2], device=cuda)
    x16 = torch.zeros((2, 4, 16, 16), device=cuda)
    s16 = torch.zeros_like(x16)
    for kw in (dict(sched=d.ddim_tables(7, 0.0, cuda)), dict(rescale=0.5), dict(noise=torch.zeros_like(x16)),
               dict(hist=torch.zeros_like(x16)), dict(geom=(torch.ones(2, device=cuda), tab[1]))):
        with pytest.raises(ValueError):
            nm.step(x16, torch.empty_like(x16), pos, y, 0, None, None, 3.0, None, invert=(tab, s16), **kw)
    with pytest.raises(ValueError):
        nm.step(x16, torch.empty_like(x16), pos, y, 0, None, None, 3.0, None, invert=(tab, x16))


# ---- 2: one network row against the oracle ---------------------------------------------------------
_STEP_REF = {}


def step_inputs():
    g = torch.Generator().manual_seed(31)
    B = 3
    x = 0.8 * torch.randn((B, 4, 32, 32), generator=g)
    src = 0.8 * torch.randn((B, 4, 32, 32), generator=g)
    y = torch.tensor([1, 3, 2])
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.4).float()
    # S = 20, strength 0.3, R = 2 (18 rows): (p, k) = (1, 0) at tau_1, (3, 0) at tau_2, (3, 2) at tau_3 with adv
    pos = torch.tensor([18, 12, 10])
    return x, src, y, vals, mask, pos


def step_ref(unet_sd, d, guidance, with_y=True):
    """The restatement of the three rows, fed oracle eps; once per kind of step."""
    key = (guidance, with_y)
    if key not in _STEP_REF:
        x, src, y, vals, mask, pos = step_inputs()
        tables = d.invert_tables(20, 0.3, 2, "cpu")
        assert tables[0][pos - 1].tolist() == [50, 100, 150] and tables[3][pos - 1].tolist() == [0, 0, 1]
        with torch.no_grad():
            if with_y:
                eps = cfg_eps(unet_sd, x, tables[0][pos - 1], y, vals, mask, guidance)
            else:  # y omitted: the null label, no condition
                eps = cfg_eps(unet_sd, x, tables[0][pos - 1], torch.zeros_like(y), None, None, 0.0)
        _STEP_REF[key] = invert_update(src, eps, pos, tables)
    return _STEP_REF[key]


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_invert_step_vs_oracle(model, cuda, unet_sd, prec):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    x, src, y, vals, mask, pos = step_inputs()
    exp, exp_src = step_ref(unet_sd, d, 3.0)
    plan = d._plan(x.to(cuda), ("invert", 20, 0.3, 2), 3.0)
    s = src.to(cuda)
    state = torch.get_rng_state()
    with model.native().precision_override(prec):
        out = d._step(model, x.to(cuda), pos.to(cuda), plan, True, *on(cuda, y), 0, *on(cuda, vals, mask), hist=s)
    e_x, e_s = rel(out, exp), rel(s, exp_src)
    print(f"[invert step {prec} 32x32 cfg 3.0] rel-L2 vs oracle: y {e_x:.3e}, src {e_s:.3e}")
    assert e_x <= TOL and e_s <= TOL, (e_x, e_s)
    assert torch.equal(s[:2].cpu(), src[:2]) and torch.equal(s[2].cpu(), out[2].cpu())  # adv rows only
    assert torch.equal(torch.get_rng_state(), state)  # nothing is drawn


def test_invert_step_without_cfg_and_foreign_model(model, cuda, unet_sd):
    """guidance 0: one conditional forward, y given or omitted (the null label); a duck-typed model takes
    the model-call + dmx_invert_update path and lands on the same numbers."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    x, src, y, vals, mask, pos = step_inputs()

    outs = {}
    for name, mdl in (("native", model), ("foreign", Foreign(model))):
        for case, g, with_y in (("cfg", 3.0, True), ("y", 0.0, True), ("no-y", 0.0, False)):
            exp, exp_src = step_ref(unet_sd, d, g, with_y)
            plan = d._plan(x.to(cuda), ("invert", 20, 0.3, 2), g)
            s = src.to(cuda)
            cond = on(cuda, vals, mask) if with_y else (None, None)
            out = d._step(mdl, x.to(cuda), pos.to(cuda), plan, True, y.to(cuda) if with_y else None, 0, *cond, hist=s)
            e_x, e_s = rel(out, exp), rel(s, exp_src)
            print(f"[invert step {name} {case}] rel-L2 vs oracle: y {e_x:.3e}, src {e_s:.3e}")
            assert e_x <= TOL and e_s <= TOL, (name, case, e_x, e_s)
            outs[name, case] = (out, s)
    for case in ("cfg", "y", "no-y"):
        assert rel(outs["foreign", case][0], outs["native", case][0]) <= TOL
        assert rel(outs["foreign", case][1], outs["native", case][1]) <= TOL


# ---- 3: trajectories against the restatement --------------------------------------------------------
@pytest.mark.parametrize("case,counts,hw,S,strength,R,g", [
    ("a", {1: 1, 2: 1}, 16, 11, None, 0, 3.0),            # 11 rows: one 8-step graph launch + three one-step launches
    ("b", {1: 1, 3: 1}, 16, 20, 0.3, 2, 3.0),             # 18 rows
    ("c", {1: 11, 2: 11, 3: 10}, 32, 4, 0.5, 1, 3.0),     # 4 rows; the 64-row batch class: Winograd convs
    ("d", {2: 1, 3: 1}, 16, 7, None, 0, 0.0),             # the host-stepped path: one forward per row
])
def test_invert_trajectory_vs_restatement(model, cuda, unet_sd, case, counts, hw, S, strength, R, g):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    B = sum(counts.values())
    y = torch.tensor([c for c, n in counts.items() for _ in range(n)])
    gen = torch.Generator().manual_seed(60 + S)
    z0 = 0.8 * torch.randn((B, 4, hw, hw), generator=gen)
    vals = torch.rand((B, 12), generator=gen)
    mask = (torch.rand((B, 12), generator=gen) > 0.3).float()
    tables = d.invert_tables(S, strength, R, "cpu")
    # is the case well conditioned?  (case c at four of its rows: the check costs two more trajectories)
    rows = torch.arange(B) if B <= 4 else torch.tensor([0, 11, 22, B - 1])
    gain = perturbation_gain(z0[rows], tables,
                             lambda x, t: cfg_eps(unet_sd, x, t, y[rows], vals[rows], mask[rows], g))
    print(f"[invert trajectory {case}] gain of a 1e-5 perturbation of z0 on the CPU: {gain:.2f}")
    assert gain < 2.0, gain
    state = torch.get_rng_state()
    out = d.invert_latent_cond(model, z0, counts, steps=S, strength=strength, refine=R, guidance_scale=g,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda))
    assert d.range_fallbacks == 0
    assert torch.equal(torch.get_rng_state(), state)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(z0.shape)
    exp = invert_ref(z0, tables, lambda x, t: cfg_eps(unet_sd, x, t, y, vals, mask, g))
    err = rel(out, exp)
    print(f"[invert trajectory {case}] B={B} {hw}x{hw} S={S} strength={strength} R={R} g={g}: "
          f"rel-L2 vs restatement = {err:.3e}")
    assert err <= TRAJ_TOL, err


# ---- 4: graph == eager, determinism, the tables and src are part of the graph key -------------------
@pytest.mark.parametrize("B", [4, 64])
def test_invert_graph_loop_equals_eager_and_is_deterministic(model, cuda, B):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    g = torch.Generator().manual_seed(2)
    x0 = (0.8 * torch.randn((B, 4, 32, 32), generator=g)).to(cuda)
    y = torch.tensor([1 + i % 3 for i in range(B)], device=cuda)
    vals = torch.rand((B, 12), generator=g).to(cuda)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(cuda) if B > 4 else torch.ones((B, 12), device=cuda)
    tab1 = d.invert_tables(20, 0.5, 1, cuda)  # 20 rows
    tab2 = d.invert_tables(20, 0.5, 2, cuda)  # 30 rows
    x = torch.empty_like(x0)  # ONE state buffer, ONE source buffer and ONE position scalar for every loop below
    src = torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def inv_loop(tab, start, steps, use_graph):
        x.copy_(x0)
        src.copy_(x0)
        t.fill_(start)
        nm.sample_loop(x, t, y, 0, vals, mask, 3.0, None, steps, use_graph=use_graph, invert=(tab, src))
        torch.cuda.synchronize()
        assert int(t.item()) == start - steps
        return x.cpu(), src.cpu()

    def ddim_loop(sched, use_graph):
        x.copy_(x0)
        t.fill_(10)
        nm.sample_loop(x, t, y, 0, vals, mask, 3.0, None, 10, seed=1234, use_graph=use_graph, sched=sched)
        torch.cuda.synchronize()
        assert int(t.item()) == 0
        return x.cpu()

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    outs = [inv_loop(tab1, 20, 19, ug) for ug in (True, False, True)]  # rows 20 .. 2: 8 + 8 + 3 launches
    assert same(outs[0], outs[1]) and same(outs[0], outs[2])
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert not torch.equal(outs[0][0], outs[0][1])  # (row 2 is a k = 0 row: x has moved on, src has not)
    if B == 4:
        a, b, s = x0.clone(), torch.empty_like(x0), x0.clone()
        for c in range(20, 1, -1):
            nm.step(a, b, torch.full((1,), c, dtype=torch.long, device=cuda), y, 0, vals, mask, 3.0, None,
                    t_stride=0, invert=(tab1, s))
            a, b = b, a
        assert torch.equal(a.cpu(), outs[0][0]) and torch.equal(s.cpu(), outs[0][1])
    # another table (another R) on the same buffers: only the tables tell its graphs from the ones above
    graph2 = inv_loop(tab2, 30, 19, True)
    eager2 = inv_loop(tab2, 30, 19, False)
    assert same(graph2, eager2) and not torch.equal(graph2[0], outs[0][0])
    # a DDIM loop, the inversion loop, the DDIM loop again, all on the same x and scalar
    ddim10 = d.ddim_tables(10, 0.0, cuda)
    eager_ddim = ddim_loop(ddim10, False)
    assert torch.equal(ddim_loop(ddim10, True), eager_ddim)
    assert same(inv_loop(tab1, 20, 19, True), outs[1])
    assert torch.equal(ddim_loop(ddim10, True), eager_ddim)
    # another source buffer with the same tables: its own graphs; the first buffer is not touched
    before = src.clone()
    src2 = torch.empty_like(x0)
    x.copy_(x0)
    src2.copy_(x0)
    t.fill_(20)
    nm.sample_loop(x, t, y, 0, vals, mask, 3.0, None, 19, use_graph=True, invert=(tab1, src2))
    torch.cuda.synchronize()
    assert same((x.cpu(), src2.cpu()), outs[1]) and torch.equal(src.cpu(), before.cpu())


# ---- 5: the round trip — the property the feature exists for ----------------------------------------
def test_invert_round_trip(model, cuda):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    z0, y, vals, mask = round_trip_inputs()
    kw = dict(cond=vals.to(cuda), cond_mask=mask.to(cuda), guidance_scale=3.0)
    state = torch.get_rng_state()
    errs, lat = {}, {}
    for R in (0, 3):
        lat[R] = d.invert_latent_cond(model, z0, [(1, 1), (3, 1)], steps=20, strength=0.3, refine=R, **kw)
        back = d.sample_latent_cond(model, [(1, 1), (3, 1)], start_latent=lat[R], strength=0.3, sampler="ddim",
                                    steps=20, vae=None, progress=False, **kw)
        errs[R] = rel(back, z0)
        print(f"[invert round trip, GPU] R={R}: rel-L2 vs z0 = {errs[R]:.3e}")
    assert torch.equal(torch.get_rng_state(), state)  # neither call draws
    assert d.range_fallbacks == 0
    assert errs[3] <= 1e-2, errs
    assert errs[0] >= 5e-2, errs
    assert errs[3] < errs[0] / 10, errs
    # an edited condition (another target label) gives another sample from the same latent
    same = d.sample_latent_cond(model, [(1, 1), (3, 1)], start_latent=lat[3], strength=0.3, sampler="ddim",
                                steps=20, vae=None, progress=False, **kw)
    edit = d.sample_latent_cond(model, [(2, 1), (3, 1)], start_latent=lat[3], strength=0.3, sampler="ddim",
                                steps=20, vae=None, progress=False, **kw)
    assert torch.isfinite(edit).all() and not torch.equal(edit[0], same[0])
    assert torch.equal(edit[1], same[1])  # (the sample whose label stayed is the same sample)
    # the second-order solver starts from the latent as it is, too
    dpm = d.sample_latent_cond(model, [(1, 1), (3, 1)], start_latent=lat[3], strength=0.3, sampler="dpmpp_2m",
                               spacing="uniform", steps=20, vae=None, progress=False, **kw)
    assert torch.isfinite(dpm).all() and tuple(dpm.shape) == tuple(z0.shape)


# ---- 6: the range guard replays a chunk from its x and its src --------------------------------------
def test_invert_range_guard_replays_in_fp32(cuda, unet_sd_overflow):
    import diff
    m = make_model(cuda, unet_sd_overflow)
    g = torch.Generator().manual_seed(35)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    mask = torch.ones((2, 12), device=cuda)
    z0 = 0.8 * torch.randn((2, 4, 16, 16), generator=g)

    def run():
        d = diff.Diffuser(8, device=cuda)
        return d, d.invert_latent_cond(m, z0, {1: 1, 2: 1}, steps=4, refine=1, cond=vals, cond_mask=mask)

    d, lat = run()
    assert d.range_fallbacks == 1
    assert torch.isfinite(lat).all() and m.native().precision == "x3"
    with m.native().precision_override("fp32"):
        d32, lat32 = run()
    assert d32.range_fallbacks == 0
    assert torch.equal(lat.cpu(), lat32.cpu())


# ---- 7: no read of unwritten workspace; shards equal the batch --------------------------------------
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
m.to(dev).eval()
d = diff.Diffuser(1000, device=dev)
nm = m.native()
g = torch.Generator().manual_seed(40)
B = 5
z0 = (0.8 * torch.randn((B, 4, 16, 16), generator=g)).to(dev)
vals = torch.rand((B, 12), generator=g).to(dev)
mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(dev)
y = torch.tensor([1] * 3 + [3] * (B - 3), device=dev)
tab = d.invert_tables(20, 0.3, 1, dev)  # 12 rows: one 8-step graph launch + three one-step launches
out = {}
for s, e in ((0, B), (0, 3), (3, B)):
    x, src = z0[s:e].clone(), z0[s:e].clone()
    t = torch.full((1,), 12, dtype=torch.long, device=dev)
    nm.sample_loop(x, t, y[s:e].contiguous(), 0, vals[s:e].contiguous(), mask[s:e].contiguous(), 3.0, None, 11,
                   sample_offset=s, invert=(tab, src))
    torch.cuda.synchronize()
    out[f"x_{s}_{e}"], out[f"src_{s}_{e}"] = x.cpu(), src.cpu()
torch.save(out, sys.argv[1])
print("[invert-poison-worker] ok", flush=True)
'''


def test_invert_loop_reads_no_unwritten_workspace(cuda, tmp_path):
    clean = run_worker(tmp_path, "clean", WORKER)
    poisoned = run_worker(tmp_path, "poison", WORKER, DMX_POISON="1")
    bad = [k for k in clean if not torch.isfinite(poisoned[k]).all() or not torch.equal(clean[k], poisoned[k])]
    assert bad == [], bad
    for what in ("x", "src"):
        parts = torch.cat([clean[f"{what}_0_3"], clean[f"{what}_3_5"]])
        assert torch.equal(clean[f"{what}_0_5"], parts), what
