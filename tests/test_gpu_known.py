"""GPU: known-region sampling (img2img start, masked inpainting) — the blend kernel, the three samplers on
the graph loop, the per-step native path and the foreign-model path, the graph key, the range guard's
replay and the public samplers — against torch-CPU restatements that take eps from the oracle
(oracle.ref.unet_cond_geom_forward) and the tables from the Diffuser.

After the step at position p has produced xg (fp32, torch's evaluation order, one rounding per op):
  kn = q_a[p-1] z0 + q_e[p-1] e0;   x' = kn where m == 0, xg where m == 1, else m xg + (1 - m) kn
and a loop entering at p0 < S starts from q_a[p0] z0 + q_e[p0] e0 (row p0: the timestep tau_p0).
Bounds are the project's: TOL for one step, TRAJ_TOL for a trajectory; the blend itself and everything
the mask keeps are held bit for bit.

Measured on an MI355X (rel-L2 against the oracle): trajectories (a) 1.1e-6, (b) 1.8e-6, (c) 1.8e-6."""
import numpy as np
import pytest
import torch

from oracle import rules
from oracle.rules import cfg_eps, known_blend, rel
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


def box_mask(B, hw, generator=None, fractional=False):
    """(B,1,hw,hw): 1 inside a box that differs per sample, 0 outside; fractional: a soft rim between."""
    m = torch.zeros((B, 1, hw, hw))
    for i in range(B):
        a = 2 + i % 3
        m[i, :, a:hw - 3, a + 1:hw - 2] = 1.0
        if fractional:
            m[i, :, a - 1, :] = 0.25
            m[i, :, :, hw - 2] = 0.6
    return m


def known_trajectory(d, mode, e0, z0, m, p0, eps_of):
    """rules.trajectory over positions p0..1 of the deterministic samplers (mode = ("ddim", S, 0.0) or
    ("dpm", S, spacing)) from the start latent, the blend after every step where m is given.
    eps_of(x, t, pos) -> eps.  Row p0 of the truncated DPM schedule is first-order (the NaN history would show)."""
    tau = d._mode_timesteps(mode)
    S = len(tau)
    tabs = d.known_tables(tau, "cpu")
    sched = d.dpm_tables(S, mode[2], "cpu", start=p0) if mode[0] == "dpm" else d.ddim_tables(S, 0.0, "cpu")
    x = e0 if p0 == S else known_blend(None, z0, e0, None, torch.full((e0.shape[0],), p0 + 1), tabs)
    blend = None if m is None else (lambda x, pos: known_blend(x, z0, e0, m, pos, tabs))
    return rules.trajectory(x, mode[0], sched, eps_of, p0=p0, blend=blend)


# ---- 1: the blend, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 7, 5), (2, 4, 16, 16), (2, 3, 16, 16), (2, 4, 34, 32)])
def test_known_blend_bit_exact(cuda, shape):
    """(3,4,7,5): the scalar path, 35 elements per row; (2,4,16,16) / (2,3,16,16): the float4 path;
    (2,4,34,32): 1088 elements per row — more than one block on either path."""
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    S = 9
    tau = d.dpm_timesteps(S, "logsnr")
    tabs, dtabs = d.known_tables(tau, "cpu"), d.known_tables(tau, cuda)
    B, C, h, w = shape
    g = torch.Generator().manual_seed(70 + h)
    xg, z0, e0 = (torch.randn(shape, generator=g) for _ in range(3))
    # masks: exact zeros, exact ones and fractions in one tensor; then all-zero and all-one
    u = torch.rand((B, 1, h, w), generator=g)
    mixed = torch.where(u < 0.3, torch.zeros_like(u), torch.where(u > 0.7, torch.ones_like(u), u))
    assert (mixed == 0).any() and (mixed == 1).any() and ((mixed > 0) & (mixed < 1)).any()
    per_sample = torch.tensor([1, S, 4][:B])
    dz, de, dx = z0.to(cuda), e0.to(cuda), xg.to(cuda)
    for m in (mixed, torch.zeros_like(mixed), torch.ones_like(mixed)):
        dm = m.to(cuda)
        for pos in (per_sample, torch.tensor([1]), torch.tensor([S]), torch.tensor([5])):
            pfull = pos if pos.numel() == B else pos.expand(B)
            exp = known_blend(xg, z0, e0, m, pfull, tabs)
            out = engine.known_blend(dx, pos.to(cuda), (dz, de, dm, *dtabs))
            assert torch.equal(out.cpu(), exp), (shape, pos)
        # the mask may also be given as (B,h,w)
        out3 = engine.known_blend(dx, per_sample.to(cuda), (dz, de, dm.reshape(B, h, w), *dtabs))
        assert torch.equal(out3.cpu(), known_blend(xg, z0, e0, m, per_sample, tabs))
    # p = 1 keeps z0 itself (row 0 is (1, 0)); m == 1 passes xg through
    one = torch.tensor([1])
    assert torch.equal(engine.known_blend(dx, one.to(cuda), (dz, de, torch.zeros_like(mixed).to(cuda), *dtabs)).cpu(), z0)
    # positions outside [1, S] are clamped
    for bad, to in ((0, 1), (-3, 1), (S + 5, S)):
        out = engine.known_blend(dx, torch.tensor([bad]).to(cuda), (dz, de, mixed.to(cuda), *dtabs))
        assert torch.equal(out.cpu(), known_blend(xg, z0, e0, mixed, torch.full((B,), to), tabs))
    # mask None: the start-latent form writes kn and does not read x (NaN there changes nothing)
    for pos in (per_sample, torch.tensor([S]), torch.tensor([3])):
        pfull = pos if pos.numel() == B else pos.expand(B)
        exp = known_blend(None, z0, e0, None, pfull, tabs)
        nan = torch.full(shape, float("nan"), device=cuda)
        out = engine.known_blend(nan, pos.to(cuda), (dz, de, None, *dtabs))
        assert torch.equal(out.cpu(), exp)
        assert torch.equal(engine.known_blend(dz, pos.to(cuda), (dz, de, None, *dtabs)).cpu(), exp)  # x may be z0
    # a non-finite xg under the mask does not reach a kept element
    keep = (mixed == 0).expand(shape)
    bad_x = torch.where(keep, torch.full_like(xg, float("nan")), torch.full_like(xg, float("inf")))
    out = engine.known_blend(bad_x.to(cuda), per_sample.to(cuda), (dz, de, mixed.to(cuda), *dtabs)).cpu()
    assert torch.equal(out[keep], known_blend(xg, z0, e0, mixed, per_sample, tabs)[keep])
    # out may alias x
    xa = xg.to(cuda)
    res = engine.known_blend(xa, per_sample.to(cuda), (dz, de, mixed.to(cuda), *dtabs), out=xa)
    assert res.data_ptr() == xa.data_ptr()
    assert torch.equal(xa.cpu(), known_blend(xg, z0, e0, mixed, per_sample, tabs))


def test_known_blend_rejects_aliases_and_mismatched_tables(model, cuda):
    import diff
    from dmx import engine
    from dmx._lib import DmxError
    d = diff.Diffuser(1000, device=cuda)
    tabs = d.known_tables(d.ddim_timesteps(6), cuda)
    x, z0, e0 = (torch.zeros((2, 4, 16, 16), device=cuda) for _ in range(3))
    m = torch.ones((2, 1, 16, 16), device=cuda)
    pos = torch.tensor([3, 3], device=cuda)
    for out in (z0, e0):  # z0 / e0 must stay constants: never the output
        with pytest.raises(DmxError):
            engine.known_blend(x, pos, (z0, e0, m, *tabs), out=out)
    for bad in ((z0, e0, m, tabs[0]), (z0[:1], e0, m, *tabs), (z0, e0.double(), m, *tabs),
                (z0, e0, m[:, :, :8], *tabs), (z0, e0, torch.ones((2, 4, 16, 16), device=cuda), *tabs),
                (z0, e0, m, tabs[0], tabs[1][:3]), (z0.cpu(), e0, m, *tabs)):
        with pytest.raises(ValueError):
            engine.known_blend(x, pos, bad)
    with pytest.raises(ValueError):
        engine.known_blend(x, torch.tensor([1, 2, 3], device=cuda), (z0, e0, m, *tabs))
    # in a step the blend's tables must cover the step's schedule: S = 6 against a 7-position schedule
    nm = model.native()
    y = torch.tensor([1, 2], device=cuda)
    out = torch.empty_like(x)
    step = dict(sched=d.ddim_tables(7, 0.0, cuda), known=(z0, e0, m, *tabs))
    with pytest.raises(DmxError, match="S differs"):
        nm.step(x, out, pos, y, 0, None, None, 3.0, None, **step)
    with pytest.raises(DmxError, match="S differs"):  # the DDPM step: S must be T
        nm.step(x, out, pos, y, 0, None, None, 3.0, d.coef_tables(cuda, True), known=(z0, e0, m, *tabs))
    with pytest.raises(DmxError, match="alias"):  # x_out must not be z0
        nm.step(x, z0, pos, y, 0, None, None, 3.0, None, sched=d.ddim_tables(6, 0.0, cuda), known=(z0, e0, m, *tabs))
    with pytest.raises(ValueError):  # a step needs the mask
        nm.step(x, out, pos, y, 0, None, None, 3.0, None, sched=d.ddim_tables(6, 0.0, cuda),
                known=(z0, e0, None, *tabs))
    t = torch.full((1,), 6, dtype=torch.long, device=cuda)
    with pytest.raises(DmxError, match="alias"):  # the loop runs in place on x: x must not be e0
        nm.sample_loop(e0, t, y, 0, None, None, 3.0, None, 2, sched=d.ddim_tables(6, 0.0, cuda),
                       known=(z0, e0, m, *tabs))


# ---- 2: default paths are untouched; an all-zero mask returns z0 ----------------------------------
SAMPLERS = {"ddpm": dict(), "ddim": dict(sampler="ddim", steps=6, eta=1.0), "dpmpp_2m": dict(sampler="dpmpp_2m", steps=6)}


@pytest.mark.parametrize("source", ["device", "host"])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_defaults_untouched_and_zero_mask_returns_z0(model, cuda, name, source):
    import diff
    d = diff.Diffuser(12 if name == "ddpm" else 1000, device=cuda)
    d.noise_source = source
    g = torch.Generator().manual_seed(80)
    B, hw = 2, 16
    vals = torch.rand((B, 12), generator=g).to(cuda)
    cmask = torch.ones((B, 12), device=cuda)
    z0 = torch.randn((B, 4, hw, hw), generator=g)
    kw = dict(z_shape=(4, hw, hw), vae=None, progress=False, cond=vals, cond_mask=cmask, **SAMPLERS[name])

    def run(**extra):
        torch.manual_seed(81)
        out = d.sample_latent_cond(model, {1: 1, 3: 1}, **kw, **extra).cpu()
        return out, torch.get_rng_state()

    plain, rng_plain = run()
    ones, rng_ones = run(init_latent=z0, mask=torch.ones((B, 1, hw, hw)))
    assert torch.equal(ones, plain) and torch.isfinite(plain).all()
    assert torch.equal(rng_ones, rng_plain)  # the blend draws nothing, in any mode
    start_only, _ = run(init_latent=z0.to(cuda))  # no mask, no strength: nothing to do
    assert torch.equal(start_only, plain)
    full, _ = run(init_latent=z0, strength=1.0)  # p0 = S: x_start = e0
    assert torch.equal(full, plain)
    zeros, rng_zeros = run(init_latent=z0, mask=torch.zeros((hw, hw)))
    assert torch.equal(zeros, z0)
    assert torch.equal(rng_zeros, rng_plain)
    assert d.range_fallbacks == 0


# ---- 3: the kept region is exact ------------------------------------------------------------------
@pytest.mark.parametrize("source", ["device", "host"])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_kept_region_is_exact(model, cuda, name, source):
    import diff
    d = diff.Diffuser(12 if name == "ddpm" else 1000, device=cuda)
    d.noise_source = source
    g = torch.Generator().manual_seed(82)
    B, hw = 2, 16
    vals = torch.rand((B, 12), generator=g).to(cuda)
    z0 = torch.randn((B, 4, hw, hw), generator=g)
    m = box_mask(B, hw)
    torch.manual_seed(83)
    out = d.sample_latent_cond(model, {2: 1, 3: 1}, vae=None, progress=False, cond=vals,
                               cond_mask=torch.ones((B, 12), device=cuda), init_latent=z0, mask=m.to(cuda),
                               strength=0.7, **SAMPLERS[name]).cpu()
    keep, regen = (m == 0).expand_as(z0), (m == 1).expand_as(z0)
    assert keep.any() and regen.any()
    assert torch.equal(out[keep], z0[keep])
    assert torch.isfinite(out).all() and not (out[regen] == z0[regen]).any()
    assert d.range_fallbacks == 0


# ---- 4: trajectories against the oracle -----------------------------------------------------------
@pytest.mark.parametrize("case,counts,hw,mode,strength,p0,source", [
    # seven steps on the device loop: the 8-step graph must not be taken for them
    ("a", {1: 1, 2: 1}, 16, ("dpm", 11, "logsnr"), 0.64, 7, "device"),
    ("b", {1: 1, 3: 1}, 16, ("ddim", 8, 0.0), None, 8, "host"),
    ("c", {1: 11, 2: 11, 3: 10}, 32, ("dpm", 4, "logsnr"), 0.75, 3, "device"),  # the 64-sample batch class
])
def test_known_trajectory_vs_oracle(model, cuda, unet_sd, case, counts, hw, mode, strength, p0, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    S = mode[1]
    assert d._known_start(strength, S) == p0
    B = sum(counts.values())
    y = torch.tensor([c for c, n in counts.items() for _ in range(n)])
    g = torch.Generator().manual_seed(160 + S)
    vals = torch.rand((B, 12), generator=g)
    cmask = (torch.rand((B, 12), generator=g) > 0.3).float()
    z0 = torch.randn((B, 4, hw, hw), generator=g)
    m = box_mask(B, hw, fractional=True)
    skw = dict(sampler="dpmpp_2m", steps=S, spacing=mode[2]) if mode[0] == "dpm" else dict(sampler="ddim", steps=S)
    torch.manual_seed(161)
    out = d.sample_latent_cond(model, counts, z_shape=(4, hw, hw), vae=None, progress=False, guidance_scale=3.0,
                               cond=vals.to(cuda), cond_mask=cmask.to(cuda), init_latent=z0.to(cuda), mask=m,
                               strength=strength, **skw)
    assert d.range_fallbacks == 0
    torch.manual_seed(161)
    e0 = torch.randn((B, 4, hw, hw))
    exp = known_trajectory(d, mode, e0, z0, m, p0, lambda x, t, pos: cfg_eps(unet_sd, x, t, y, vals, cmask))
    err = rel(out, exp)
    print(f"[known trajectory {case}] B={B} {hw}x{hw} {mode} p0={p0} {source}: rel-L2 vs oracle = {err:.3e}")
    assert err <= TRAJ_TOL, err
    keep = (m == 0).expand_as(z0)
    assert torch.equal(out.cpu()[keep], z0[keep])


# ---- 5: graph == eager, determinism, the known region is part of the graph key --------------------
@pytest.mark.parametrize("B", [4, 64])
def test_known_graph_loop_equals_eager_and_keys_apart(model, cuda, unet_sd, B):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(3)
    hw, S, p0 = 32, 11, 10  # ten steps: one launch of the 8-step graph and two of the one-step graph
    x0 = torch.randn((B, 4, hw, hw), generator=g).to(cuda)
    z0, e0 = (torch.randn((B, 4, hw, hw), generator=g).to(cuda) for _ in range(2))
    y = torch.tensor([1 + i % 3 for i in range(B)], device=cuda)
    vals = torch.rand((B, 12), generator=g).to(cuda)
    cmask = (torch.rand((B, 12), generator=g) > 0.3).float().to(cuda) if B > 4 else torch.ones((B, 12), device=cuda)
    sched = d.dpm_tables(S, "logsnr", cuda, start=p0)
    tabs = d.known_tables(d.dpm_timesteps(S, "logsnr"), cuda)
    mask1 = box_mask(B, hw, fractional=True).to(cuda)
    mask2 = (1 - box_mask(B, hw)).to(cuda).contiguous()  # a second mask buffer: keep the inside instead
    x = torch.empty_like(x0)  # ONE state buffer, ONE history and ONE position scalar for every loop below
    hist = torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(nm, mask, use_graph=True):
        x.copy_(x0)
        hist.fill_(float("nan"))  # row p0 of the truncated schedule does not read it
        t.fill_(p0)
        kw = dict(known=(z0, e0, mask, *tabs)) if mask is not None else {}
        nm.sample_loop(x, t, y, 0, vals, cmask, 3.0, None, p0, use_graph=use_graph, sched=sched, hist=hist, **kw)
        torch.cuda.synchronize()
        assert int(t.item()) == 0
        return x.cpu()

    nm = model.native()
    calls = (mask1, None, mask2)
    got = [loop(nm, mk) for mk in calls]  # known, plain, known with another mask: three graph pairs in turn
    for mk, res in zip(calls, got):  # each as the same call gives it on a model that has no graph yet
        fresh = make_model(cuda, unet_sd)
        assert torch.equal(loop(fresh.native(), mk), res)
        del fresh
    assert torch.equal(loop(nm, mask1), got[0]) and torch.isfinite(got[0]).all()
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2])
    assert torch.equal(loop(nm, mask1, use_graph=False), got[0])
    keep = (mask1 == 0).expand_as(z0).cpu()
    assert torch.equal(got[0][keep], z0.cpu()[keep])
    if B == 4:  # the per-step calls with the blend inside the step
        a, b, h = x0.clone(), torch.empty_like(x0), torch.full_like(x0, float("nan"))
        for p in range(p0, 0, -1):
            nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), y, 0, vals, cmask, 3.0, None,
                    t_stride=0, sched=sched, hist=h, known=(z0, e0, mask1, *tabs))
            a, b = b, a
        assert torch.equal(a.cpu(), got[0])


# ---- 6: the range guard's replay -------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
def test_known_range_guard_replay(cuda, unet_sd_overflow, source):
    import diff
    m = make_model(cuda, unet_sd_overflow)
    g = torch.Generator().manual_seed(135)
    vals = torch.rand((2, 12), generator=g).to(cuda)
    cmask = torch.ones((2, 12), device=cuda)
    z0 = torch.randn((2, 4, 16, 16), generator=g)
    mask = box_mask(2, 16, fractional=True)

    def run():
        d = diff.Diffuser(1000, device=cuda)
        d.noise_source = source
        d.GUARD_CHUNK = 3  # p0 = 7 of S = 9: chunks 7..5, 4..2, 1
        torch.manual_seed(136)
        lat = d.sample_latent_cond(m, {1: 1, 2: 1}, vae=None, progress=False, cond=vals, cond_mask=cmask,
                                   sampler="dpmpp_2m", steps=9, init_latent=z0, mask=mask, strength=0.8)
        return d, lat.cpu()

    d, lat = run()
    assert d._known_start(0.8, 9) == 7
    assert d.range_fallbacks == 3  # the overflow sits in the first block: every chunk is replayed
    assert torch.isfinite(lat).all() and m.native().precision == "x3"
    with m.native().precision_override("fp32"):
        d32, lat32 = run()
    assert d32.range_fallbacks == 0
    assert torch.equal(lat, lat32)
    keep = (mask == 0).expand_as(z0)
    assert torch.equal(lat[keep], z0[keep])


# ---- 7, 8: public paths ----------------------------------------------------------------------------
@pytest.mark.parametrize("source,name", [("host", "dpmpp_2m"), ("device", "dpmpp_2m"), ("host", "ddpm"),
                                         ("device", "ddim")])
def test_known_sharded_world1_equals_diffuser(model, cuda, source, name):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(12 if name == "ddpm" else 1000, device=cuda)
    d.noise_source = source
    g = torch.Generator().manual_seed(201)
    vals = torch.rand((5, 12), generator=g).to(cuda)
    cmask = (torch.rand((5, 12), generator=g) > 0.3).float().to(cuda)
    z0 = torch.randn((5, 4, 16, 16), generator=g)
    kw = dict(cond=vals, cond_mask=cmask, init_latent=z0, mask=box_mask(5, 16, fractional=True), strength=0.6,
              **SAMPLERS[name])
    torch.manual_seed(202)
    lat = dd.ShardedCondSampler(d, model, None).sample({1: 3, 3: 2}, decode=False, **kw)
    s_sharded = torch.get_rng_state()
    torch.manual_seed(202)
    single = d.sample_latent_cond(model, {1: 3, 3: 2}, vae=None, progress=False, **kw)
    assert torch.equal(lat.cpu(), single.cpu()) and torch.isfinite(single).all()
    assert torch.equal(s_sharded, torch.get_rng_state())
    with pytest.raises(ValueError):
        dd.ShardedCondSampler(d, model, None).sample({1: 3, 3: 2}, z_shape=(4, 16, 16), decode=False, strength=0.5)


def test_known_entity_csv_sampler(model, vae, cuda):
    import os

    import diff
    from conftest import GOLDEN
    from entityCsvSampler import EntityCsvSampler
    csv = os.path.join(GOLDEN, "entities.csv")
    d = diff.Diffuser(1000, device=cuda)
    s = EntityCsvSampler(d, model, vae, class_id=1, base_wh=(400, 400), device=cuda)
    torch.manual_seed(209)
    with torch.no_grad():
        z0 = vae.encode(torch.rand((1, 3, 128, 128), device=cuda))[0]  # an image's latent: (1,4,16,16)
    assert tuple(z0.shape) == (1, 4, 16, 16)
    mask = box_mask(1, 16)[0, 0]
    kw = dict(sampler="dpmpp_2m", steps=5, init_latent=z0, mask=mask, strength=0.8)
    torch.manual_seed(210)
    imgs = s.sample(csv, count=2, start=1, guidance_scale=3.0, **kw)
    vals, cmask = s.load_cond(csv, count=2, start=1)
    torch.manual_seed(210)
    exp = d.sample_latent_cond(model, (1, 2), vae=vae, guidance_scale=3.0, cond=vals, cond_mask=cmask,
                               progress=False, **kw)
    assert len(imgs) == len(exp) == 2
    for a, b in zip(imgs, exp):
        assert a.size == b.size == (128, 128) and np.array_equal(np.asarray(a), np.asarray(b))


# ---- 9: foreign (duck-typed) models: the blend as a launch of its own -------------------------------
MIX_W, MIX_MU, MIX_STD = (0.4, 0.6), (-1.0, 0.6), 0.25


def mixture_eps(x, ab_t):
    """test_gpu_dpm.py's closed-form eps of a per-element two-component Gaussian mixture."""
    import math
    a, s = torch.sqrt(ab_t).view(-1, 1, 1, 1), torch.sqrt(1 - ab_t).view(-1, 1, 1, 1)
    var = a * a * MIX_STD ** 2 + s * s
    dk = torch.stack([x - a * mu for mu in MIX_MU])
    logit = torch.stack([math.log(w) - dk[k] ** 2 / (2 * var) for k, w in enumerate(MIX_W)])
    r = torch.softmax(logit, dim=0)
    return s * (r * dk).sum(0) / var


class MixtureModel(torch.nn.Module):  # duck-typed: no .native()
    def __init__(self, alpha_bars, as_tuple=False):
        super().__init__()
        self.ab, self.as_tuple = alpha_bars, as_tuple

    def forward(self, x, t, y, cond_vals=None, cond_mask=None):
        e = mixture_eps(x, self.ab[t - 1])
        return (e, None) if self.as_tuple else e


@pytest.mark.parametrize("mode", [("ddim", 6, 0.0), ("dpm", 6, "logsnr")])
def test_known_foreign_model_matches_restatement(cuda, mode):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    B, hw, S, strength = 3, 8, mode[1], 0.7
    p0 = d._known_start(strength, S)
    assert p0 == 4
    g = torch.Generator().manual_seed(300)
    z0 = torch.randn((B, 4, hw, hw), generator=g)
    m = torch.rand((B, 1, hw, hw), generator=g)
    m[:, :, :3] = 0.0
    m[:, :, 5:] = 1.0
    skw = dict(sampler="dpmpp_2m", steps=S) if mode[0] == "dpm" else dict(sampler="ddim", steps=S)
    mdl = MixtureModel(d.alpha_bars)
    ab = d._host[1]
    # the bound is TOL per step; the whole run of p0 steps is held to one TOL here, which asks more
    torch.manual_seed(301)
    got = d.sample_latent_cond(mdl, {1: B}, vae=None, progress=False, guidance_scale=0.0, init_latent=z0, mask=m,
                               strength=strength, **skw)
    torch.manual_seed(301)
    e0 = torch.randn((B, 4, hw, hw))
    exp = known_trajectory(d, mode, e0, z0, m, p0, lambda x, t, pos: mixture_eps(x, ab[t - 1]))
    err = rel(got, exp)
    print(f"[known foreign {mode}] rel-L2 vs the fp32 CPU restatement = {err:.3e}")
    assert err <= TOL, err
    keep = (m == 0).expand_as(z0)
    assert torch.equal(got.cpu()[keep], z0[keep])


def test_known_foreign_model_ddpm(cuda):
    """The DDPM update of a foreign model followed by the blend: all ones is the plain call, all zeros z0."""
    import diff
    d = diff.Diffuser(10, device=cuda)
    mdl = MixtureModel(d.alpha_bars, as_tuple=True)
    z0 = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(310))

    def run(**extra):
        torch.manual_seed(311)
        return d.sample_latent_cond(mdl, {1: 2}, z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=1.0,
                                    **extra).cpu()

    plain = run()
    assert torch.equal(run(init_latent=z0, mask=torch.ones((8, 8))), plain)
    assert torch.equal(run(init_latent=z0, mask=torch.zeros((8, 8))), z0)
    half = torch.zeros((8, 8))
    half[:, 4:] = 1.0
    out = run(init_latent=z0, mask=half, strength=0.5)
    assert torch.equal(out[..., :4], z0[..., :4]) and torch.isfinite(out).all()
    assert not (out[..., 4:] == z0[..., 4:]).any()
