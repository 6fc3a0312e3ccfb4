"""CPU-only: DDIM inversion — the row tables against a float64 restatement, the argument rules of
invert_latent_cond and of sample_latent_cond's start_latent, the graph-key program, and the round-trip
property of the maths on the oracle network (no GPU: torch fp32 throughout).

Definitions: tau = ddim_timesteps(S), tau_0 = 0 with ab[0] := 1, p0 = _known_start(strength, S).
Position p = 1..p0 goes from s = tau_{p-1} up to t = tau_p in the rows k = 0..R,
  i_x = sqrt(ab[t]/ab[s]),  i_e = sqrt(1-ab[t]) - i_x sqrt(1-ab[s]),  y = i_x src + i_e eps(x, t_eval),
  t_eval = s (tau_1 at p = 1) for k = 0 and t for k >= 1;  x <- y;  adv = (k == R): src <- y.
The N = p0 (R+1) rows are stored in countdown order: the counter c = N..1 reads row c - 1, j = N - c.

This module also holds the torch restatement of the loop that tests/test_gpu_invert.py compares the
GPU against (invert_ref, ddim_back_ref)."""
import math
import os
import shutil
import subprocess

import pytest
import torch

import diff
from conftest import REPO
from oracle import rules
from oracle.rules import cfg_eps, invert_update, rel


# ---- the loops on the rules of oracle/rules.py --------------------------------------------------------
def invert_ref(z0, tables, eps_of):
    """The whole loop from x == src == z0; eps_of(x, t) -> eps at the network timesteps t (B,)."""
    N = int(tables[0].numel())
    x, src = z0, z0
    with torch.no_grad():
        for c in range(N, 0, -1):
            pos = torch.full((z0.shape[0],), c, dtype=torch.long)
            x, src = invert_update(src, eps_of(x, tables[0][pos - 1]), pos, tables)
    return x


def ddim_back_ref(x, sched, p0, eps_of):
    """DDIM eta = 0 from position p0 down to 1."""
    return rules.trajectory(x, "ddim", sched, lambda x, t, pos: eps_of(x, t), p0=p0)


def round_trip_inputs():
    """The inputs of the round-trip property, in the draw order the issue fixes."""
    g = torch.Generator().manual_seed(5)
    z0 = 0.8 * torch.randn((2, 4, 16, 16), generator=g)
    vals = torch.rand((2, 12), generator=g)
    mask = (torch.rand((2, 12), generator=g) > 0.3).float()
    return z0, torch.tensor([1, 3]), vals, mask


def perturbation_gain(z0, tables, eps_of, scale=1e-5):
    """How much of a `scale` relative perturbation of z0 the restatement passes on (1 = all of it)."""
    g = torch.Generator().manual_seed(77)
    dz = torch.randn(z0.shape, generator=g)
    dz = dz * (scale * z0.norm() / dz.norm())
    a, b = invert_ref(z0, tables, eps_of), invert_ref(z0 + dz, tables, eps_of)
    return rel(b, a) / scale


# ---- 1: the tables -------------------------------------------------------------------------------
@pytest.mark.parametrize("S,strength,R", [(20, None, 0), (20, 0.3, 2), (1000, None, 0), (7, 0.5, 1)])
def test_invert_tables_against_float64(S, strength, R):
    d = diff.Diffuser(1000)
    t_eval, i_x, i_e, adv = d.invert_tables(S, strength, R)
    tau = d.ddim_timesteps(S)
    p0 = d._known_start(strength, S)
    N = p0 * (R + 1)
    assert (t_eval.dtype, i_x.dtype, i_e.dtype, adv.dtype) == (torch.long, torch.float32, torch.float32, torch.int32)
    assert all(v.shape == (N,) and v.is_contiguous() for v in (t_eval, i_x, i_e, adv))
    ab = [1.0] + [float(v) for v in d._host[1].double()]
    tau0 = [0] + tau
    for c in range(N, 0, -1):  # the countdown order: c reads row c - 1, the forward index is N - c
        j = N - c
        p, k = j // (R + 1) + 1, j % (R + 1)
        s, t = tau0[p - 1], tau0[p]
        ix = math.sqrt(ab[t] / ab[s])
        ie = math.sqrt(1 - ab[t]) - ix * math.sqrt(1 - ab[s])
        assert int(t_eval[c - 1]) == ((s if p > 1 else tau[0]) if k == 0 else t)
        assert float(i_x[c - 1]) == float(torch.tensor(ix, dtype=torch.float64).float())
        assert float(i_e[c - 1]) == float(torch.tensor(ie, dtype=torch.float64).float())
        assert int(adv[c - 1]) == (1 if k == R else 0)
    assert int(t_eval[N - 1]) == tau[0]  # p = 1, k = 0: there is no timestep 0
    assert bool((i_x <= 1).all()) and bool((i_x > 0).all())
    # adv is set exactly once per position, on the row the countdown reads last
    rows = adv.view(p0, R + 1)  # (row c - 1 = N - 1 - j: positions descend, and so do the k within one)
    assert bool((rows.sum(1) == 1).all()) and bool((rows[:, 0] == 1).all())
    # the p = 1 rows are (sqrt(ab), sqrt(1 - ab)) of tau_1
    ab1 = d._host[1].double()[tau[0] - 1]
    for k in range(R + 1):
        c = N - k
        assert float(i_x[c - 1]) == float(torch.sqrt(ab1).float())
        assert float(i_e[c - 1]) == float(torch.sqrt(1 - ab1).float())
    assert d.invert_tables(S, strength, R) is d.invert_tables(S, strength, R)  # cached


def test_invert_tables_argument_rules():
    d = diff.Diffuser(40)
    for bad in (dict(steps=0), dict(steps=41), dict(steps=4.0), dict(steps=4, refine=-1), dict(steps=4, refine=1.0),
                dict(steps=4, refine=True), dict(steps=4, strength=0.0), dict(steps=4, strength=1.5)):
        with pytest.raises(ValueError):
            d.invert_tables(**bad)


# ---- 2: argument rules of the two public entries ----------------------------------------------------
def test_invert_latent_cond_argument_rules():
    d = diff.Diffuser(40)
    z = torch.randn(2, 4, 6, 5)
    ok = dict(model=None, init_latent=z, class_counts=(1, 2), steps=4)
    bad_calls = [
        dict(refine=-1), dict(refine=1.5), dict(refine="2"), dict(refine=True), dict(refine=None),
        dict(steps=0), dict(steps=41), dict(steps=None), dict(steps=2.0),
        dict(strength=0.0), dict(strength=1.5), dict(strength=float("nan")),
        dict(guidance_scale=-1.0), dict(guidance_scale=float("inf")), dict(guidance_scale=[3.0, 3.0]),
        dict(init_latent=None), dict(init_latent=torch.randn(3, 4, 6, 5)), dict(init_latent=torch.randn(6, 5)),
        dict(init_latent=[[1.0]]),
        dict(class_counts={1: 0}),
        dict(cond=torch.zeros(3, 12)),
    ]
    torch.manual_seed(3)
    before = torch.get_rng_state()
    for kw in bad_calls:
        with pytest.raises(ValueError):
            d.invert_latent_cond(**{**ok, **kw})
    assert torch.equal(torch.get_rng_state(), before)


def test_start_latent_argument_rules():
    d = diff.Diffuser(40)
    z = torch.randn(2, 4, 6, 5)
    ok = dict(model=None, class_counts=(1, 2), progress=False)
    ddim = dict(sampler="ddim", steps=4)
    bad_calls = [
        dict(start_latent=z),                                            # the ddpm sampler walks every timestep
        dict(start_latent=z, strength=0.5),
        dict(start_latent=z, init_latent=z, **ddim),
        dict(start_latent=z, init_latent=z, strength=0.5, **ddim),
        dict(start_latent=z, mask=torch.ones(6, 5), **ddim),
        dict(start_latent=z, strength=0.0, **ddim),
        dict(start_latent=z, strength=1.5, **ddim),
        dict(start_latent=z, z_shape=(4, 6, 6), **ddim),                 # disagrees with z_shape
        dict(start_latent=torch.randn(3, 4, 6, 5), **ddim),              # 3 samples for a batch of 2
        dict(start_latent=[[1.0]], **ddim),
        dict(strength=0.5, z_shape=(4, 6, 5), **ddim),                   # strength alone still raises, as today
        dict(strength=0.5, z_shape=(4, 6, 5)),
    ]
    torch.manual_seed(3)
    before = torch.get_rng_state()
    for kw in bad_calls:
        with pytest.raises(ValueError):
            d.sample_latent_cond(**ok, **kw)
    assert torch.equal(torch.get_rng_state(), before)


def test_start_latent_enters_the_loop_as_it_is_and_draws_nothing():
    d = diff.Diffuser(40)
    d._latent_shape = lambda *a, **k: (_ for _ in ()).throw(AssertionError("_latent_shape called"))
    seen = {}

    def loop(model, x, *a, **k):
        seen["x"], seen["mode"], seen["kw"] = x, a[6], k
        return x

    d._run_cond_loop = loop
    z = torch.randn(4, 6, 5)
    before = torch.get_rng_state()
    for sampler, rule in (("ddim", "ddim"), ("dpmpp_2m", "dpm")):
        out = d.sample_latent_cond(None, (1, 3), progress=False, start_latent=z, strength=0.3, sampler=sampler, steps=20)
        assert torch.equal(out, z.expand(3, 4, 6, 5)) and seen["mode"][0] == rule
        assert seen["kw"]["start"] == 6 and seen["kw"]["known"] is None
    out = d.sample_latent_cond(None, (1, 3), progress=False, start_latent=z, sampler="ddim", steps=20)
    assert seen["kw"]["start"] == 20
    assert torch.equal(torch.get_rng_state(), before)
    # without the keyword the loop is called as it always was
    d.sample_latent_cond(None, (1, 3), z_shape=(4, 6, 5), progress=False, sampler="ddim", steps=20)
    assert "start" not in seen["kw"]


def test_plans_of_the_two_entries():
    d = diff.Diffuser(1000)
    x = torch.randn(2, 4, 6, 5)
    plan = d._plan(x, ("invert", 20, 0.3, 2), 3.0)
    assert plan.rule == "invert" and plan.start == 18 and not plan.draws and plan.scale == 3.0
    assert plan.sched is d.invert_tables(20, 0.3, 2, x.device) and plan.x_start is x
    src = plan.new_hist(x)
    assert torch.equal(src, x) and src.data_ptr() != x.data_ptr()
    assert plan.kwargs(True, src, seed=0, use_graph=True) == dict(seed=0, use_graph=True, invert=(plan.sched, src))
    with pytest.raises(ValueError):
        d._plan(x, ("invert", 20, 0.3, 2), 3.0, rescale=0.5)
    # a start-latent plan: the strided plan entered at p0; DPM's entry row is first-order
    plan = d._plan(x, ("ddim", 20, 0.0), 3.0, start=6)
    assert plan.rule == "ddim" and plan.start == 6 and plan.x_start is x and plan.known is None
    plan = d._plan(x, ("dpm", 20, "logsnr"), 3.0, start=6)
    assert plan.sched is d.dpm_tables(20, "logsnr", x.device, 6) and float(plan.sched[5][5]) == 0.0
    with pytest.raises(ValueError):
        d._plan(x, None, 3.0, start=6)


# ---- 3: the graph-key program -----------------------------------------------------------------------
def test_step_mode_check_builds_and_passes(tmp_path):
    rocm_clang = os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..", "llvm", "bin",
                              "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which(rocm_clang)
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / "step_mode_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), "-I",
                    os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    os.path.join(REPO, "tools", "step_mode_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "step_mode_check: ok" in out
    src = open(os.path.join(REPO, "tools", "step_mode_check.cpp")).read()
    assert "invert" in src  # the inversion cases are part of it


# ---- 4: the property the feature exists for, on the restatement alone -------------------------------
def test_round_trip_of_the_restatement(unet_sd):
    """Invert over the first 6 of 20 positions (t <= 300), sample back with DDIM eta = 0 under the same
    condition at CFG 3.0.  Measured here: R = 0 2.4e-1, R = 3 1.6e-3 (the GPU test's conditions are
    err(R=3) <= 1e-2, err(R=0) >= 5e-2, err(R=3) < err(R=0)/10)."""
    d = diff.Diffuser(1000)
    z0, y, vals, mask = round_trip_inputs()
    sched = d.ddim_tables(20, 0.0)

    def eps_of(x, t):
        return cfg_eps(unet_sd, x, t, y, vals, mask, 3.0)

    errs = {}
    for R in (0, 3):
        x = invert_ref(z0, d.invert_tables(20, 0.3, R), eps_of)
        errs[R] = rel(ddim_back_ref(x, sched, 6, eps_of), z0)
        print(f"[round trip, CPU restatement] R={R}: rel-L2 = {errs[R]:.3e}")
    assert errs[3] <= 1e-2 and errs[0] >= 5e-2 and errs[3] < errs[0] / 10, errs
    gain = perturbation_gain(z0, d.invert_tables(20, 0.3, 3), eps_of)
    print(f"[round trip, CPU restatement] gain of a 1e-5 perturbation of z0 through the inversion: {gain:.2f}")
    assert gain < 2.0, gain
