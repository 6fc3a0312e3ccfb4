"""GPU: geometry guidance — the data-only backward to the network input (dmx_train_backward_input), the
loss seed and the mix (dmx_geom_seed / dmx_geom_mix), the geometry-guided step and loop
(dmx_step_geom / dmx_sample_loop_geom) and the samplers' geom_scale keyword — against the CPU oracle:
oracle.train_ref.forward with x as an autograd leaf and the per-sample loss
  L_n = sum_j m_nj (geom_nj - v_nj)^2 / max(sum_j m_nj, 1e-6)
summed, and torch restatements of  eps' = eps + (s_n sqrt(1 - ab_t)) dL_n/dx  and of the three updates.

Bounds are the project's: GRAD_TOL = 1e-4 per-sample rel-L2 for a gradient (test_gpu_train.py), that
file's rtol 1e-4 / atol 2e-5 for loss and geom, TOL = 2e-5 for one step.  A guided step against the
oracle's own gradient is held to TOL + GRAD_TOL * share, share = |x'_guided - x'_plain| / |x'_guided|
from the oracle: the step bound plus the gradient bound times the part of the update that guidance
moves; share >= 0.05 is asserted in every case so that a no-op cannot pass.

Measured on an MI355X (rel-L2): geom_grad's gradient per sample 1.9e-6 .. 3.8e-6, the empty-mask
row exactly 0; input_grad with d_eps alone / both cotangents 1.8e-6 .. 2.3e-6; row 0 alone 2.0e-6 .. 3.8e-6;
guided steps on the GPU's own gradient 4.0e-7 .. 7.3e-7 (DPM history 2.8e-7 .. 4.4e-7); guided steps against
the oracle 5.9e-7 .. 2.0e-6 at shares 0.093 .. 0.76 (bounds 2.9e-5 .. 9.6e-5); the bit-equalities hold; the
guided loop lowers the final masked loss 0.28616 -> 0.26291 (8.1 %), as the oracle's loop does."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref, train_ref
from oracle.rules import ddim_update, dpm_update, rel
from support import make_model, make_vae, per_sample_rel, run_worker

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4   # a gradient against the oracle, per sample (the project's gradient bound)
TOL = 2e-5        # one step (the project's step bound)
G = 3.0
S_STEP = 2000.0   # the guided steps' scale
SHAPES = [(3, 8), (3, 16), (2, 28)]


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    return make_model(cuda, unet_sd)


@pytest.fixture(scope="module")
def model2(cuda, unet_sd):
    """A second network with the same weights: its own arena and its own graph slots."""
    return make_model(cuda, unet_sd)


# ---- the torch restatements ---------------------------------------------------------------------
def loss_rows(geom, vals, mask):
    """masked_geom_mse row by row."""
    return (mask * (geom - vals).pow(2)).sum(-1) / mask.sum(-1).clamp_min(1e-6)


def oracle_grad(sd, x, t, y, vals, mask, d_eps=None, with_geom=True):
    """The oracle's forward with x a leaf -> (loss rows, dL/dx, geom, eps); L = the summed per-sample
    loss (with_geom) plus <d_eps, eps>."""
    xl = x.clone().requires_grad_(True)
    eps, geom = train_ref.forward(sd, xl, t, y, vals, mask)
    rows = loss_rows(geom, vals, mask)
    total = rows.sum() if with_geom else geom.sum() * 0.0
    if d_eps is not None:
        total = total + (eps * d_eps).sum()
    g, = torch.autograd.grad(total, xl)
    return rows.detach(), g, geom.detach(), eps.detach()


def mix_ref(eps, grad, scale, sig, pos):
    """eps' = eps + (scale sig[pos-1]) grad, one rounding per torch op; eps's bits where scale or grad is 0."""
    s = scale.view(-1, 1, 1, 1)
    k = (scale * sig[pos - 1]).view(-1, 1, 1, 1)
    return torch.where((s == 0) | (grad == 0), eps, eps + k * grad)


def case(B, hw, seed, ts):
    """x, t, y, vals, mask: the last row's mask all zero, one row with label 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, hw, hw), generator=g)
    y = torch.tensor([2, 0, 3][:B])
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    mask[-1] = 0.0
    return x, torch.tensor(ts[:B]), y, vals, mask


_GRAD_REF = {}


def grad_ref(sd, B, hw):
    """Inputs at t = {1, 500, 1000} and the oracle's loss / gradient / geom / eps, once per shape."""
    if (B, hw) not in _GRAD_REF:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        inp = case(B, hw, 30 + hw, [1, 500, 1000])
        _GRAD_REF[(B, hw)] = (inp, oracle_grad(sd, *inp))
    return _GRAD_REF[(B, hw)]


# ---- 1: the input gradient against the oracle -----------------------------------------------------
@pytest.mark.parametrize("B,hw", SHAPES)
def test_input_gradient_vs_oracle(model, cuda, unet_sd, B, hw):
    """Measured (per-sample rel-L2 vs the oracle): geom_grad 2.0e-6, 1.9e-6, 0 at 8x8; 2.8e-6, 3.6e-6, 0 at
    16x16; 3.8e-6, 0 at 28x28.  input_grad with d_eps alone / both cotangents: 1.8e-6 / 1.9e-6, 2.3e-6 /
    2.3e-6, 2.2e-6 / 2.2e-6."""
    (x, t, y, vals, mask), (rows, g_ref, geom_ref, eps_ref) = grad_ref(unet_sd, B, hw)
    dv = [v.to(cuda) for v in (x, t, y, vals, mask)]
    was_training = model.training
    with torch.no_grad():
        loss, grad, geom, eps = model.geom_grad(*dv)
    assert not model.training and not was_training and not grad.requires_grad
    errs = per_sample_rel(grad, g_ref)
    print(f"[geom_grad B={B} {hw}x{hw}] per-sample rel-L2 vs oracle = {[f'{e:.2e}' for e in errs]}")
    assert max(errs) <= GRAD_TOL, errs
    assert bool((grad[-1] == 0).all()) and float(loss[-1]) == 0.0   # the empty-mask row: exactly zero
    assert float(g_ref[-1].abs().max()) == 0.0
    assert float(grad[0].abs().max()) > 0
    np.testing.assert_allclose(loss.cpu().numpy(), rows.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(geom.cpu().numpy(), geom_ref.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(eps.cpu().numpy(), eps_ref.numpy(), rtol=1e-4, atol=2e-5)
    # input_grad with a random d_eps alone, and with both cotangents (the seed = dL/dgeom)
    nm = model.native()
    gen = torch.Generator().manual_seed(31 + hw)
    d_eps = torch.randn(x.shape, generator=gen)
    den = mask.sum(-1, keepdim=True).clamp_min(1e-6)
    _, geom_n, tape = nm.train_forward(*dv)
    seed = 2 * mask * (geom_n.cpu() - vals) / den
    only = nm.input_grad(tape, d_eps.to(cuda), None)
    both = nm.input_grad(tape, d_eps.to(cuda), seed.to(cuda))
    _, r_only, _, _ = oracle_grad(unet_sd, x, t, y, vals, mask, d_eps, with_geom=False)
    _, r_both, _, _ = oracle_grad(unet_sd, x, t, y, vals, mask, d_eps)
    e1, e2 = per_sample_rel(only, r_only), per_sample_rel(both, r_both)
    print(f"[input_grad B={B} {hw}x{hw}] d_eps alone {max(e1):.2e}, both cotangents {max(e2):.2e}")
    assert max(e1) <= GRAD_TOL and max(e2) <= GRAD_TOL, (e1, e2)


# ---- 2: a row does not depend on the batch ---------------------------------------------------------
@pytest.mark.parametrize("B,hw", SHAPES)
def test_row_does_not_depend_on_the_batch(model, cuda, unet_sd, B, hw):
    (x, t, y, vals, mask), (rows, g_ref, _, _) = grad_ref(unet_sd, B, hw)
    dv = [v[:1].to(cuda).contiguous() for v in (x, t, y, vals, mask)]
    loss, grad, _, _ = model.geom_grad(*dv)
    err = per_sample_rel(grad, g_ref[:1])[0]
    print(f"[geom_grad row 0 alone {hw}x{hw}] rel-L2 vs the oracle's in-batch row = {err:.2e}")
    assert err <= GRAD_TOL, err
    np.testing.assert_allclose(loss.cpu().numpy(), rows[:1].numpy(), rtol=1e-4, atol=2e-5)


# ---- 3: the parameter backward is untouched ---------------------------------------------------------
def test_parameter_backward_untouched_and_stale_tape(model, cuda, unet_sd):
    import diff
    from dmx import _lib
    nm = model.native()
    (x, t, y, vals, mask), _ = grad_ref(unet_sd, 3, 8)
    dv = [v.to(cuda) for v in (x, t, y, vals, mask)]
    gen = torch.Generator().manual_seed(5)
    d_eps = torch.randn(x.shape, generator=gen).to(cuda)
    d_geom = torch.randn((3, 12), generator=gen).to(cuda)
    _, _, tape = nm.train_forward(*dv)
    want = nm.train_backward(tape, d_eps, d_geom)
    _, _, tape = nm.train_forward(*dv)
    dx = nm.input_grad(tape, d_eps, d_geom)
    got = nm.train_backward(tape, d_eps, d_geom)
    assert torch.isfinite(dx).all()
    assert [k for k in want if not torch.equal(want[k], got[k])] == []
    assert torch.equal(dx, nm.input_grad(tape, d_eps, d_geom))     # and it repeats bit for bit
    with pytest.raises(_lib.DmxError, match="stale tape"):
        nm.input_grad(tape - 1, d_eps, d_geom)
    # a geometry-guided step replaces the tape
    d = diff.Diffuser(1000, device=cuda)
    out = torch.empty_like(dv[0])
    scale = torch.full((3,), S_STEP, device=cuda)
    nm.step(dv[0], out, dv[1], dv[2], 0, dv[3], dv[4], G, d.coef_tables(cuda, True), torch.zeros_like(dv[0]),
            geom=(scale, d.geom_sig(cuda)))
    with pytest.raises(_lib.DmxError, match="stale tape"):
        nm.train_backward(tape, d_eps, d_geom)
    with pytest.raises(_lib.DmxError, match="stale tape"):
        nm.input_grad(tape, d_eps, d_geom)


# ---- 4: geom_mix against its restatement, bit for bit --------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 8, 8), (2, 3, 5, 7), (1, 1, 1, 1)])
def test_geom_mix_vs_restatement(cuda, shape):
    from dmx import engine
    gen = torch.Generator().manual_seed(sum(shape))
    n = shape[0]
    eps, grad = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen) * 1e-3
    grad.view(-1)[::3] = 0.0
    eps.view(-1)[0] = -0.0
    sig = torch.rand((7,), generator=gen)
    pos = torch.tensor([7, 1, 4][:n])
    scale = torch.tensor([1500.0, 0.0, 2.5e3][:n])
    if n > 1:
        grad[1].view(-1)[1] = float("inf")     # a zero-scale row keeps eps's bits whatever the gradient
    exp = mix_ref(eps, grad, scale, sig, pos)
    out = engine.geom_mix(eps.to(cuda), grad.to(cuda), scale.to(cuda), sig.to(cuda), pos.to(cuda)).cpu()
    assert torch.equal(out.view(torch.int32), exp.view(torch.int32))
    if n > 1:
        assert torch.equal(out[1].view(torch.int32), eps[1].view(torch.int32))
    assert not torch.equal(out[0], eps[0]) or shape == (1, 1, 1, 1)
    # a scalar scale and one position for every sample
    exp1 = mix_ref(eps, grad, torch.full((n,), 800.0), sig, torch.full((n,), 3))
    out1 = engine.geom_mix(eps.to(cuda), grad.to(cuda), 800.0, sig.to(cuda), torch.tensor([3])).cpu()
    assert torch.equal(out1.view(torch.int32), exp1.view(torch.int32))
    with pytest.raises(ValueError):
        engine.geom_mix(eps.to(cuda), grad.to(cuda), torch.ones(n + 1), sig.to(cuda), pos.to(cuda))
    with pytest.raises(ValueError):
        engine.geom_mix(eps.to(cuda), torch.cat([grad, grad], -1).to(cuda), scale, sig.to(cuda), pos.to(cuda))


# ---- 5, 6: the guided step ------------------------------------------------------------------------------
# The strided rules step from t = 500, 1000, 250: positions 2, 4, 1 of the 4-position schedules over
# T = 1000.  One DDPM step of that chain moves x by beta_t <= 0.02 of eps, so guidance could not reach
# a 5 % share of x' there: the DDPM rule steps a coarse chain instead (T = 8, beta up to 0.5) from
# t = 5, 8, 2.  Neither choice favours the code: the shares are the oracle's, checked on the CPU
# (8x8 / 16x16: ddpm 0.30 / 0.093, ddim 0.76 / 0.22, dpm 0.75 / 0.22).  The last row's mask is empty in both.
STEP_T = [500, 1000, 250]
STEP_POS = [2, 4, 1]
DDPM_T, DDPM_BETA_END, DDPM_ROWS = 8, 0.5, [5, 8, 2]
_STEP_REF = {}


def make_d(kind, dev):
    import diff
    return diff.Diffuser(DDPM_T, 1e-4, DDPM_BETA_END, device=dev) if kind == "ddpm" else diff.Diffuser(1000, device=dev)


def step_ref(sd, hw, kind):
    """Inputs and the oracle's eu / ec / gradient at the rule's timesteps, once per size and chain."""
    key = (hw, kind == "ddpm")
    if key not in _STEP_REF:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        x, t, y, vals, mask = case(3, hw, 50 + hw, DDPM_ROWS if kind == "ddpm" else STEP_T)
        gen = torch.Generator().manual_seed(51 + hw)
        hist, nz = torch.randn(x.shape, generator=gen), torch.randn(x.shape, generator=gen)
        _, g_ref, _, ec = oracle_grad(sd, x, t, y, vals, mask)
        with torch.no_grad():
            eu = train_ref.forward(sd, x, t, torch.zeros_like(y), vals, mask)[0]
        _STEP_REF[key] = (x, t, y, vals, mask, hist, nz, eu, ec, g_ref)
    return _STEP_REF[key]


def rule_tables(d, kind, dev):
    if kind == "ddpm":
        return d.coef_tables(dev, True), None, d.geom_sig(dev)
    sched = d.ddim_tables(4, 0.5, dev) if kind == "ddim" else d.dpm_tables(4, "uniform", dev)
    return None, sched, sched[1]


def update_ref(d, kind, x, eps, t, pos, nz, hist):
    """-> (x', hist') of the rule on the CPU."""
    if kind == "ddpm":
        _, a, ab = ref.schedule(DDPM_T, 1e-4, DDPM_BETA_END)
        return ref.ddpm_update(x, eps, t, a, ab, nz), None
    if kind == "ddim":
        return ddim_update(x, eps, pos, d.ddim_tables(4, 0.5, "cpu"), nz), None
    return dpm_update(x, eps, pos, d.dpm_tables(4, "uniform", "cpu"), hist)


def guided_step_ref(d, kind, sd, hw, grad, scale, nz=None):
    x, t, y, vals, mask, hist, nz0, eu, ec, _ = step_ref(sd, hw, kind)
    nz = nz0 if nz is None else nz
    pos = torch.tensor(STEP_POS)
    eg = eu + G * (ec - eu)
    sig = rule_tables(d, kind, "cpu")[2]
    eps = mix_ref(eg, grad, scale, sig, t if kind == "ddpm" else pos) if grad is not None else eg
    return update_ref(d, kind, x, eps, t, pos, nz, hist)


def native_guided_step(nm, d, cuda, kind, sd, hw, scale):
    x, t, y, vals, mask, hist, nz, _, _, _ = step_ref(sd, hw, kind)
    tables, sched, sig = rule_tables(d, kind, cuda)
    out, h = torch.empty(x.shape, device=cuda), hist.to(cuda)
    p = (t if kind == "ddpm" else torch.tensor(STEP_POS)).to(cuda)
    kw = dict(sched=sched) if sched is not None else {}
    if kind == "dpm":
        kw["hist"] = h
    nm.step(x.to(cuda), out, p, y.to(cuda), 0, vals.to(cuda), mask.to(cuda), G, tables,
            None if kind == "dpm" else nz.to(cuda), geom=(scale.to(cuda), sig), **kw)
    return out, h


@pytest.mark.parametrize("hw", [8, 16])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_guided_step_arithmetic(model, cuda, unet_sd, kind, hw):
    """eu / ec from the oracle, the gradient from the GPU's own geom_grad: the step's own arithmetic."""
    d = make_d(kind, cuda)
    x, t, y, vals, mask = step_ref(unet_sd, hw, kind)[:5]
    scale = torch.full((3,), S_STEP)
    grad = model.geom_grad(*(v.to(cuda) for v in (x, t, y, vals, mask)))[1].cpu()
    exp, exp_h = guided_step_ref(d, kind, unet_sd, hw, grad, scale)
    out, h = native_guided_step(model.native(), d, cuda, kind, unet_sd, hw, scale)
    err = rel(out, exp)
    print(f"[guided step {kind} {hw}x{hw}] rel-L2 vs restatement on the GPU's gradient = {err:.3e}")
    assert err <= TOL, err
    if kind == "dpm":
        eh = rel(h, exp_h)
        print(f"[guided step dpm {hw}x{hw}] history rel-L2 = {eh:.3e}")
        assert eh <= TOL, eh


@pytest.mark.parametrize("hw", [8, 16])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_guided_step_vs_oracle(model, cuda, unet_sd, kind, hw):
    """End to end: the oracle's gradient in the restatement; bound TOL + GRAD_TOL * share, share >= 0.05."""
    d = make_d(kind, cuda)
    scale = torch.full((3,), S_STEP)
    g_ref = step_ref(unet_sd, hw, kind)[9]
    exp, exp_h = guided_step_ref(d, kind, unet_sd, hw, g_ref, scale)
    plain, _ = guided_step_ref(d, kind, unet_sd, hw, None, scale)
    share = float((exp - plain).norm() / exp.norm())
    assert share >= 0.05, share
    out, h = native_guided_step(model.native(), d, cuda, kind, unet_sd, hw, scale)
    err = rel(out, exp)
    print(f"[guided step {kind} {hw}x{hw}] rel-L2 vs oracle = {err:.3e}, share = {share:.3f}, "
          f"bound = {TOL + GRAD_TOL * share:.3e}")
    assert err <= TOL + GRAD_TOL * share, (err, share)
    assert rel(out[-1], plain[-1]) <= TOL     # the empty-mask row is the plain step
    if kind == "dpm":
        assert rel(h, exp_h) <= TOL + GRAD_TOL * share


# ---- 7: geom_scale = 0 is today's loop -----------------------------------------------------------------
def test_zero_scale_is_the_plain_call(cuda, unet_sd):
    import diff
    mdl = make_model(cuda, unet_sd)
    nm = mdl.native()
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = "device"
    x, t, y, vals, mask = (v.to(cuda) for v in case(3, 8, 70, [9, 9, 9]))
    kw = dict(z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=G, cond=vals, cond_mask=mask, sampler="ddim",
              steps=9, eta=0.5)
    outs = []
    for extra in ({}, dict(geom_scale=0.0), dict(geom_scale=[0.0, 0.0, 0.0])):
        torch.manual_seed(71)
        outs.append(d.sample_latent_cond(mdl, {2: 1, 1: 1, 3: 1}, **kw, **extra).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.isfinite(outs[0]).all()
    plan = d._plan(x, ("ddim", 9, 0.5), G, geom=d._geom_args(0.0, 3))
    assert plan.geom is None and "geom" not in plan.kwargs(True, seed=1, use_graph=True)
    # a step and a device loop with geom=None are the plain ones; the plain loop's graph slot is reused
    sched = d.ddim_tables(9, 0.5, cuda)
    a, b = torch.empty_like(x), torch.empty_like(x)
    nm.step(x, a, torch.full((3,), 5, device=cuda), y, 0, vals, mask, G, None, None, seed=3, sched=sched)
    nm.step(x, b, torch.full((3,), 5, device=cuda), y, 0, vals, mask, G, None, None, seed=3, sched=sched, geom=None)
    assert torch.equal(a, b)
    xs, tt = torch.empty_like(x), torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(**extra):
        xs.copy_(x)
        tt.fill_(9)
        c0 = nm.graph_captures()
        nm.sample_loop(xs, tt, y, 0, vals, mask, G, None, 9, seed=3, sched=sched, **extra)
        torch.cuda.synchronize()
        return xs.clone(), nm.graph_captures() - c0

    first, cap1 = loop()
    second, cap2 = loop(geom=None)
    assert cap1 == 1 and cap2 == 0 and torch.equal(first, second)


# ---- 8: loop structure -----------------------------------------------------------------------------------
def loop_inputs(d, kind, cuda, S):
    x0, _, y, vals, mask = (v.to(cuda) for v in case(3, 8, 80, [1, 1, 1]))
    if kind == "ddpm":
        return x0, y, vals, mask, d.coef_tables(cuda, True), None, d.geom_sig(cuda)
    sched = d.ddim_tables(S, 1.0, cuda) if kind == "ddim" else d.dpm_tables(S, "logsnr", cuda)
    return x0, y, vals, mask, None, sched, sched[1]


@pytest.mark.parametrize("kind,steps", [("ddpm", 4), ("ddim", 4), ("dpm", 4), ("ddim", 10)])
def test_guided_loop_graph_eager_steps_fresh(model, model2, cuda, kind, steps):
    """A device loop (graph), the same loop eager, single steps, and a second model: bit-equal.  The
    10-step case replays the 8-step graph (the position scalar's ping-pong) and two 1-step graphs."""
    import diff
    d = diff.Diffuser(12 if kind == "ddpm" else 1000, device=cuda)
    S = 12
    x0, y, vals, mask, tables, sched, sig = loop_inputs(d, kind, cuda, S)
    scale = torch.tensor([1000.0, 0.0, 1500.0], device=cuda)
    kw = dict(sched=sched) if sched is not None else {}

    def loop(mdl, use_graph):
        x, hist = x0.clone(), torch.full_like(x0, float("nan"))
        t = torch.full((1,), S, dtype=torch.long, device=cuda)
        hk = dict(hist=hist) if kind == "dpm" else {}
        mdl.native().sample_loop(x, t, y, 0, vals, mask, G, tables, steps, seed=7, use_graph=use_graph,
                                 geom=(scale, sig), **kw, **hk)
        torch.cuda.synchronize()
        assert int(t.item()) == S - steps
        return x.cpu()

    graph, eager, again, fresh = loop(model, True), loop(model, False), loop(model, True), loop(model2, True)
    assert torch.isfinite(graph).all()
    for other in (eager, again, fresh):
        assert torch.equal(graph, other)
    nm = model.native()
    a, b, hist = x0.clone(), torch.empty_like(x0), torch.full_like(x0, float("nan"))
    hk = dict(hist=hist) if kind == "dpm" else {}
    for p in range(S, S - steps, -1):
        nm.step(a, b, torch.full((1,), p, dtype=torch.long, device=cuda), y, 0, vals, mask, G, tables, None, seed=7,
                t_stride=0, geom=(scale, sig), **kw, **hk)
        a, b = b, a
    assert torch.equal(a.cpu(), graph)
    # and the guidance moved the guided rows only
    x, hist = x0.clone(), torch.full_like(x0, float("nan"))
    t = torch.full((1,), S, dtype=torch.long, device=cuda)
    model.native().sample_loop(x, t, y, 0, vals, mask, G, tables, steps, seed=7, **kw,
                               **(dict(hist=hist) if kind == "dpm" else {}))
    plain = x.cpu()
    assert not torch.equal(plain[0], graph[0])
    assert rel(graph[1:], plain[1:]) <= TOL   # zero scale; empty mask: the plain loop (its eps goes through the arena)


def test_guided_and_plain_loops_keep_their_graphs(cuda, unet_sd):
    """Guided, plain, guided loops on one model, one x and one scalar capture 1, 1, 0 graph pairs."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    nm = make_model(cuda, unet_sd).native()   # a fresh arena and empty slots
    x0, _, y, vals, mask = (v.to(cuda) for v in case(2, 16, 81, [1, 1]))
    mask[-1] = 1.0
    sched = d.dpm_tables(10, "logsnr", cuda)
    scale = torch.full((2,), 1000.0, device=cuda)
    x, hist = torch.empty_like(x0), torch.empty_like(x0)
    t = torch.zeros((1,), dtype=torch.long, device=cuda)

    def loop(guided, use_graph=True):
        x.copy_(x0)
        hist.fill_(float("nan"))
        t.fill_(10)
        c0 = nm.graph_captures()
        nm.sample_loop(x, t, y, 0, vals, mask, G, None, 10, use_graph=use_graph, sched=sched, hist=hist,
                       **(dict(geom=(scale, sched[1])) if guided else {}))
        torch.cuda.synchronize()
        assert int(t.item()) == 0
        return x.clone(), nm.graph_captures() - c0

    want_g, _ = loop(True, use_graph=False)   # (the larger plan first: the arena will not grow below)
    want_p, _ = loop(False, use_graph=False)
    assert not torch.equal(want_g, want_p)
    for guided, captures, want in ((True, 1, want_g), (False, 1, want_p), (True, 0, want_g)):
        out, cap = loop(guided)
        assert cap == captures, (guided, cap, captures)
        assert torch.equal(out, want)


# ---- 9: with a known region ---------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
def test_known_region_with_geometry_guidance(model, cuda, source):
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    gen = torch.Generator().manual_seed(920)
    B = 2
    z0 = torch.randn((B, 4, 8, 8), generator=gen)
    m = torch.ones((B, 1, 8, 8))
    m[:, :, :, :4] = 0.0          # keep the left half
    vals = torch.rand((B, 12), generator=gen)
    mask = (torch.rand((B, 12), generator=gen) > 0.3).float()
    kw = dict(z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=G, cond=vals.to(cuda),
              cond_mask=mask.to(cuda), sampler="dpmpp_2m", steps=6, init_latent=z0.to(cuda), mask=m.to(cuda),
              strength=0.7)
    torch.manual_seed(923)
    out = d.sample_latent_cond(model, {1: 1, 3: 1}, geom_scale=1000.0, **kw).cpu()
    torch.manual_seed(923)
    plain = d.sample_latent_cond(model, {1: 1, 3: 1}, **kw).cpu()
    keep = (m == 0).expand_as(z0)
    assert torch.equal(out[keep], z0[keep]) and torch.equal(plain[keep], z0[keep])
    assert torch.isfinite(out).all() and not torch.equal(out, plain)


# ---- 10: the sampler surface --------------------------------------------------------------------------------
@pytest.mark.parametrize("case_name,kw", [("ddpm", dict()), ("ddim", dict(sampler="ddim", steps=6, eta=0.5)),
                                           ("dpmpp_2m", dict(sampler="dpmpp_2m", steps=6))])
def test_sampler_equals_own_step_loop(model, cuda, case_name, kw):
    """Host-noise mode: sample_latent_cond(geom_scale=s) is the loop over NativeModel.step, bit for bit."""
    import diff
    T = 8 if case_name == "ddpm" else 1000
    d = diff.Diffuser(T, device=cuda)
    d.noise_source = "host"
    B = 3
    _, _, _, vals, mask = (v.to(cuda) for v in case(B, 8, 90, [1, 1, 1]))
    y = torch.tensor([1, 1, 3], device=cuda)
    gs = [1000.0, 0.0, 500.0]
    torch.manual_seed(91)
    out = d.sample_latent_cond(model, {1: 2, 3: 1}, z_shape=(4, 8, 8), vae=None, progress=False, guidance_scale=G,
                               cond=vals, cond_mask=mask, geom_scale=gs, **kw)
    assert d.range_fallbacks == 0
    torch.manual_seed(91)
    x = torch.randn((B, 4, 8, 8)).to(cuda)
    mode = d._sampler_mode(kw.get("sampler", "ddpm"), kw.get("steps"), kw.get("eta", 0.0), None, T)
    nm = model.native()
    scale = torch.tensor(gs, device=cuda)
    if mode is None:
        tables, sched, sig, S, draws = d.coef_tables(cuda, True), None, d.geom_sig(cuda), T, True
    elif mode[0] == "ddim":
        sched = d.ddim_tables(mode[1], mode[2], cuda)
        tables, sig, S, draws = None, sched[1], 6, True
    else:
        sched = d.dpm_tables(mode[1], mode[2], cuda)
        tables, sig, S, draws = None, sched[1], 6, False
    hist = torch.empty_like(x)
    for p in range(S, 0, -1):
        nz = torch.randn(x.shape).to(cuda) if draws else None
        nxt = torch.empty_like(x)
        nm.step(x, nxt, torch.full((B,), p, device=cuda), y, 0, vals, mask, G, tables, nz, geom=(scale, sig),
                **(dict(sched=sched) if sched is not None else {}), **(dict(hist=hist) if not draws else {}))
        x = nxt
    assert torch.isfinite(out).all() and torch.equal(out, x)


@pytest.mark.parametrize("source,kw", [("device", dict(sampler="dpmpp_2m", steps=6)),
                                       ("host", dict(sampler="ddim", steps=5, eta=1.0))])
def test_sharded_world1_equals_diffuser(model, cuda, source, kw):
    import diff
    from dmx import distributed as dd
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = source
    _, _, _, vals, mask = (v.to(cuda) for v in case(3, 8, 95, [1, 1, 1]))
    gkw = dict(geom_scale=[1000.0, 250.0, 0.0], guidance_scale=G)
    torch.manual_seed(902)
    lat = dd.ShardedCondSampler(d, model, None).sample({1: 2, 3: 1}, z_shape=(4, 8, 8), cond=vals, cond_mask=mask,
                                                       decode=False, **kw, **gkw)
    s_sharded = torch.get_rng_state()
    torch.manual_seed(902)
    single = d.sample_latent_cond(model, {1: 2, 3: 1}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals,
                                  cond_mask=mask, **kw, **gkw)
    assert torch.equal(lat.cpu(), single.cpu()) and torch.isfinite(single).all()
    assert torch.equal(s_sharded, torch.get_rng_state())
    torch.manual_seed(902)
    plain = d.sample_latent_cond(model, {1: 2, 3: 1}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals,
                                 cond_mask=mask, guidance_scale=G, **kw)
    assert not torch.equal(plain, single)
    assert torch.equal(s_sharded, torch.get_rng_state())   # the draw order does not depend on the guidance


def test_entity_csv_sampler_passes_geom_scale(model, cuda, vae_sd):
    import diff
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
    same = s.sample(csv, geom_scale=0.0, **kw)
    torch.manual_seed(510)
    other = s.sample(csv, geom_scale=2000.0, **kw)
    vals, mask = s.load_cond(csv, count=2, start=1)
    torch.manual_seed(510)
    exp = d.sample_latent_cond(model, (1, 2), vae=vae, guidance_scale=3.0, cond=vals, cond_mask=mask,
                               sampler="dpmpp_2m", steps=4, progress=False, geom_scale=2000.0)
    for a, b in zip(plain, same):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(other, exp):      # the keyword passes through
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_foreign_model_guided_step_vs_oracle(model, cuda, unet_sd, kind):
    """A duck-typed torch model (the oracle's network on the GPU, autograd over its own forward): the
    guided step against the oracle restatement, bound as in test_guided_step_vs_oracle."""
    import diff
    d = make_d(kind, cuda)
    hw = 8

    class Foreign(torch.nn.Module):  # not a dmx network: no .native(); returns (eps, geom), differentiable in x
        def forward(self, x, t, y, cond_vals=None, cond_mask=None):
            e, g = train_ref.forward(unet_sd, x.cpu(), t.cpu(), y.cpu(), cond_vals.cpu(), cond_mask.cpu())
            return e.to(x.device), g.to(x.device)

    class NoGeom(torch.nn.Module):
        def forward(self, x, t, y, cond_vals=None, cond_mask=None):
            return Foreign.forward(self, x, t, y, cond_vals, cond_mask)[0]

    x, t, y, vals, mask, hist, _, _, _, g_ref = step_ref(unet_sd, hw, kind)
    scale = torch.full((3,), S_STEP)
    tables, sched, sig = rule_tables(d, kind, cuda)
    d.noise_source = "host"
    torch.manual_seed(5)
    nz = torch.randn(x.shape)   # the draw the host-noise step makes
    torch.manual_seed(5)
    exp, exp_h = guided_step_ref(d, kind, unet_sd, hw, g_ref, scale, nz)
    plain, _ = guided_step_ref(d, kind, unet_sd, hw, None, scale, nz)
    share = float((exp - plain).norm() / exp.norm())
    assert share >= 0.05, share
    rule = {"ddpm": "ddpm", "ddim": "ddim", "dpm": "dpm"}[kind]
    plan = diff._SamplerPlan(rule, tables=tables, sched=sched, draws=kind != "dpm", scale=G,
                             geom=(scale.to(cuda), sig))
    p = (t if kind == "ddpm" else torch.tensor(STEP_POS)).to(cuda)
    h = hist.to(cuda)
    dv = [v.to(cuda) for v in (x, y, vals, mask)]
    out = d._step(Foreign(), dv[0], p, plan, True, dv[1], 0, dv[2], dv[3], hist=h if kind == "dpm" else None)
    err = rel(out, exp)
    print(f"[foreign model guided step {kind}] rel-L2 vs oracle = {err:.3e}, share = {share:.3f}")
    assert err <= TOL + GRAD_TOL * share, (err, share)
    with pytest.raises(ValueError, match="geom"):
        d._step(NoGeom(), dv[0], p, plan, True, dv[1], 0, dv[2], dv[3], hist=h if kind == "dpm" else None)


# ---- 11: it guides ------------------------------------------------------------------------------------------
GUIDE_SEED = 2


def guide_inputs(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    vals = torch.rand((4, 12), generator=g)
    mask = (torch.rand((4, 12), generator=g) > 0.3).float()
    return vals, mask


def final_loss(sd, x, y, vals, mask):
    """The masked loss of a final latent, by the oracle at t = 1, averaged over the rows."""
    with torch.no_grad():
        geom = train_ref.forward(sd, x, torch.ones(x.shape[0], dtype=torch.long), y, vals, mask)[1]
    return float(loss_rows(geom, vals, mask).mean())


def test_it_guides(model, cuda, unet_sd):
    """Host-noise DDIM, S = 8, CFG 3, B = 4 at 8x8: the final latent's masked loss (oracle, t = 1, mean
    over rows) is lower with geom_scale = 1000 than with 0.  Seed 2 was chosen on the CPU with an oracle
    restatement of the same loop (tools/geom_guide_bench.py --oracle-seeds 4): the oracle alone lowers
    the loss 0.28616 -> 0.26291, 8.1 % (seeds 0, 1, 3: 6.7 %, 5.6 %, 6.0 %)."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    d.noise_source = "host"
    vals, mask = guide_inputs(GUIDE_SEED)
    y = torch.tensor([1, 2, 3, 1])
    outs = []
    for s in (0.0, 1000.0):
        torch.manual_seed(GUIDE_SEED)
        outs.append(d.sample_latent_cond(model, [(1, 1), (2, 1), (3, 1), (1, 1)], z_shape=(4, 8, 8), vae=None,
                                         progress=False, guidance_scale=G, cond=vals.to(cuda), cond_mask=mask.to(cuda),
                                         sampler="ddim", steps=8, geom_scale=s).cpu())
    l0, l1 = (final_loss(unet_sd, o, y, vals, mask) for o in outs)
    print(f"[it guides] masked loss {l0:.5f} -> {l1:.5f} ({100 * (1 - l1 / l0):.1f} % lower)")
    assert torch.isfinite(outs[1]).all() and l1 < l0, (l0, l1)


# ---- errors from the C entries --------------------------------------------------------------------------------
def test_c_entries_reject_bad_geometry_guidance(model, cuda):
    """Argument checks on the host: every case returns DMX_E_ARG with a message and launches nothing."""
    import diff
    from dmx import _lib, synth
    from models.unet_cond import UnetCond
    d = diff.Diffuser(1000, device=cuda)
    nm = model.native()
    lib = nm.lib
    B = 2
    x = torch.zeros((B, 4, 8, 8), device=cuda)
    out = torch.empty_like(x)
    t = torch.full((B,), 5, dtype=torch.long, device=cuda)
    y = torch.ones((B,), dtype=torch.long, device=cuda)
    vals, mask = torch.rand((B, 12), device=cuda), torch.ones((B, 12), device=cuda)
    tables = d.coef_tables(cuda, True)
    sig, scale = d.geom_sig(cuda), torch.ones((B,), device=cuda)
    nm.ctx.ensure_time_table(1000)

    def call(handle, guidance=G, yy=y, vv=vals, mm=mask, sc=scale, sg=sig, S=1000, loop=False, comp=None):
        a = nm._args(x, out, t, 1, yy, 0, vv, mm, guidance, tables, x, 0, 0)
        gg = _lib.GeomGuide(sc.data_ptr() if sc is not None else None, sg.data_ptr() if sg is not None else None, S)
        with torch.cuda.device(cuda):
            if loop:
                rc = lib.dmx_sample_loop_geom(handle, ctypes.byref(a), None, None, None, ctypes.byref(gg), 1, 0, None)
            else:
                rc = lib.dmx_step_geom(handle, ctypes.byref(a), None, None, None, ctypes.byref(gg), None)
        return rc, (lib.dmx_last_error() or b"").decode()

    um = UnetCond()
    um.load_state_dict({k: v for k, v in synth.unet_cond_geom_weights(0).items() if not k.startswith("geom_head.")})
    plain = um.to(cuda).eval().native()
    bad = dict(no_guidance=dict(guidance=0.0), no_y=dict(yy=None), no_vals=dict(vv=None, mm=None),
               null_scale=dict(sc=None), null_sig=dict(sg=None), wrong_S=dict(S=999), alias=dict(sc=out))
    for loop in (False, True):
        for name, kw in bad.items():
            rc, msg = call(nm.handle, loop=loop, **kw)
            assert rc == _lib.DMX_E_ARG and msg, (name, loop, rc, msg)
        rc, msg = call(plain.handle, loop=loop)
        assert rc == _lib.DMX_E_ARG and "GeomHead" in msg, (loop, rc, msg)
    torch.cuda.synchronize()
    for kw in (dict(rescale=0.5), dict(compose=(y[None].repeat(2, 1), None, None, scale[None]))):
        with pytest.raises(ValueError):
            nm.step(x, out, t, y, 0, vals, mask, G, tables, x, geom=(scale, sig), **kw)
    with pytest.raises(ValueError):
        nm.step(x, out, t, y, 0, vals, mask, G, tables, x, geom=(scale[:1], sig))
    with pytest.raises(ValueError):
        plain.step(x, out, t, y, 0, vals, mask, G, tables, x, geom=(scale, sig))
    with pytest.raises(ValueError):
        d.sample_latent_cond(um, {1: 2}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals, cond_mask=mask,
                             geom_scale=1.0)


# ---- 12: workspace diagnostics ----------------------------------------------------------------------------------
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
for in_ch in (4, 3):
    m = UnetCondWithGeomHead(in_ch=in_ch)
    m.load_state_dict(synth.unet_cond_geom_weights(0, in_ch=in_ch))
    m.to(dev).eval()
    d = diff.Diffuser(4, device=dev)
    tables = d.coef_tables(dev, clamp_prev=True)
    nm = m.native()
    y = torch.tensor([1, 0, 3], device=dev)
    vals = torch.rand((B, 12), generator=g).to(dev)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float().to(dev)
    mask[-1] = 0
    scale = torch.tensor([2000.0, 1000.0, 500.0], device=dev)
    for hw in (16, 28):
        x = torch.randn((B, in_ch, hw, hw), generator=g).to(dev)
        noise = torch.randn((B, in_ch, hw, hw), generator=g).to(dev)
        tt = torch.full((B,), 4, dtype=torch.long, device=dev)
        o = torch.empty_like(x)
        nm.step(x, o, tt, y, 0, vals, mask, 3.0, tables, noise, geom=(scale, d.geom_sig(dev)))
        out[f"step_c{in_ch}_{hw}"] = o.cpu()
        loss, grad, geom, eps = nm.geom_grad(x, tt, y, vals, mask)
        out[f"grad_c{in_ch}_{hw}"] = grad.cpu()
torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print("[geom-worker] ok", flush=True)
'''


def test_guided_step_reads_no_unwritten_workspace(cuda, tmp_path):
    """One guided step and one geom_grad (in_ch = 4 and 3; 16x16 and 28x28) in fresh processes, with and
    without DMX_POISON=1 / DMX_CHECK=1: finite and bit-identical."""
    clean = run_worker(tmp_path, "clean", WORKER)
    diag = run_worker(tmp_path, "diag", WORKER, DMX_POISON="1", DMX_CHECK="1")
    bad = [k for k in clean if not torch.isfinite(diag[k]).all() or not torch.equal(clean[k], diag[k])]
    assert bad == [], bad
