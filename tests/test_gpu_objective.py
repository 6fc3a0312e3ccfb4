"""The native training objective (include/dmx.h dmx_train_noise / dmx_objective_loss / dmx_objective_seed,
Diffuser.training_loss) on the GPU.

Bounds, from the arithmetic and not from what the kernels give:
- z_noisy given t and noise: torch's bits (two products and a sum, one rounding each, on the same device).
- the losses against float64 on the CPU from the same fp32 inputs, 1e-6 relative: the fp32 difference and
  square err by at most 2^-23 relative on each (positive) term, so on their sum; the double accumulation
  adds ~1e-16 per term; one final rounding to fp32 (6e-8).
- the seeds, 1e-6 relative per element: the coefficient, the difference and the product round once each
  (3 x 6e-8; the geometry seed also reads the fp32 denominator).
- gradients end to end: the project's bound for the native backward, 1e-4 per-tensor relative L2
  against the CPU oracle (tests/test_gpu_train.py).
- draws: 5 sigma of the binomial share (B = 4096, p = 0.5: 5 * 0.5 / 64 = 0.039) and of the sample mean
  and variance of N normals (5 / sqrt(N), 5 * sqrt(2 / N))."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

T = 1000
SHAPES = [(3, 4, 8, 8), (1, 4, 28, 28), (5, 3, 9, 7)]  # the last: C*h*w = 189, no multiple of 4 or of 256


def _diffuser(dev):
    import diff
    return diff.Diffuser(T, device=dev)


def _front_inputs(shape, seed=0, gd=12):
    B = shape[0]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g)
    noise = torch.randn(shape, generator=g)
    t = torch.randint(1, T + 1, (B,), generator=g)
    t[0], t[-1] = 1, T
    y = torch.randint(1, 4, (B,), generator=g)
    vals = torch.rand((B, gd), generator=g) - 0.25
    mask = (torch.rand((B, gd), generator=g) > 0.3).float()
    drop = torch.zeros(B, dtype=torch.bool)
    drop[B // 2] = True
    return z, noise, t, y, vals, mask, drop


# ---- front kernel, t and noise given -------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_noise_given_is_torch_bit_for_bit(cuda, shape):
    from dmx import engine
    d = _diffuser(cuda)
    sa, s1 = d.noise_tables(cuda)
    z, noise, t, y, vals, mask, drop = (v.to(cuda) for v in _front_inputs(shape))
    B = shape[0]
    for tt in ([t] if B > 1 else [torch.full_like(t, 1), torch.full_like(t, T)]):
        zn, nz, t_o, d_o, y_u, v_u, m_u = engine.train_noise(z, sa, s1, tt, noise, drop, y, 7, vals, mask)
        ab = d.alpha_bars[tt - 1].view(-1, 1, 1, 1)
        assert ab.is_cuda
        ref = torch.sqrt(ab) * z + torch.sqrt(1 - ab) * noise
        assert torch.equal(zn, ref)
        assert torch.equal(nz, noise) and torch.equal(t_o, tt) and torch.equal(d_o, drop)
        k = B // 2
        assert int(y_u[k]) == 7 and float(v_u[k].abs().sum()) == 0.0 and float(m_u[k].abs().sum()) == 0.0
        keep = ~drop
        assert torch.equal(y_u[keep], y[keep])
        assert torch.equal(v_u[keep].view(torch.int32), vals[keep].view(torch.int32))
        assert torch.equal(m_u[keep].view(torch.int32), mask[keep].view(torch.int32))
    # nothing dropped when no drop is given and the probability is 0; no condition, no label: outputs None
    zn, _, _, d_o, y_u, v_u, m_u = engine.train_noise(z, sa, s1, t, noise)
    assert torch.equal(zn, torch.sqrt(d.alpha_bars[t - 1].view(-1, 1, 1, 1)) * z
                       + torch.sqrt(1 - d.alpha_bars[t - 1].view(-1, 1, 1, 1)) * noise)
    assert not bool(d_o.any()) and y_u is None and v_u is None and m_u is None


def test_noise_refusals(cuda):
    from dmx import _lib, engine
    d = _diffuser(cuda)
    sa, s1 = d.noise_tables(cuda)
    z = torch.zeros((2, 4, 8, 8), device=cuda)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            engine.train_noise(z, sa, s1, cfg_drop_prob=bad)
    with pytest.raises(ValueError):
        engine.train_noise(z, sa, s1[:10])
    with pytest.raises(ValueError):
        engine.train_noise(z, sa, s1, t=torch.ones(3, dtype=torch.long))
    with pytest.raises(ValueError):
        engine.train_noise(z, sa, s1, vals=torch.zeros((2, 12)))
    lib = _lib.load()
    assert lib.dmx_train_noise(None, None) == _lib.DMX_E_ARG
    a = _lib.NoiseArgs(B=0, C=4, h=8, w=8, T=1000)
    assert lib.dmx_train_noise(a, None) == _lib.DMX_E_ARG  # null z
    assert lib.dmx_objective_loss(None, None) == _lib.DMX_E_ARG
    assert lib.dmx_objective_seed(None, None, None, None, None) == _lib.DMX_E_ARG


# ---- draws ------------------------------------------------------------------------------------------------
def test_draws_are_seeded_and_in_range(cuda):
    from dmx import engine
    d = _diffuser(cuda)
    sa, s1 = d.noise_tables(cuda)
    z = torch.randn((6, 4, 8, 8), generator=torch.Generator().manual_seed(1)).to(cuda)
    torch.manual_seed(123)
    s_a = d._seed()
    torch.manual_seed(123)
    s_b = d._seed()
    torch.manual_seed(124)
    s_c = d._seed()
    assert s_a == s_b != s_c
    a = engine.train_noise(z, sa, s1, cfg_drop_prob=0.5, seed=s_a)
    b = engine.train_noise(z, sa, s1, cfg_drop_prob=0.5, seed=s_b)
    c = engine.train_noise(z, sa, s1, cfg_drop_prob=0.5, seed=s_c)
    for i in range(4):  # z_noisy, noise, t, drop
        assert torch.equal(a[i], b[i])
    assert not torch.equal(a[1], c[1]) and not torch.equal(a[2], c[2])
    for r in (a, c):
        assert int(r[2].min()) >= 1 and int(r[2].max()) <= T and r[2].dtype == torch.long
        assert r[3].dtype == torch.bool and bool(torch.isfinite(r[1]).all())
        ab = d.alpha_bars[r[2] - 1].view(-1, 1, 1, 1)
        assert torch.equal(r[0], torch.sqrt(ab) * z + torch.sqrt(1 - ab) * r[1])  # the drawn values are the used ones
    assert not bool(engine.train_noise(z, sa, s1, cfg_drop_prob=0.0, seed=s_a)[3].any())
    assert bool(engine.train_noise(z, sa, s1, cfg_drop_prob=1.0, seed=s_a)[3].all())
    # T = 12: a short table, every draw inside it
    d12 = __import__("diff").Diffuser(12, device=cuda)
    r = engine.train_noise(z.repeat(50, 1, 1, 1), *d12.noise_tables(cuda), seed=9)
    assert int(r[2].min()) == 1 and int(r[2].max()) == 12
    # a mixed call: t given, the rest drawn under the same seed as before
    m = engine.train_noise(z, sa, s1, t=a[2], cfg_drop_prob=0.5, seed=s_a)
    assert torch.equal(m[0], a[0]) and torch.equal(m[1], a[1]) and torch.equal(m[3], a[3])


def test_draw_statistics(cuda):
    from dmx import engine
    d = _diffuser(cuda)
    sa, s1 = d.noise_tables(cuda)
    B = 4096
    z = torch.zeros((B, 4, 8, 8), device=cuda)
    _, noise, t, drop, _, _, _ = engine.train_noise(z, sa, s1, cfg_drop_prob=0.5, seed=2024)
    share = float(drop.float().mean())
    n = noise.numel()
    mean, var = float(noise.double().mean()), float(noise.double().var())
    print(f"[draws] dropped share {share:.4f}, noise mean {mean:.2e}, var - 1 {var - 1:.2e}, "
          f"t in [{int(t.min())}, {int(t.max())}], mean t {float(t.double().mean()):.1f}")
    assert abs(share - 0.5) <= 0.039
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert int(t.min()) >= 1 and int(t.max()) <= T
    # uniform t: the mean of B draws from U{1..T} has sigma sqrt((T^2 - 1) / 12 / B)
    assert abs(float(t.double().mean()) - (T + 1) / 2) <= 5 * math.sqrt((T * T - 1) / 12 / B)


@pytest.mark.parametrize("chw", [(4, 8, 8), (3, 9, 7)])
def test_draws_do_not_depend_on_the_sharding(cuda, chw):
    from dmx import engine
    d = _diffuser(cuda)
    sa, s1 = d.noise_tables(cuda)
    B, k = 6, 2
    z = torch.randn((B, *chw), generator=torch.Generator().manual_seed(4)).to(cuda)
    whole = engine.train_noise(z, sa, s1, cfg_drop_prob=0.5, seed=77)
    shard = engine.train_noise(z[k:], sa, s1, cfg_drop_prob=0.5, seed=77, sample_offset=k)
    for i in range(4):
        assert torch.equal(whole[i][k:], shard[i]), i
    other = engine.train_noise(z[k:], sa, s1, cfg_drop_prob=0.5, seed=77, sample_offset=0)
    assert not torch.equal(whole[1][k:], other[1])


# ---- loss and seed kernels ------------------------------------------------------------------------------
def _loss_inputs(shape, seed=5, gd=12):
    B = shape[0]
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(shape, generator=g)
    noise = torch.randn(shape, generator=g)
    t = torch.randint(1, T + 1, (B,), generator=g)
    t[0] = 3  # min-SNR weight < 1 there
    geom = torch.randn((B, gd), generator=g)
    vals = torch.rand((B, gd), generator=g)
    mask = (torch.rand((B, gd), generator=g) > 0.3).float()
    mask[0, 0] = 1.0
    return eps, noise, t, geom, vals, mask


def _loss_ref(eps, noise, t, w, geom, vals, mask, lam, denom=None):
    e, n = eps.double(), noise.double()
    per = w.double()[t - 1] * ((e - n) ** 2).flatten(1).mean(dim=1)
    num = (mask.double() * (geom.double() - vals.double()) ** 2).sum()
    dn = max(float(mask.double().sum()) if denom is None else float(denom), 1e-6)
    gl = num / dn
    return per.mean() + lam * gl, per.mean(), gl, per, dn


def _close(a, b, rel=1e-6):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return bool((torch.abs(a - b) <= rel * torch.abs(b)).all())


@pytest.mark.parametrize("weighting", ["uniform", "min_snr"])
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_seed_vs_float64(cuda, shape, weighting):
    from dmx import engine
    d = _diffuser(cuda)
    eps, noise, t, geom, vals, mask = _loss_inputs(shape)
    w = d.loss_weights(weighting, device="cpu")
    if weighting == "min_snr":
        assert float(w[t - 1].min()) < 1.0
    lam = 0.5
    dv = [v.to(cuda) for v in (eps, noise, t, geom, vals, mask)]
    wd = None if weighting == "uniform" else w.to(cuda)
    for denom in (None, 3.5):
        obj = engine.objective_loss(dv[0], dv[1], dv[2], wd, dv[3], dv[4], dv[5], lam, denom)
        loss, nl, gl, per, dn = _loss_ref(eps, noise, t, w, geom, vals, mask, lam, denom)
        print(f"[objective {shape} {weighting} denom={denom}] loss {float(obj.loss):.9g} vs {float(loss):.9g}")
        assert _close(obj.loss, loss) and _close(obj.noise_loss, nl) and _close(obj.geom_loss, gl)
        assert _close(obj.per_sample, per)
        again = engine.objective_loss(dv[0], dv[1], dv[2], wd, dv[3], dv[4], dv[5], lam, denom)
        assert torch.equal(again._out, obj._out) and torch.equal(again.per_sample, obj.per_sample)
        # the seed: d loss / d eps and d loss / d geom, scaled by the upstream scalar on the device
        B, chw = shape[0], eps[0].numel()
        ref_e = (2.0 * w.double()[t - 1] / (B * chw)).view(-1, 1, 1, 1) * (eps.double() - noise.double())
        ref_g = lam * 2.0 * mask.double() * (geom.double() - vals.double()) / dn
        d_eps, d_geom = engine.objective_seed(obj)
        assert _close(d_eps, ref_e) and _close(d_geom, ref_g)
        q_eps, q_geom = engine.objective_seed(obj, torch.tensor(0.25, device=cuda))
        assert torch.equal(q_eps, 0.25 * d_eps) and torch.equal(q_geom, 0.25 * d_geom)
        only_eps, none = engine.objective_seed(obj, want_geom=False)
        assert none is None and torch.equal(only_eps, d_eps)
    # no geometry term
    obj = engine.objective_loss(dv[0], dv[1], dv[2], wd)
    assert float(obj.geom_loss) == 0.0 and float(obj.loss) == float(obj.noise_loss)
    assert engine.objective_seed(obj)[1] is None


def test_all_zero_mask(cuda):
    from dmx import engine
    eps, noise, t, geom, vals, mask = (v.to(cuda) for v in _loss_inputs(SHAPES[0]))
    obj = engine.objective_loss(eps, noise, None, None, geom, vals, torch.zeros_like(mask), 0.5)
    assert float(obj.geom_loss) == 0.0 and float(obj.loss) == float(obj.noise_loss)
    assert math.isfinite(float(obj.loss))
    d_eps, d_geom = engine.objective_seed(obj)
    assert float(d_geom.abs().sum()) == 0.0 and bool(torch.isfinite(d_eps).all())


# ---- end to end ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(unet_sd)
    return m.to(cuda).train()


def _e2e_inputs(B, hw, seed=31):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, 4, hw, hw), generator=g)
    noise = torch.randn((B, 4, hw, hw), generator=g)
    classes = torch.randint(1, 4, (B,), generator=g)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    t = torch.tensor([1000, 40, 1][:B])  # min-SNR weights < 1 at the small ones
    drop = torch.zeros(B, dtype=torch.bool)
    drop[B - 1] = True
    return z, noise, classes, vals, mask, t, drop


def _loop_inputs(d, z, noise, classes, vals, mask, t, drop):
    """What the loop feeds the network (train_latent_cond.py:137-145), on the CPU."""
    ab = d._host[1][t - 1].view(-1, 1, 1, 1)
    z_noisy = torch.sqrt(ab) * z + torch.sqrt(1 - ab) * noise
    keep = (~drop).float().unsqueeze(1)
    return z_noisy, torch.where(drop, torch.zeros_like(classes), classes), vals * keep, mask * keep


def _rel_l2(a, b):
    return float((a.detach().double().cpu() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def _native_grads(d, model, inputs, cuda, lam, weighting, halves=1):
    z, noise, classes, vals, mask, t, drop = (v.to(cuda) for v in inputs)
    model.zero_grad(set_to_none=True)
    for _ in range(halves):
        res = d.training_loss(model, z, classes, vals, mask, geom_lambda=lam, weighting=weighting, t=t, noise=noise,
                              drop=drop)
        (res.loss / halves).backward()
    return res, {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()}


@pytest.mark.parametrize("B,hw,weighting", [(3, 8, "uniform"), (3, 8, "min_snr"), (2, 28, "uniform")])
def test_training_loss_gradients_vs_oracle(cuda, model, unet_sd, B, hw, weighting):
    from losses.geom_losses import masked_geom_mse
    from oracle import train_ref
    d = _diffuser(cuda)
    lam = 0.5
    inputs = _e2e_inputs(B, hw)
    z, noise, classes, vals, mask, t, drop = inputs
    res, grads = _native_grads(d, model, inputs, cuda, lam, weighting)
    assert res.loss.requires_grad and res.loss.dim() == 0 and not res.noise_loss.requires_grad
    assert torch.equal(res.t.cpu(), t) and torch.equal(res.drop.cpu(), drop)
    z_noisy, y_used, vals_used, mask_used = _loop_inputs(d, z, noise, classes, vals, mask, t, drop)
    if weighting == "uniform":
        rloss, _, _, ref = train_ref.loss_and_grads(unet_sd, z_noisy, t, y_used, vals_used, mask_used, noise, vals,
                                                    mask_used, lam, True, False)
    else:
        w = d.loss_weights("min_snr", device="cpu")
        assert float(w[t - 1].min()) < 1.0
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in unet_sd.items()}
        eps, g = train_ref.forward(leaves, z_noisy, t, y_used, vals_used, mask_used)
        rloss = (w[t - 1] * ((eps - noise) ** 2).mean(dim=(1, 2, 3))).mean() \
            + lam * train_ref.masked_geom_mse(g, vals, mask_used)
        rloss.backward()
        ref = {k: v.grad for k, v in leaves.items()}
        rloss = rloss.detach()
    assert abs(float(res.loss.detach()) - float(rloss)) <= 2e-5 * float(rloss)
    worst = []
    for n in grads:
        assert (grads[n] is None) == (ref[n] is None), n
        if ref[n] is not None:
            worst.append((_rel_l2(grads[n], ref[n]), n))
    worst.sort(reverse=True)
    print(f"[objective e2e B={B} {hw}x{hw} {weighting}] worst rel-L2 vs oracle:", worst[:3])
    assert worst[0][0] <= 1e-4, worst[:5]
    if hw == 8 and weighting == "uniform":
        # gradient accumulation: two halves make the whole
        _, acc = _native_grads(d, model, inputs, cuda, lam, weighting, halves=2)
        for n in grads:
            assert _rel_l2(acc[n], grads[n].cpu()) <= 1e-6, n
        # the existing torch-op path on the same model and inputs
        dv = [v.to(cuda) for v in (z_noisy, t, y_used, vals_used, mask_used, noise, vals)]
        eps, gp = model(dv[0], dv[1], dv[2], cond_vals=dv[3], cond_mask=dv[4])
        loop = F.mse_loss(eps, dv[5]) + lam * masked_geom_mse(gp, dv[6], dv[4])
        assert abs(float(loop.detach()) - float(res.loss.detach())) <= 1e-5 * float(loop.detach())


def test_unused_branches_get_none(cuda, model):
    d = _diffuser(cuda)
    z, noise, classes, vals, mask, t, drop = (v.to(cuda) for v in _e2e_inputs(3, 8))
    model.zero_grad(set_to_none=True)
    d.training_loss(model, z, classes, t=t, noise=noise, drop=drop).loss.backward()
    for n, p in model.named_parameters():
        assert (p.grad is None) == n.startswith(("cond_mlp.", "geom_head.")), n
    model.zero_grad(set_to_none=True)
    d.training_loss(model, z, classes, vals, mask, t=t, noise=noise, drop=drop).loss.backward()  # geom_lambda = 0
    for n, p in model.named_parameters():
        assert (p.grad is None) == n.startswith("geom_head."), n
    model.zero_grad(set_to_none=True)


def test_no_grad_keeps_a_pending_tape(cuda, model):
    d = _diffuser(cuda)
    inputs = _e2e_inputs(3, 8)
    z, noise, classes, vals, mask, t, drop = (v.to(cuda) for v in inputs)
    kw = dict(geom_lambda=0.5, t=t, noise=noise, drop=drop)
    _, want = _native_grads(d, model, inputs, cuda, 0.5, "uniform")
    model.zero_grad(set_to_none=True)
    pending = d.training_loss(model, z, classes, vals, mask, **kw)
    with torch.no_grad():
        val = d.training_loss(model, z, classes, vals, mask, **kw)
    assert val.loss.grad_fn is None and not val.loss.requires_grad
    model.eval()
    try:
        ev = d.training_loss(model, z, classes, vals, mask, **kw)
    finally:
        model.train()
    assert ev.loss.grad_fn is None and float(ev.loss) == float(val.loss)
    # the ordinary forward computes in the default precision mode, the taped one in exact fp32: the
    # project's forward bound (1e-4 relative, as in smoke) is what ties the two losses
    assert abs(float(val.loss) - float(pending.loss.detach())) <= 1e-4 * float(val.loss)
    assert _close(val.per_sample, pending.per_sample.cpu(), rel=1e-4)
    pending.loss.backward()
    for n, p in model.named_parameters():
        assert _rel_l2(p.grad, want[n].cpu()) <= 1e-6, n
    model.zero_grad(set_to_none=True)


def test_drawn_iteration_is_seeded(cuda, model):
    d = _diffuser(cuda)
    z, _, classes, vals, mask, _, _ = (v.to(cuda) for v in _e2e_inputs(3, 8))
    out = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        r = d.training_loss(model, z, classes, vals, mask, geom_lambda=0.5, cfg_drop_prob=0.5, weighting="min_snr")
        out.append((r.t.cpu(), r.drop.cpu(), float(r.loss.detach()), r.per_sample.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert torch.equal(out[0][3], out[1][3])
    assert not torch.equal(out[0][0], out[2][0]) and out[0][2] != out[2][2]
    assert int(out[0][0].min()) >= 1 and int(out[0][0].max()) <= T and math.isfinite(out[0][2])


def test_optimizer_step_is_seen_by_the_next_call(cuda, unet_sd):
    import dmx.optim as O
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(unet_sd)
    m.to(cuda).train()
    d = _diffuser(cuda)
    z, noise, classes, vals, mask, t, drop = (v.to(cuda) for v in _e2e_inputs(3, 8))
    kw = dict(geom_lambda=0.5, t=t, noise=noise, drop=drop)
    opt = O.Adam(m.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in m.parameters()]
    first = d.training_loss(m, z, classes, vals, mask, **kw)
    opt.zero_grad(set_to_none=True)
    first.loss.backward()
    opt.step()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    second = d.training_loss(m, z, classes, vals, mask, **kw)
    l1, l2 = float(first.loss.detach()), float(second.loss.detach())
    print(f"[objective] loss {l1:.6f} -> {l2:.6f} after one Adam step")
    assert math.isfinite(l2) and l2 != l1
