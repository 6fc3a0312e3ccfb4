"""The native VAE training step (include/dmx.h dmx_vae_train_forward / dmx_vae_train_backward) driven
the way train_vae.py drives the reference: drop-in VAE in train mode, `x_recon, z, loss, parts =
vae(x)`, loss.backward(), torch Adam.  The gradient reference is torch autograd over
oracle.ref.vae_forward (pinned to the reference by tests/test_vae_train_oracle.py).
Tolerances: forward outputs at the project's forward bound (TOL of test_gpu_parity.py); every
gradient tensor within 1e-4 rel-L2 of the oracle's (the bound test_gpu_train.py uses for the same
arithmetic, ~35x the fp32 oracle's own 2.8e-6 distance from the fp64 oracle); the reference's recorded
statistics within 2e-4 of each tensor's L2 norm."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_parity import TOL  # noqa: E402
from test_vae_train_oracle import GOLD, oracle_step, params_after_close, vae_grad_stats_close  # noqa: E402
from oracle import ref  # noqa: E402
from oracle.rules import rel  # noqa: E402

GRAD_TOL = 1e-4


@pytest.fixture(scope="module")
def sd0():
    from dmx import synth
    return synth.vae_weights(0)


def _vae(sd, dev):
    from models.vae import VAE
    v = VAE()
    v.load_state_dict(sd)
    return v.to(dev).train()


def _x(shape, seed=7):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _worst(grads, refg, what):
    worst = []
    for n, b in refg.items():
        a = grads[n].detach().double().cpu()
        worst.append((float((a - b.double()).norm() / max(float(b.double().norm()), 1e-30)), n))
    worst.sort(reverse=True)
    print(f"[vae train {what}] worst rel-L2 vs oracle:", worst[:5])
    return worst


def _dropin_step(v, x, seed):
    torch.manual_seed(seed)
    x_recon, z, loss, parts = v(x)
    v.zero_grad(set_to_none=True)
    loss.backward()
    torch.manual_seed(seed)
    eps = torch.randn(z.shape, device=x.device)  # the draw forward made, replayed
    return x_recon, z, loss, parts, eps


@pytest.mark.parametrize("shape", [(3, 24, 16), (2, 64, 64)])
def test_dropin_step_matches_oracle(cuda, sd0, shape):
    """(3, 24, 16): non-square, odd batch, 2 x 3 latents, every stride-2 border tap; (2, 64, 64):
    multi-chunk GroupNorm reductions, several wgrad row splits."""
    n, h, w = shape
    v = _vae(sd0, cuda)
    x = _x((n, 3, h, w))
    x_recon, z, loss, parts, eps = _dropin_step(v, x.to(cuda), 11)
    exp_recon, exp_z, exp_loss, refg = oracle_step(sd0, x, eps.cpu())
    assert rel(x_recon.detach(), exp_recon) < TOL and rel(z.detach(), exp_z) < TOL
    assert abs(float(loss.detach()) - float(exp_loss)) <= TOL * abs(float(exp_loss))
    assert not parts["kl"].requires_grad and not parts["recon_mse"].requires_grad
    grads = {k: p.grad for k, p in v.named_parameters()}
    assert all(g is not None for g in grads.values())
    worst = _worst(grads, refg, shape)
    assert worst[0][0] <= GRAD_TOL, worst[:5]


def test_dropin_step_matches_reference_fixture(cuda, sd0):
    """The reference's own step (tests/golden/vae_train_step.npz): loss, x_recon and the recorded
    gradient statistics, with the drop-in's device draw replaced by the reference's CPU draw."""
    from models._native import _NativeVaeTrainFn
    v = _vae(sd0, cuda)
    x, eps = torch.from_numpy(GOLD["x"]).to(cuda), torch.from_numpy(GOLD["eps"]).to(cuda)
    names = [k for k, _ in v.named_parameters()]
    assert names == list(GOLD["names"])
    x_recon, z, kl = _NativeVaeTrainFn.apply(v, names, x, eps, *v.parameters())
    loss = F.mse_loss(x_recon, x) + 1e-6 * kl.mean()
    loss.backward()
    assert abs(float(loss.detach()) - float(GOLD["loss"])) <= TOL * float(GOLD["loss"])
    assert abs(float(kl.detach().mean()) - float(GOLD["kl"])) <= TOL * float(GOLD["kl"])
    assert rel(x_recon.detach(), GOLD["x_recon"]) < TOL and rel(z.detach(), GOLD["z"]) < TOL
    assert vae_grad_stats_close({k: p.grad for k, p in v.named_parameters()}, names) == []


def _three_cotangent_grads(v, sd, x, eps, dev):
    from models._native import _NativeVaeTrainFn
    names = [k for k, _ in v.named_parameters()]
    xd = x.to(dev)
    x_recon, z, kl = _NativeVaeTrainFn.apply(v, names, xd, eps.to(dev), *v.parameters())
    assert kl.shape == (x.size(0),)
    loss = F.mse_loss(x_recon, xd) + 0.3 * z.square().mean() + 0.5 * kl.mean()
    v.zero_grad(set_to_none=True)
    loss.backward()
    _, _, exp_loss, refg = oracle_step(
        sd, x, eps, lambda xr, zz, k: F.mse_loss(xr, x) + 0.3 * zz.square().mean() + 0.5 * k)
    assert abs(float(loss.detach()) - float(exp_loss)) <= TOL * abs(float(exp_loss))
    return {k: p.grad for k, p in v.named_parameters()}, refg


def test_all_three_cotangents(cuda, sd0):
    """The 1e-6 KL weight of VAE.forward's loss hides the d_kl and d_z paths: a loss with O(1)
    weights on z and the per-sample KL."""
    x = _x((2, 3, 32, 32))
    eps = torch.randn((2, 4, 4, 4), generator=torch.Generator().manual_seed(3))
    grads, refg = _three_cotangent_grads(_vae(sd0, cuda), sd0, x, eps, cuda)
    worst = _worst(grads, refg, "3 cotangents")
    assert worst[0][0] <= GRAD_TOL, worst[:5]


def test_clamp_gradient(cuda, sd0):
    """to_logvar.bias = -35 on two channels: the lower clamp is active there, so those rows of
    to_logvar.weight / .bias take exactly the oracle's gradient — zero from the clamped path."""
    sd = {k: v.clone() for k, v in sd0.items()}
    sd["to_logvar.bias"][[1, 3]] = -35.0
    x = _x((2, 3, 32, 32))
    eps = torch.randn((2, 4, 4, 4), generator=torch.Generator().manual_seed(3))
    grads, refg = _three_cotangent_grads(_vae(sd, cuda), sd, x, eps, cuda)
    for k in ("to_logvar.weight", "to_logvar.bias"):
        assert float(refg[k][[1, 3]].abs().max()) == 0.0  # the clamp is active in the oracle
        assert float(grads[k][[1, 3]].abs().max()) == 0.0, k
        assert float(refg[k][[0, 2]].abs().max()) > 0.0
    worst = _worst(grads, refg, "clamp")
    assert worst[0][0] <= GRAD_TOL, worst[:5]


def test_step_is_deterministic(cuda, sd0):
    x = _x((2, 3, 64, 64)).to(cuda)
    runs = []
    for _ in range(2):
        v = _vae(sd0, cuda)
        x_recon, z, loss, _, _ = _dropin_step(v, x, 5)
        runs.append((x_recon.detach().clone(), {k: p.grad.detach().clone() for k, p in v.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_two_adam_steps_and_refresh(cuda, sd0):
    """Two torch Adam(lr=1e-3) steps on the drop-in vs the same two steps on the CPU with the oracle
    forward (and vs the reference's recorded parameters); after step 1 the refreshed model's forward
    and backward equal, bit for bit, those of a model built from scratch from the updated weights."""
    from models._native import _NativeVaeTrainFn
    lr = float(GOLD["lr"])
    x = torch.from_numpy(GOLD["x"])
    v = _vae(sd0, cuda)
    names = [k for k, _ in v.named_parameters()]
    opt = torch.optim.Adam(v.parameters(), lr=lr)
    cpu = {k: t.clone().requires_grad_(True) for k, t in sd0.items()}
    copt = torch.optim.Adam(cpu.values(), lr=lr)
    xd = x.to(cuda)
    for step, key in enumerate(("eps", "eps2")):
        eps = torch.from_numpy(GOLD[key])
        x_recon, z, kl = _NativeVaeTrainFn.apply(v, names, xd, eps.to(cuda), *v.parameters())
        loss = F.mse_loss(x_recon, xd) + 1e-6 * kl.mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 1:  # the step-2 forward / backward ran on refreshed weights: a fresh model agrees exactly
            assert v.native() is nm0
            fresh = _vae({k: p.detach().cpu() for k, p in v.named_parameters()}, cuda)
            fr, fz, fk = _NativeVaeTrainFn.apply(fresh, names, xd, eps.to(cuda), *fresh.parameters())
            (F.mse_loss(fr, xd) + 1e-6 * fk.mean()).backward()
            assert torch.equal(fr, x_recon) and torch.equal(fz, z) and torch.equal(fk, kl)
            for (k, p), q in zip(v.named_parameters(), fresh.parameters()):
                assert torch.equal(p.grad, q.grad), k
        opt.step()
        nm0 = v.native() if step == 0 else nm0
        copt.zero_grad(set_to_none=True)
        ref.vae_forward(cpu, x, eps)[2].backward()
        copt.step()
    got = dict(v.named_parameters())
    ok, info = params_after_close(got, names)
    assert ok, info
    d = np.concatenate([(got[k].detach().cpu() - cpu[k].detach()).abs().reshape(-1).numpy() for k in names])
    a = np.concatenate([cpu[k].detach().abs().reshape(-1).numpy() for k in names])
    print("[vae train adam] max |dp| vs oracle:", float(d.max()), "bulk:", float((d <= 1e-6 + 1e-5 * a).mean()))
    assert d.max() <= 2.1 * lr and (d <= 1e-6 + 1e-5 * a).mean() >= 0.97


def test_inference_forward_after_refresh_equals_fresh_model(cuda, sd0):
    """After optimizer.step() a no_grad forward through the refreshed model equals, bit for bit, a
    forward through a freshly constructed model loaded from the updated state dict."""
    v = _vae(sd0, cuda)
    x = _x((2, 3, 32, 32)).to(cuda)
    opt = torch.optim.Adam(v.parameters(), lr=1e-3)
    _dropin_step(v, x, 2)
    nm0 = v.native()
    opt.step()
    outs = []
    fresh = _vae({k: p.detach().cpu() for k, p in v.named_parameters()}, cuda)
    for mod in (v, fresh):
        torch.manual_seed(4)
        with torch.no_grad():
            outs.append(mod(x))
    assert v.native() is nm0  # refreshed, not rebuilt
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], outs[1][2])


def test_rng_input_grad_and_no_grad_path(cuda, sd0):
    v = _vae(sd0, cuda)
    x = _x((2, 3, 32, 32), seed=5).to(cuda)
    # training-mode forward advances the device RNG by exactly one randn of z's shape
    torch.manual_seed(9)
    x_recon, z, loss, parts = v(x)
    assert loss.grad_fn is not None and x_recon.grad_fn is not None
    after = torch.randn(3, device=cuda)
    torch.manual_seed(9)
    _ = torch.randn((2, 4, 4, 4), device=cuda)
    assert torch.equal(after, torch.randn(3, device=cuda))
    # gradients for x are refused
    with pytest.raises(NotImplementedError):
        v(x.clone().requires_grad_(True))
    # no_grad: today's inference path, bit for bit (encode -> decode on the inference kernels)
    torch.manual_seed(9)
    with torch.no_grad():
        r0, z0, l0, p0 = v(x)
    assert r0.grad_fn is None and z0.grad_fn is None and l0.grad_fn is None
    torch.manual_seed(9)
    with torch.no_grad():
        z1, kl1 = v.encode(x)
        r1 = v.decode(z1)
    assert torch.equal(z0, z1) and torch.equal(r0, r1)
    assert torch.equal(l0, F.mse_loss(r1, x) + 1e-6 * kl1)
    # frozen parameters: the inference path too
    for p in v.parameters():
        p.requires_grad_(False)
    torch.manual_seed(9)
    r2, z2, l2, _ = v(x)
    assert r2.grad_fn is None and torch.equal(r2, r0) and torch.equal(z2, z0)


def test_stale_vae_tape_is_refused(cuda, sd0):
    from dmx import _lib
    v = _vae(sd0, cuda)
    x = _x((2, 3, 32, 32)).to(cuda)
    l1 = v(x)[2]
    l2 = v(x)[2]
    with pytest.raises(_lib.DmxError, match="stale tape"):
        l1.backward()
    l2.backward()
    assert all(p.grad is not None for p in v.parameters())
