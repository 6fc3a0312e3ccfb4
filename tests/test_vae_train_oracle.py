"""The VAE training-step oracle — torch autograd over oracle.ref.vae_forward with the state dict's
tensors set to requires_grad — pinned to the reference's own loss.backward() and Adam steps
(tests/golden/vae_train_step.npz, make_golden_vae_train.py).  CPU only.  It is the gradient
reference of tests/test_gpu_vae_train.py."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "diffusion-model_amd"))

from oracle import ref  # noqa: E402
from dmx import synth  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "vae_train_step.npz"))


def oracle_step(sd, x, eps, loss_fn=None):
    """-> (x_recon, z, loss, {name: grad}) of loss_fn(x_recon, z, kl) (kl = the per-sample KL's mean)
    over fresh leaf copies of sd; the default loss is VAE.forward's mse + 1e-6 kl (oracle.ref.vae_forward)."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    x_recon, z, loss, recon, kl = ref.vae_forward(params, x, eps)
    if loss_fn is not None:
        loss = loss_fn(x_recon, z, kl)
    grads = torch.autograd.grad(loss, list(params.values()))
    return x_recon.detach(), z.detach(), loss.detach(), dict(zip(params.keys(), grads))


def vae_grad_stats_close(grads, names, rel=2e-4):
    """Per parameter: sum and L2 of the gradient and 16 sampled entries vs the reference's, within
    rel of the tensor's L2 norm (the rule of test_train_oracle.grad_stats_close)."""
    idx, gsum, gl2, gval = GOLD["idx"], GOLD["g_sum"], GOLD["g_l2"], GOLD["g_val"]
    scale = float(np.max(gl2))
    bad = []
    for k, n in enumerate(names):
        g = grads[n].detach().double().cpu().reshape(-1)
        if abs(float(g.norm()) - gl2[k]) > rel * gl2[k] + 1e-9 * scale:
            bad.append((n, "l2", float(g.norm()), gl2[k]))
        if abs(float(g.sum()) - gsum[k]) > rel * gl2[k] * np.sqrt(g.numel()) + 1e-9 * scale:
            bad.append((n, "sum", float(g.sum()), gsum[k]))
        v = g[torch.from_numpy(idx[k])].numpy()
        if np.max(np.abs(v - gval[k])) > rel * gl2[k] + 1e-9 * scale:
            bad.append((n, "vals", float(np.max(np.abs(v - gval[k]))), gl2[k]))
    return bad


def params_after_close(params, names):
    """The sampled parameter entries after the two Adam steps vs the reference's, in the bound of
    test_two_adam_steps_match_reference scaled to this fixture's lr (first-step Adam updates are
    lr * sign(g): entries whose gradient is at rounding level may flip, the bulk agrees to rounding)."""
    idx, after, lr = GOLD["idx"], GOLD["p_after"], float(GOLD["lr"])
    got = np.stack([params[n].detach().cpu().reshape(-1)[torch.from_numpy(i)].numpy() for n, i in zip(names, idx)])
    d = np.abs(got - after)
    return d.max() <= 2.1 * lr and (d <= 1e-6 + 1e-5 * np.abs(after)).mean() >= 0.97, (float(d.max()),
                                                                                       float((d <= 1e-6 + 1e-5 * np.abs(after)).mean()))


def test_oracle_vae_grads_match_reference():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = synth.vae_weights(0)
    names = list(GOLD["names"])
    assert names == list(sd.keys())
    x, eps = torch.from_numpy(GOLD["x"]), torch.from_numpy(GOLD["eps"])
    torch.manual_seed(int(GOLD["seed"]))
    assert torch.equal(torch.randn(eps.shape), eps)  # the stored draw is the replay of the seed
    x_recon, z, loss, grads = oracle_step(sd, x, eps)
    assert abs(float(loss) - float(GOLD["loss"])) <= 1e-5 * float(GOLD["loss"])
    np.testing.assert_allclose(x_recon.numpy(), GOLD["x_recon"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(z.numpy(), GOLD["z"], rtol=1e-4, atol=1e-5)
    assert vae_grad_stats_close(grads, names) == []


def test_oracle_vae_two_adam_steps_match_reference():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = synth.vae_weights(0)
    names = list(sd.keys())
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(params.values(), lr=float(GOLD["lr"]))
    x = torch.from_numpy(GOLD["x"])
    for key in ("eps", "eps2"):
        opt.zero_grad(set_to_none=True)
        loss = ref.vae_forward(params, x, torch.from_numpy(GOLD[key]))[2]
        loss.backward()
        opt.step()
    ok, info = params_after_close(params, names)
    assert ok, info
