"""What only the tests need, once: the model loaders, the overflow weights, the seeded conditions, the
device noise, small comparisons and the fresh-process worker runner.  A plain module next to the tests
(not a conftest); the rules the kernels are held to live in oracle/rules.py."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_model(dev, sd):
    """The conditional U-Net with the weights sd, on dev, in eval mode."""
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(sd)
    return m.to(dev).eval()


def make_vae(dev, sd):
    from models.vae import VAE
    v = VAE()
    v.load_state_dict(sd)
    return v.to(dev).eval()


def overflow_sd():
    """An overflowing GroupNorm gamma: the x3 split's hi plane leaves the f16 range in the first block."""
    from dmx import synth
    sd = synth.unet_cond_geom_weights(0)
    sd["inc.double_conv.1.weight"] = sd["inc.double_conv.1.weight"] * 1e5
    return sd


def cond(B, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.tensor([1 + i % 3 for i in range(B)])
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    return y, vals, mask


def device_noise(d, seed, shape, t, cuda):
    """The Philox normals a DDPM / DDIM step draws at timestep t: an eps-form update with x = eps = 0,
    c2 = sd = 1 returns them unchanged (none at t = 1)."""
    from dmx import engine
    n = d.num_timesteps
    z = torch.zeros(shape, device=cuda)
    tabs = (torch.zeros(n, device=cuda), torch.ones(n, device=cuda), torch.ones(n, device=cuda))
    return engine.ddpm_update(z, z, None, 0.0, torch.full((shape[0],), t, device=cuda), tabs, None, seed=seed).cpu()


def on(dev, *ts):
    return tuple(None if t is None else t.to(dev).contiguous() for t in ts)


def mode_tables(d, mode):
    """(rule, CPU tables) of a _sampler_mode result, as oracle.rules.trajectory takes them."""
    from oracle import ref
    if mode is None:
        return "ddpm", ref.schedule(d.num_timesteps)
    if mode[0] == "ddim":
        return "ddim", d.ddim_tables(mode[1], mode[2], "cpu")
    return "dpm", d.dpm_tables(mode[1], mode[2], "cpu")


def ulps(a, b):
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


def per_sample_rel(a, b):
    a, b = a.double().cpu().flatten(1), b.double().cpu().flatten(1)
    return [(float((a[i] - b[i]).norm() / b[i].norm()) if float(b[i].norm()) > 0 else float(a[i].norm()))
            for i in range(a.shape[0])]


def run_worker(tmp_path, tag, worker, clear=("DMX_POISON", "DMX_CHECK", "DMX_PRECISION"), timeout=240, **env_over):
    """Run the source `worker` (which sees ROOT and saves a dict of tensors to sys.argv[1]) in a fresh
    process under the environment plus env_over, the variables of `clear` removed unless given -> the dict."""
    path = str(tmp_path / f"out_{tag}.pt")
    env = dict(os.environ, **env_over)
    for k in clear:
        if k not in env_over:
            env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + worker, path], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(path, weights_only=True)
