"""Golden vectors of the VAE training step (train_vae.py: `_, _, loss, _ = vae(x);
loss.backward(); optimizer.step()`), from the reference's own models/vae.py (build container
only; the reference never travels to the GPU box).

Run from the repo root:  python tests/golden/make_golden_vae_train.py

vae_train_step.npz: the reference VAE() with weights = dmx.synth.vae_weights(0) in train mode on
the CPU, x ~ U[0,1) of shape (2,3,32,32), two steps of torch.optim.Adam(lr=1e-3), each preceded by
torch.manual_seed(seed) / manual_seed(seed2) so that encode's randn_like draw can be replayed
(eps, eps2 are those draws).  Stored: x, the seeds, eps, eps2, the first step's x_recon, z, loss,
recon_mse and kl, and per parameter (state_dict order) in the scheme of train_step.npz the
gradient's sum and L2 norm, 16 sampled gradient entries, and the same 16 entries of the parameter
after the two Adam steps.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
SAMPLES = 16
SEED, SEED2 = 7, 8


def main():
    torch.set_num_threads(8)
    sys.path.insert(0, os.path.join(REPO, "diffusion-model_amd"))
    from dmx import synth  # our seeded weight generator (no reference code)
    sys.path.insert(0, REF)
    from models.vae import VAE  # noqa: E402  (reference)

    m = VAE()
    m.load_state_dict(synth.vae_weights(0))
    m.train()
    names = [n for n, _ in m.named_parameters()]
    x = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(SEED))
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    rec = {"x": x.numpy(), "seed": np.int64(SEED), "seed2": np.int64(SEED2), "names": np.array(names),
           "lr": np.float64(1e-3)}
    for step, seed in enumerate((SEED, SEED2)):
        torch.manual_seed(seed)
        x_recon, z, loss, parts = m(x)
        torch.manual_seed(seed)
        eps = torch.randn(z.shape)  # the randn_like(std) draw of encode, replayed
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 0:
            ps = dict(m.named_parameters())
            rng = np.random.default_rng(SEED)
            idx = np.stack([rng.integers(0, ps[n].numel(), SAMPLES) for n in names])
            rec.update({
                "eps": eps.numpy(), "x_recon": x_recon.detach().numpy(), "z": z.detach().numpy(),
                "loss": np.float64(loss.item()), "recon": np.float64(parts["recon_mse"].item()),
                "kl": np.float64(parts["kl"].item()), "idx": idx,
                "g_sum": np.array([float(ps[n].grad.double().sum()) for n in names]),
                "g_l2": np.array([float(ps[n].grad.double().norm()) for n in names]),
                "g_val": np.stack([ps[n].grad.reshape(-1)[torch.from_numpy(i)].numpy() for n, i in zip(names, idx)]),
            })
        else:
            rec["eps2"] = eps.numpy()
        opt.step()
    ps = dict(m.named_parameters())
    rec["p_after"] = np.stack([ps[n].detach().reshape(-1)[torch.from_numpy(i)].numpy()
                               for n, i in zip(names, rec["idx"])])
    np.savez_compressed(os.path.join(HERE, "vae_train_step.npz"), **rec)
    print("[golden-vae-train] loss=%.6f recon=%.6f kl=%.6f" % (rec["loss"], rec["recon"], rec["kl"]))


if __name__ == "__main__":
    main()
