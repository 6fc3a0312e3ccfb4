"""CPU-only: the training objective's host side — Diffuser.loss_weights, and Diffuser.training_loss on its
torch-op path (a foreign model on the CPU), which defines what the native kernels compute: the noised
latent bit for bit, the CFG dropout of the loop (train_latent_cond.py:136-159), the loss and its
gradients against autograd of the spelled-out expression, min-SNR weighting, geom_denom, the refusals."""
import inspect

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import diff
from losses.geom_losses import masked_geom_mse


# ---- loss_weights ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1000, 12])
def test_loss_weights(T):
    d = diff.Diffuser(T)
    u = d.loss_weights("uniform")
    assert u.dtype == torch.float32 and tuple(u.shape) == (T,) and torch.equal(u, torch.ones(T))
    assert torch.equal(d.loss_weights(), u)
    ab = torch.cumprod(1 - torch.linspace(0.0001, 0.02, T), dim=0)
    assert torch.equal(ab, d.alpha_bars)
    snr = ab.double() / (1 - ab.double())
    mid = float(snr[T // 2])  # a gamma inside the schedule's SNR range: both regimes occur
    for gamma in (5.0, mid):
        w = d.loss_weights("min_snr", snr_gamma=gamma)
        assert w.dtype == torch.float32 and tuple(w.shape) == (T,)
        assert torch.equal(w, (torch.minimum(snr, torch.tensor(gamma, dtype=torch.float64)) / snr).float())
        low = snr <= gamma
        assert torch.equal(w[low], torch.ones(int(low.sum())))
        assert bool((w[~low] < 1).all()) and bool((w > 0).all())
        if gamma == mid or T == 1000:
            assert 0 < int(low.sum()) < T
    for bad in ("snr", "", None, "MIN_SNR"):
        with pytest.raises(ValueError):
            d.loss_weights(bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), None, "5"):
        with pytest.raises(ValueError):
            d.loss_weights("min_snr", snr_gamma=bad)


# ---- the torch-op path ---------------------------------------------------------------------------------
class TinyNet(nn.Module):
    """Stands in for the network: every input reaches the outputs, and the inputs are recorded."""

    def __init__(self, gd=5, head=True):
        super().__init__()
        self.conv = nn.Conv2d(4, 4, 3, padding=1)
        self.emb = nn.Embedding(4, 4)
        self.cond = nn.Linear(2 * gd, 4)
        if head:
            self.geom_head = nn.Linear(4, gd)
        self.seen = None

    def forward(self, x, t, y, cond_vals=None, cond_mask=None):
        self.seen = (x, t, y, cond_vals, cond_mask)
        e = self.emb(y) + torch.sin(t.float() / 100.0).unsqueeze(1)
        if cond_vals is not None:
            e = e + self.cond(torch.cat([cond_vals, cond_mask], dim=1))
        h = self.conv(x) * (1 + e[:, :, None, None])
        if hasattr(self, "geom_head"):
            return h, self.geom_head(h.mean(dim=(2, 3)))
        return h


def _batch(T=1000, B=3, gd=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, 4, 8, 8), generator=g)
    noise = torch.randn((B, 4, 8, 8), generator=g)
    classes = torch.tensor([1, 3, 2])[:B]
    vals = torch.rand((B, gd), generator=g)
    mask = (torch.rand((B, gd), generator=g) > 0.3).float()
    mask[0, 0] = 1.0
    t = torch.tensor([1, T, 417])[:B]
    drop = torch.tensor([False, True, False])[:B]
    return z, noise, classes, vals, mask, t, drop


def _spelled_out(d, net, z, noise, classes, vals, mask, t, drop, lam, weights=None, denom=None):
    """train_latent_cond.py:137-159 as written there (add_noise's formula, the loop's dropout and losses)."""
    ab = d.alpha_bars[t - 1].view(-1, 1, 1, 1)
    z_noisy = torch.sqrt(ab) * z + torch.sqrt(1 - ab) * noise
    y_used = torch.where(drop, torch.zeros_like(classes), classes)
    keep = (~drop).float().unsqueeze(1)
    vals_used, mask_used = vals * keep, mask * keep
    eps, geom = net(z_noisy, t, y_used, cond_vals=vals_used, cond_mask=mask_used)
    if weights is None:
        loss_noise = F.mse_loss(eps, noise)
    else:
        loss_noise = (weights[t - 1] * ((eps - noise) ** 2).mean(dim=(1, 2, 3))).mean()
    loss_geom = masked_geom_mse(geom, vals, mask * keep, denom=denom)
    return loss_noise + lam * loss_geom, loss_noise, loss_geom, (z_noisy, y_used, vals_used, mask_used)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def test_training_loss_signature():
    p = inspect.signature(diff.Diffuser.training_loss).parameters
    assert list(p)[:6] == ["self", "model", "z", "classes", "cond", "cond_mask"]
    kw = {k: v.default for k, v in p.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert kw == dict(geom_lambda=0.0, cfg_drop_prob=0.0, null_label=0, weighting="uniform", snr_gamma=5.0, t=None,
                      noise=None, drop=None, geom_denom=None, sample_offset=0)


@pytest.mark.parametrize("weighting", ["uniform", "min_snr"])
def test_torch_path_matches_the_loop(weighting):
    torch.manual_seed(3)
    d = diff.Diffuser(1000)
    net = TinyNet()
    z, noise, classes, vals, mask, t, drop = _batch()
    lam = 0.5
    res = d.training_loss(net, z, classes, vals, mask, geom_lambda=lam, weighting=weighting, t=t, noise=noise,
                          drop=drop)
    seen = net.seen
    net.zero_grad(set_to_none=True)
    res.loss.backward()
    got = {n: p.grad.clone() for n, p in net.named_parameters()}
    w = None if weighting == "uniform" else d.loss_weights("min_snr")
    if w is not None:
        assert float(w[t - 1].min()) < 1.0  # the weighting is not vacuous on this batch
    ref, ref_noise, ref_geom, used = _spelled_out(d, net, z, noise, classes, vals, mask, t, drop, lam, w)
    # the model saw add_noise's bits and the loop's dropped inputs
    assert torch.equal(seen[0], used[0]) and torch.equal(seen[1], t)
    assert torch.equal(seen[2], used[1]) and seen[2][1] == 0
    assert torch.equal(seen[3], used[2]) and torch.equal(seen[4], used[3])
    assert float(seen[3][1].abs().sum()) == 0.0 and float(seen[4][1].abs().sum()) == 0.0
    assert torch.equal(seen[3][0], vals[0]) and torch.equal(seen[4][2], mask[2])
    assert abs(float(res.loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
    assert abs(float(res.noise_loss) - float(ref_noise.detach())) <= 1e-6 * abs(float(ref_noise.detach()))
    assert abs(float(res.geom_loss) - float(ref_geom.detach())) <= 1e-6 * abs(float(ref_geom.detach()))
    assert abs(float(res.per_sample.mean()) - float(ref_noise.detach())) <= 1e-6 * abs(float(ref_noise.detach()))
    net.zero_grad(set_to_none=True)
    ref.backward()
    for n, p in net.named_parameters():
        assert _rel(got[n], p.grad) <= 1e-6, n
    assert res.loss.requires_grad and not res.noise_loss.requires_grad and not res.per_sample.requires_grad
    assert torch.equal(res.t, t) and torch.equal(res.drop, drop) and res.drop.dtype == torch.bool
    assert tuple(res.per_sample.shape) == (3,) and tuple(res.eps.shape) == tuple(z.shape)
    assert tuple(res.geom.shape) == (3, 5)


def test_geom_denom_is_honoured():
    torch.manual_seed(3)
    d = diff.Diffuser(1000)
    net = TinyNet()
    z, noise, classes, vals, mask, t, drop = _batch()
    den = torch.tensor(7.25)
    res = d.training_loss(net, z, classes, vals, mask, geom_lambda=0.5, t=t, noise=noise, drop=drop, geom_denom=den)
    ref, _, ref_geom, _ = _spelled_out(d, net, z, noise, classes, vals, mask, t, drop, 0.5, denom=den)
    own = d.training_loss(net, z, classes, vals, mask, geom_lambda=0.5, t=t, noise=noise, drop=drop)
    assert abs(float(res.loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
    assert abs(float(res.geom_loss) - float(ref_geom.detach())) <= 1e-6 * abs(float(ref_geom.detach()))
    keep = (~drop).float().unsqueeze(1)
    ratio = float((mask * keep).sum()) / 7.25
    assert abs(float(res.geom_loss) - ratio * float(own.geom_loss)) <= 1e-6 * float(res.geom_loss)
    f = d.training_loss(net, z, classes, vals, mask, geom_lambda=0.5, t=t, noise=noise, drop=drop, geom_denom=7.25)
    assert float(f.loss.detach()) == float(res.loss.detach())


def test_draws_follow_torch_generator_and_no_grad():
    d = diff.Diffuser(50)
    net = TinyNet()
    z, _, classes, vals, mask, _, _ = _batch(T=50)
    torch.manual_seed(11)
    a = d.training_loss(net, z, classes, vals, mask, cfg_drop_prob=0.5)
    torch.manual_seed(11)
    b = d.training_loss(net, z, classes, vals, mask, cfg_drop_prob=0.5)
    assert torch.equal(a.t, b.t) and torch.equal(a.drop, b.drop) and float(a.loss.detach()) == float(b.loss.detach())
    assert int(a.t.min()) >= 1 and int(a.t.max()) <= 50
    assert not bool(d.training_loss(net, z, classes, vals, mask, cfg_drop_prob=0.0).drop.any())
    assert bool(d.training_loss(net, z, classes, vals, mask, cfg_drop_prob=1.0).drop.all())
    with torch.no_grad():
        c = d.training_loss(net, z, classes, vals, mask)
    assert c.loss.grad_fn is None and not c.loss.requires_grad
    # a model without a head and without a condition: the noise loss alone
    plain = TinyNet(head=False)
    r = d.training_loss(plain, z, classes)
    assert plain.seen[3] is None and r.geom is None and float(r.geom_loss) == 0.0
    assert float(r.loss.detach()) == float(r.noise_loss)


def test_refusals_draw_nothing():
    d = diff.Diffuser(1000)
    net, plain = TinyNet(), TinyNet(head=False)
    z, noise, classes, vals, mask, t, drop = _batch()
    cases = [
        (net, (z, classes, vals, mask), dict(weighting="snr")),
        (net, (z, classes, vals, mask), dict(weighting="min_snr", snr_gamma=0.0)),
        (net, (z[0], classes, vals, mask), {}),
        (net, (z, classes[:2], vals, mask), {}),
        (net, (z, classes, vals[:2], mask[:2]), {}),
        (net, (z, classes, vals, mask[:, :4]), {}),
        (net, (z, classes, vals, mask), dict(t=t[:2])),
        (net, (z, classes, vals, mask), dict(noise=noise[:, :3])),
        (net, (z, classes, vals, mask), dict(drop=drop[:1])),
        (net, (z, classes, vals, None), {}),
        (net, (z, classes, None, mask), {}),
        (plain, (z, classes, vals, mask), dict(geom_lambda=0.5)),
        (net, (z, classes), dict(geom_lambda=0.5)),
        (net, (z, classes, vals, mask), dict(geom_lambda=-0.5)),
        (net, (z, classes, vals, mask), dict(geom_lambda=float("nan"))),
        (net, (z, classes, vals, mask), dict(geom_lambda=float("inf"))),
        (net, (z, classes, vals, mask), dict(cfg_drop_prob=-0.1)),
        (net, (z, classes, vals, mask), dict(cfg_drop_prob=1.1)),
        (net, (z, classes, vals, mask), dict(cfg_drop_prob=float("nan"))),
        (net, (z, classes, vals, mask), dict(drop=drop, cfg_drop_prob=0.1)),
        (net, (z, classes, vals, mask), dict(t=torch.tensor([0, 5, 9]))),
        (net, (z, classes, vals, mask), dict(t=torch.tensor([1, 1001, 9]))),
    ]
    torch.manual_seed(5)
    before = torch.get_rng_state()
    for model, args, kw in cases:
        model.seen = None
        with pytest.raises(ValueError):
            d.training_loss(model, *args, **kw)
        assert model.seen is None
        assert torch.equal(torch.get_rng_state(), before), kw
    # and the same call with nothing wrong does draw
    d.training_loss(net, z, classes, vals, mask)
    assert not torch.equal(torch.get_rng_state(), before)
