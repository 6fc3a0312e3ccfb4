"""The float64 mode of the VAE training oracle and the preconditions of the bound the GPU tests of the native
VAE training step (tests/test_gpu_vae_train_classes.py) derive from it.  CPU only; nothing here touches the
code under test.

The oracle is torch autograd over oracle.ref.vae_encode / vae_decode with every leaf and input cast to the
dtype asked for (those functions are dtype-agnostic).  Its loss, with row weights r_n and a loss scale c, is

  c sum_n r_n ( w_recon sum((x_recon_n - x_n)^2) / numel(x) + w_z sum(z_n^2) / numel(z) + w_kl kl_n / N )

which for r = 1 is  w_recon mse(x_recon, x) + w_z mean(z^2) + w_kl mean(kl)  — VAE.forward's loss at the weights
(1, 0, 1e-6), the three-cotangent loss of tests/test_gpu_vae_train.py at (1, 0.3, 0.5).  Without row weights
the loss is spelled the second way, so that the fp32 run is test_vae_train_oracle.oracle_step's bit for bit.

The bound is the one of tests/test_train_oracle_f64.py (FACTOR, CAP, e32, tensor_errs, row_errs are imported
from there, not restated): E32 = max over tensors |g32 - g64| / |g64| is the fp32 oracle's own rounding noise,
a native tensor passes within FACTOR E32, and FACTOR E32 <= CAP keeps a noisy reference from opening it."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_train_oracle_f64 import CAP, FACTOR, e32, is_zero, rel_l2, row_errs, tensor_errs, threads  # noqa: E402
from test_forward_oracle_f64 import SPREAD_MIN_B, spread  # noqa: E402
from test_vae_train_oracle import GOLD, oracle_step  # noqa: E402
from oracle import ref  # noqa: E402
from dmx import synth  # noqa: E402

FWD_LOSS = dict(w_recon=1.0, w_z=0.0, w_kl=1e-6)    # VAE.forward's own loss
THREE_LOSS = dict(w_recon=1.0, w_z=0.3, w_kl=0.5)   # O(1) weights on all three outputs
LOSSES = {"fwd": FWD_LOSS, "three": THREE_LOSS}

# (n, h, w) of the GPU module's plan classes (its CLASSES dict says what each is there for) and edge shapes
CLASS_SHAPES = [(1, 8, 8), (5, 40, 24), (2, 56, 48), (17, 16, 16), (17, 32, 32), (64, 16, 16), (65, 8, 8),
                (64, 32, 32), (1, 128, 128)]
THREE_SHAPES = [(5, 40, 24), (64, 16, 16), (2, 56, 48)]
EDGE_SHAPES = [(3, 24, 16), (2, 56, 48)]
LIVE_SHAPE = (17, 16, 16)
# shapes of tests/test_gpu_vae_train.py that are no class here: the bound's precondition holds there too
CPU_ONLY_SHAPES = [(2, 64, 64)]


def make_case(n, h, w, seed=None):
    """x uniform in [0, 1) of shape (n, 3, h, w) and the reparameterisation draw eps = randn (n, 4, h/8, w/8)
    from one seeded generator (default seed: a function of the shape)."""
    g = torch.Generator().manual_seed(100000 * n + 100 * h + w if seed is None else seed)
    x = torch.rand((n, 3, h, w), generator=g)
    eps = torch.randn((n, 4, h // 8, w // 8), generator=g)
    return SimpleNamespace(n=n, h=h, w=w, x=x, eps=eps)


def weights():
    return synth.vae_weights(0)


def _forward(sd, c, dtype):
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = c.x.to(dtype)
    z, kl_mean, mu, logvar = ref.vae_encode(leaves, x, c.eps.to(dtype))
    x_recon = ref.vae_decode(leaves, z)
    kl = 0.5 * torch.sum(torch.exp(logvar) + mu ** 2 - 1.0 - logvar, dim=(1, 2, 3)) / (c.h * c.w)
    return leaves, x, x_recon, z, kl, kl_mean


def _row_terms(x, x_recon, z, kl, w_recon, w_z, w_kl):
    """Per-sample loss terms (n,); a term whose weight is 0 is left out of the graph."""
    t = torch.zeros(x.size(0), dtype=x.dtype)
    if w_recon != 0.0:
        t = t + w_recon * ((x_recon - x) ** 2).flatten(1).sum(1) / x.numel()
    if w_z != 0.0:
        t = t + w_z * (z ** 2).flatten(1).sum(1) / z.numel()
    if w_kl != 0.0:
        t = t + w_kl * kl / x.size(0)
    return t


def oracle(sd, c, dtype, w_recon=1.0, w_z=0.0, w_kl=1e-6, row_w=None, scale=1.0):
    """The module docstring's loss -> x_recon, z, kl (per sample), loss (unscaled), grads {name: tensor or
    None} (None: the loss does not reach the parameter) of scale x loss."""
    leaves, x, x_recon, z, kl, kl_mean = _forward(sd, c, dtype)
    if row_w is None:
        loss = None
        for wt, term in ((w_recon, lambda: F.mse_loss(x_recon, x)), (w_z, lambda: z.square().mean()),
                         (w_kl, lambda: kl_mean)):
            if wt != 0.0:
                loss = wt * term() if loss is None else loss + wt * term()
    else:
        loss = (row_w.to(dtype) * _row_terms(x, x_recon, z, kl, w_recon, w_z, w_kl)).sum()
    grads = torch.autograd.grad(loss if scale == 1.0 else loss * scale, list(leaves.values()), allow_unused=True)
    return SimpleNamespace(x_recon=x_recon.detach(), z=z.detach(), kl=kl.detach(), loss=loss.detach(),
                           grads=dict(zip(leaves.keys(), grads)))


def oracle_rows(sd, c, dtype, w_recon=1.0, w_z=0.0, w_kl=1e-6):
    """[{name: grad}] per sample: the gradients of each sample's own loss term (row_w = a unit vector), from one
    forward."""
    leaves, x, x_recon, z, kl, _ = _forward(sd, c, dtype)
    t = _row_terms(x, x_recon, z, kl, w_recon, w_z, w_kl)
    return [dict(zip(leaves.keys(), torch.autograd.grad(t[i], list(leaves.values()), retain_graph=True,
                                                        allow_unused=True))) for i in range(c.n)]


_PAIR, _ROWS = {}, {}


def oracle_pair(key, sd, c, **kw):
    """(fp32 oracle, float64 oracle) of one case and loss, computed once per key and not modified."""
    if key not in _PAIR:
        threads()
        _PAIR[key] = (oracle(sd, c, torch.float32, **kw), oracle(sd, c, torch.float64, **kw))
    return _PAIR[key]


def rows_pair(key, sd, c, **kw):
    """(fp32, float64) oracle_rows of one case and loss, once per key."""
    if key not in _ROWS:
        threads()
        _ROWS[key] = (oracle_rows(sd, c, torch.float32, **kw), oracle_rows(sd, c, torch.float64, **kw))
    return _ROWS[key]


def kl_errs(a, b):
    """Per-sample relative difference of the scalar KL."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return [float(abs(a[i] - b[i]) / abs(b[i])) for i in range(a.numel())]


def upper_clamp_weights(bias=40.0, channel=2):
    """The weights with to_logvar.bias raised on one channel so that its unclamped logvar exceeds 20."""
    sd = {k: v.clone() for k, v in weights().items()}
    sd["to_logvar.bias"][channel] = bias
    return sd


# ---- the CPU pins ------------------------------------------------------------------------------------
_ALL = ([(s, "fwd") for s in CLASS_SHAPES + EDGE_SHAPES[:1] + CPU_ONLY_SHAPES]
        + [(s, "three") for s in CLASS_SHAPES + EDGE_SHAPES[:1] + CPU_ONLY_SHAPES])


@pytest.mark.parametrize("shape,loss", _ALL, ids=lambda v: str(v).replace(" ", ""))
def test_cap_and_zero_pattern(shape, loss):
    """Every GPU case under both losses: FACTOR E32 <= CAP for the gradients and for the per-sample forward
    outputs, the two oracles agree on which tensors are exactly zero, and from SPREAD_MIN_B samples on the fp32
    oracle's own per-sample worst / median is below 2."""
    sd, c = weights(), make_case(*shape)
    o32, o64 = oracle_pair((shape, loss), sd, c, **LOSSES[loss])
    assert all(v is None or v.dtype == torch.float64 for v in o64.grads.values())
    E = e32(o32.grads, o64.grads)
    own_r, own_z, own_k = row_errs(o32.x_recon, o64.x_recon), row_errs(o32.z, o64.z), kl_errs(o32.kl, o64.kl)
    print(f"[vae f64 {shape} {loss}] E32 {E:.2e}; per sample x_recon {max(own_r):.2e} z {max(own_z):.2e} (min "
          f"{min(own_z):.2e}) kl {max(own_k):.2e}")
    assert [n for n in sd if is_zero(o32.grads[n]) != is_zero(o64.grads[n])] == []
    assert not any(is_zero(g) for g in o64.grads.values())
    assert 0.0 < FACTOR * E <= CAP, E
    assert abs(float(o32.loss) - float(o64.loss)) <= 1e-5 * float(o64.loss)
    for own in (own_r, own_z, own_k):
        assert FACTOR * max(own) <= CAP, own
    assert min(own_r) > 0.0 and min(own_z) > 0.0
    if c.n >= SPREAD_MIN_B:  # (z has as few as 4 numbers per sample: its spread is wider than x_recon's)
        print(f"[vae f64 {shape} {loss}] worst / median: x_recon {spread(own_r):.2f}, z {spread(own_z):.2f}")
        assert spread(own_r) < 2.0, spread(own_r)


@pytest.mark.parametrize("k", [-24, 24])
def test_loss_scale_scales_every_float64_gradient(k):
    sd, c, s = weights(), make_case(3, 24, 16), 2.0 ** k
    threads()
    g1 = oracle(sd, c, torch.float64, **THREE_LOSS)
    gs = oracle(sd, c, torch.float64, scale=s, **THREE_LOSS)
    assert float(gs.loss) == float(g1.loss)  # the returned loss is the unscaled one
    errs = tensor_errs(gs.grads, g1.grads, scale=s)
    assert len(errs) == len(sd) and errs[0][0] <= 1e-12, errs[:5]
    for n in sd:  # entry by entry, not only in norm
        d = (gs.grads[n] * 2.0 ** -k - g1.grads[n]).abs().max()
        assert float(d) <= 1e-12 * float(g1.grads[n].abs().max()), n


@pytest.mark.parametrize("loss", ["fwd", "three"])
def test_fp32_path_is_oracle_step(loss):
    """At the reference fixture's shape the fp32 run is test_vae_train_oracle.oracle_step's, bit for bit."""
    threads()
    sd = weights()
    x, eps = torch.from_numpy(GOLD["x"]), torch.from_numpy(GOLD["eps"])
    c = SimpleNamespace(n=x.size(0), h=x.size(2), w=x.size(3), x=x, eps=eps)
    fn = None if loss == "fwd" else (lambda xr, zz, k: F.mse_loss(xr, x) + 0.3 * zz.square().mean() + 0.5 * k)
    xr, z, l, grads = oracle_step(sd, x, eps, fn)
    o = oracle(sd, c, torch.float32, **LOSSES[loss])
    assert o.loss.dtype == torch.float32 and torch.equal(o.loss, l)
    assert torch.equal(o.x_recon, xr) and torch.equal(o.z, z)
    assert [n for n in sd if not torch.equal(o.grads[n], grads[n])] == []
    assert abs(float(o.kl.mean()) - float(GOLD["kl"])) <= 1e-5 * float(GOLD["kl"])


def test_row_weights_spell_the_same_loss():
    """row_w = 1 is the unweighted loss; row_w's gradients are linear in it; oracle_rows are its unit vectors."""
    threads()
    sd, c = weights(), make_case(3, 24, 16)
    a = oracle(sd, c, torch.float64, **THREE_LOSS)
    b = oracle(sd, c, torch.float64, row_w=torch.ones(3), **THREE_LOSS)
    assert abs(float(a.loss) - float(b.loss)) <= 1e-12 * float(a.loss)
    assert tensor_errs(b.grads, a.grads)[0][0] <= 1e-12
    r = torch.tensor([1.0, 2.0 ** -10, 0.0])
    w = oracle(sd, c, torch.float64, row_w=r, **THREE_LOSS)
    rows = oracle_rows(sd, c, torch.float64, **THREE_LOSS)
    mix = {n: sum(float(r[i]) * rows[i][n] for i in range(3)) for n in sd}
    assert tensor_errs(w.grads, mix)[0][0] <= 1e-12


@pytest.mark.parametrize("only", ["w_z", "w_kl"])
def test_decoder_takes_no_gradient_from_z_or_kl(only):
    """A z-only or KL-only loss does not reach the decoder: all 26 dec.* tensors are zero in both oracles, and
    every other tensor is not."""
    sd, c = weights(), make_case(3, 24, 16)
    kw = dict(w_recon=0.0, w_z=0.0, w_kl=0.0)
    kw[only] = THREE_LOSS[only]
    o32, o64 = oracle_pair(((3, 24, 16), only), sd, c, **kw)
    dec = [n for n in sd if n.startswith("dec.")]
    assert len(dec) == 26 and all(is_zero(o64.grads[n]) and is_zero(o32.grads[n]) for n in dec)
    assert not any(is_zero(o64.grads[n]) for n in sd if n not in dec)
    assert FACTOR * e32(o32.grads, o64.grads) <= CAP


def test_single_live_sample_cap_and_spread():
    """LIVE_SHAPE: each sample's own E32 (maximum over tensors of the gradient of that sample's loss term) keeps
    FACTOR E32 <= CAP, and the samples' worst / median is below 2."""
    sd, c = weights(), make_case(*LIVE_SHAPE)
    r32, r64 = rows_pair((LIVE_SHAPE, "fwd"), sd, c, **FWD_LOSS)
    own = [e32(a, b) for a, b in zip(r32, r64)]
    print(f"[vae f64 single live sample {LIVE_SHAPE}] E32 per sample {min(own):.2e} .. {max(own):.2e}, worst / "
          f"median {spread(own):.2f}")
    assert FACTOR * max(own) <= CAP and spread(own) < 2.0


def test_upper_clamp_case():
    """to_logvar.bias = 40 on channel 2: the unclamped logvar exceeds 20 everywhere on it, so that channel's rows
    of to_logvar.weight / .bias are exactly zero in both oracles, and the bound's precondition holds."""
    sd, c = upper_clamp_weights(), make_case(2, 32, 32)
    with torch.no_grad():  # the head is affine in its bias: the unclamped logvar is the plain one plus the raise
        lv = ref.vae_encode({k: v.double() for k, v in weights().items()}, c.x.double(), c.eps.double())[3][:, 2]
    assert -30.0 < float(lv.min()) and float(lv.max()) < 20.0
    assert float(lv.min()) + float(sd["to_logvar.bias"][2] - weights()["to_logvar.bias"][2]) > 20.0
    o32, o64 = oracle_pair(((2, 32, 32), "upper clamp"), sd, c, **THREE_LOSS)
    for k in ("to_logvar.weight", "to_logvar.bias"):
        for o in (o32, o64):
            assert float(o.grads[k][2].abs().max()) == 0.0 and float(o.grads[k][[0, 1, 3]].abs().min()) >= 0.0
            assert bool(o.grads[k][[0, 1, 3]].any())
    E = e32(o32.grads, o64.grads)
    print(f"[vae f64 upper clamp] E32 {E:.2e}, loss {float(o64.loss):.4e}")
    assert all(bool(torch.isfinite(g).all()) for g in o64.grads.values())
    assert FACTOR * E <= CAP, E
