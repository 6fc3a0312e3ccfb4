"""The float64 mode of the training oracle (oracle/train_ref.py, dtype=torch.float64) and the bound the
GPU gradient tests derive from it.  CPU only; tests/test_gpu_train_classes.py imports the helpers.

The float64 oracle is the fp32 oracle's graph with the leaves and every floating input cast up; t and y
stay integers and the sinusoidal table of t keeps the reference's fp32 values.  Its distance from the
fp32 oracle is the fp32 oracle's own rounding noise, E32, measured without any code under test:

  E32(case) = max over tensors of |g32 - g64| / |g64|        (L2 norms, tensors with g64 == 0 left out)

A native tensor passes when |native - g64| / |g64| <= FACTOR * E32 with FACTOR = 8 = 4 x 2: the x3 split
carries a product to about 2^-22 where fp32 carries 2^-24 (4), and a different, fixed summation order
accounts for the other 2.  FACTOR * E32 <= CAP = 5e-5 is asserted too, so that a noisy reference cannot
open the bound.  A tensor whose float64 gradient is exactly zero (or None) must be exactly zero."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_train_oracle import GOLD, case_inputs, case_weights, grad_stats_close  # noqa: E402
from oracle import train_ref  # noqa: E402
from dmx import synth  # noqa: E402

LAM = 0.5        # the geometry term's weight in every case's loss
FACTOR = 8.0     # native bound = FACTOR * E32
CAP = 5e-5       # and FACTOR * E32 may not exceed this
F64_VS_F32 = 1e-5  # the two oracles against each other, per tensor (measured here: 2.4e-6, 4.7e-6)


def threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def make_case(B, hw, shallow=False, zero_mask_row=None):
    """Seeded inputs of one training step: t over 1..1000 with 1 and 1000 present when B >= 2, row 1
    CFG-dropped (label 0, zeroed vals and mask) when B >= 3, a target gt of its own for the geometry
    term.  shallow: the UnetCond case (no vals / mask / gt).  zero_mask_row: that row's mask zeroed."""
    g = torch.Generator().manual_seed(1000 * B + hw)
    x = torch.randn((B, 4, hw, hw), generator=g)
    t = torch.randint(1, 1001, (B,), generator=g)
    y = torch.randint(1, 4, (B,), generator=g)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    noise = torch.randn((B, 4, hw, hw), generator=g)
    gt = torch.rand((B, 12), generator=g)
    if B >= 2:
        t[0], t[-1] = 1, 1000
    if B >= 3:
        y[1] = 0
        vals[1] = 0.0
        mask[1] = 0.0
    if zero_mask_row is not None:
        mask[zero_mask_row] = 0.0
    if shallow:
        vals = mask = gt = None
    return SimpleNamespace(B=B, hw=hw, x=x, t=t, y=y, vals=vals, mask=mask, noise=noise, gt=gt, shallow=shallow)


def weights(shallow=False):
    if not shallow:
        return synth.unet_cond_geom_weights(0)
    sd = synth.unet_cond_geom_weights(0, remove_deep_conv=True)
    return {k: v for k, v in sd.items() if not k.startswith("geom_head.")}


def oracle(sd, c, dtype, w_eps=1.0, w_geom=LAM, row_w=None):
    """loss = w_eps mse(eps, noise) + w_geom masked_geom_mse(geom, gt, mask), each sample's share of both
    terms weighted by row_w (default 1), with the parameters and x as leaves -> loss, eps, geom, grads
    {name: tensor or None}, dx.  A term whose weight is 0 is left out of the graph."""
    cast = lambda v: v.to(dtype) if v is not None else None  # noqa: E731
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xl = c.x.to(dtype).clone().requires_grad_(True)
    eps, g = train_ref.forward(leaves, xl, c.t, c.y, c.vals, c.mask, not c.shallow, c.shallow, dtype)
    r = torch.ones(c.B, dtype=dtype) if row_w is None else row_w.to(dtype)
    loss = eps.sum() * 0.0
    if w_eps != 0.0:
        loss = loss + w_eps * (r.view(-1, 1, 1, 1) * (eps - cast(c.noise)) ** 2).sum() / eps.numel()
    if g is not None and w_geom != 0.0:
        m = cast(c.mask)
        loss = loss + w_geom * (r.view(-1, 1) * (g - cast(c.gt)) ** 2 * m).sum() / m.sum().clamp_min(1e-6)
    loss.backward()
    return SimpleNamespace(loss=loss.detach(), eps=eps.detach(), geom=None if g is None else g.detach(),
                           grads={k: v.grad for k, v in leaves.items()}, dx=xl.grad)


def is_zero(g):
    return g is None or not bool(g.any())


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def tensor_errs(grads, g64, scale=1.0):
    """[(rel-L2 of grads[n] against scale * g64[n], n)] over the tensors whose float64 gradient is not zero."""
    return sorted(((rel_l2(grads[n], g64[n] * scale), n) for n in g64 if not is_zero(g64[n])), reverse=True)


def e32(g32, g64):
    return tensor_errs(g32, g64)[0][0]


def row_errs(a, b):
    """Per-sample rel-L2 of a against b (rows of b that are exactly zero: |a| itself)."""
    a, b = a.detach().double().cpu().flatten(1), b.detach().double().cpu().flatten(1)
    return [float((a[i] - b[i]).norm() / b[i].norm()) if bool(b[i].any()) else float(a[i].norm())
            for i in range(a.shape[0])]


_PAIR = {}


def oracle_pair(key, sd, c, **kw):
    """(fp32 oracle, float64 oracle) of one case and loss, computed once per key and not modified."""
    if key not in _PAIR:
        threads()
        _PAIR[key] = (oracle(sd, c, torch.float32, **kw), oracle(sd, c, torch.float64, **kw))
    return _PAIR[key]


# ---- the CPU pins ------------------------------------------------------------------------------------
SHAPES = [(2, 12), (3, 16)]


@pytest.mark.parametrize("B,hw", SHAPES)
def test_float64_oracle_agrees_with_fp32_oracle(B, hw):
    threads()
    sd, c = weights(), make_case(B, hw)
    args = (sd, c.x, c.t, c.y, c.vals, c.mask, c.noise, c.gt, c.mask, LAM)
    l32, e32_, g32_, grads32 = train_ref.loss_and_grads(*args)
    l64, e64, g64_, grads64 = train_ref.loss_and_grads(*args, dtype=torch.float64)
    assert l32.dtype == torch.float32 and l64.dtype == torch.float64
    assert all(v.dtype == torch.float64 for v in grads64.values())
    assert abs(float(l32) - float(l64)) <= 1e-5 * float(l64)
    assert rel_l2(e32_, e64) <= F64_VS_F32 and rel_l2(g32_, g64_) <= F64_VS_F32
    errs = tensor_errs(grads32, grads64)
    print(f"[f64 oracle B={B} {hw}x{hw}] fp32 oracle vs float64, worst: {errs[:3]}")
    assert len(errs) == len(sd) and errs[0][0] <= F64_VS_F32, errs[:5]
    # the test helper (x a leaf as well, the loss spelled out per sample) is the same loss
    o = oracle(sd, c, torch.float64)
    assert abs(float(o.loss) - float(l64)) <= 1e-12 * float(l64)
    assert tensor_errs(o.grads, grads64)[0][0] <= 1e-12
    assert o.dx.dtype == torch.float64 and o.dx.shape == c.x.shape and bool(o.dx.any())


@pytest.mark.parametrize("B,hw", SHAPES)
def test_loss_scale_scales_every_float64_gradient(B, hw):
    threads()
    sd, c = weights(), make_case(B, hw)
    args = (sd, c.x, c.t, c.y, c.vals, c.mask, c.noise, c.gt, c.mask, LAM)
    l1, _, _, g1 = train_ref.loss_and_grads(*args, dtype=torch.float64)
    ls, _, _, gs = train_ref.loss_and_grads(*args, dtype=torch.float64, loss_scale=2.0 ** -12)
    assert float(ls) == float(l1)  # the returned loss is the unscaled one
    errs = tensor_errs(gs, g1, scale=2.0 ** -12)
    assert len(errs) == len(sd) and errs[0][0] <= 1e-12, errs[:5]
    for n in g1:  # and entry by entry, not only in norm
        d = (gs[n] * 2.0 ** 12 - g1[n]).abs().max()
        assert float(d) <= 1e-12 * float(g1[n].abs().max()), n


def test_default_dtype_is_todays_fp32_path():
    """dtype's default leaves the fp32 results bit for bit (nothing is cast), and so does an explicit
    torch.float32 on fp32 tensors (the casts return the same tensors)."""
    threads()
    sd, c = weights(), make_case(2, 12)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    eps, g = train_ref.ref.unet_cond_geom_forward(leaves, c.x, c.t, c.y, c.vals, c.mask, False)
    loss = torch.nn.functional.mse_loss(eps, c.noise) + LAM * train_ref.masked_geom_mse(g, c.gt, c.mask)
    loss.backward()
    l, e, gg, grads = train_ref.loss_and_grads(sd, c.x, c.t, c.y, c.vals, c.mask, c.noise, c.gt, c.mask, LAM)
    assert torch.equal(l, loss.detach()) and torch.equal(e, eps.detach()) and torch.equal(gg, g.detach())
    assert [n for n in sd if not torch.equal(grads[n], leaves[n].grad)] == []
    _, _, _, explicit = train_ref.loss_and_grads(sd, c.x, c.t, c.y, c.vals, c.mask, c.noise, c.gt, c.mask, LAM,
                                                 dtype=torch.float32)
    assert [n for n in sd if not torch.equal(explicit[n], grads[n])] == []


def test_no_dtype_runs_in_the_dtype_given():
    """Without dtype= nothing is cast: a caller that hands in float64 weights and inputs (tools/
    gelu_train_study.py's float64 arms) gets the float64 run, bit for bit the one dtype=torch.float64 makes
    of the fp32 tensors, and not the fp32 run."""
    threads()
    sd, c = weights(), make_case(2, 12)
    up = lambda v: v.double()  # noqa: E731
    sd64 = {k: up(v) for k, v in sd.items()}
    l64, e64, g64_, grads64 = train_ref.loss_and_grads(sd64, up(c.x), c.t, c.y, up(c.vals), up(c.mask), up(c.noise),
                                                       up(c.gt), up(c.mask), LAM)
    args = (sd, c.x, c.t, c.y, c.vals, c.mask, c.noise, c.gt, c.mask, LAM)
    lc, ec, gc, gradsc = train_ref.loss_and_grads(*args, dtype=torch.float64)
    assert l64.dtype == e64.dtype == g64_.dtype == torch.float64
    assert all(v.dtype == torch.float64 for v in grads64.values())
    assert torch.equal(l64, lc) and torch.equal(e64, ec) and torch.equal(g64_, gc)
    assert [n for n in sd if not torch.equal(grads64[n], gradsc[n])] == []
    _, _, _, grads32 = train_ref.loss_and_grads(*args)
    assert all(v.dtype == torch.float32 for v in grads32.values())
    assert tensor_errs(grads32, grads64)[0][0] > 1e-8  # (the two runs are different runs)
    eps, g = train_ref.forward(sd64, up(c.x), c.t, c.y, up(c.vals), up(c.mask))
    assert eps.dtype == g.dtype == torch.float64 and torch.equal(eps, ec)
    e32, _ = train_ref.forward(sd64, up(c.x), c.t, c.y, up(c.vals), up(c.mask), dtype=torch.float32)
    assert e32.dtype == torch.float32  # an explicit dtype casts, down as well as up


@pytest.mark.parametrize("tag", ["g", "c"])
def test_float64_grads_keep_the_reference_statistics(tag):
    """The float64 gradients, cast to fp32, against the reference's own recorded statistics."""
    threads()
    sd, geom, shallow = case_weights(tag)
    x, t, y, vals, mask, noise, gt = case_inputs(tag)
    loss, _, _, grads = train_ref.loss_and_grads(sd, x, t, y, vals, mask, noise, gt, mask, float(GOLD[f"{tag}_lam"]),
                                                 geom, shallow, dtype=torch.float64)
    assert abs(float(loss) - float(GOLD[f"{tag}_loss"])) <= 1e-5 * float(GOLD[f"{tag}_loss"])
    g32 = {k: (None if v is None else v.float()) for k, v in grads.items()}
    assert grad_stats_close(tag, g32, list(sd.keys())) == []
