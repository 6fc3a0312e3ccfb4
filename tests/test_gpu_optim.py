"""The native optimizer step (dmx/optim.py, csrc/optim.h) on the device.

Synthetic list: sizes [1, 3, 63, 64, 65, C-1, C, C+1, 2C+5, 0] (C = the chunk size) plus three views
into one flat buffer at element offsets 1 (one element), 2 (C+1 elements, 8-byte aligned only) and C+3
(67 elements, 4-byte aligned only); the gradient of the C+1 tensor is itself a view at offset 1.  These
are the smallest cases where chunk tails, tensor boundaries and the 128-bit path can go wrong.

The comparison rule everywhere: the same fresh gradients go to the native optimizer, to
torch.optim.Adam(foreach=False, fused=False) on the CPU in fp32 (the reference) and to the same
formula in fp64 on the CPU (the truth).  For each of the state tensors p, exp_avg, exp_avg_sq (and
ema, grad_norm), taken over the whole list, the native max-abs error against the truth must be at
most 4 x the reference's (the update is about ten fp32 roundings whose order is free), and the
reference's own error must be non-zero so that the bound says something.

Measured on an MI355X (ten plain steps): see DESIGN.md §6q."""
import math
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

from test_train_oracle import GOLD, case_inputs, case_weights  # noqa: E402

from dmx.optim import CHUNK as C  # noqa: E402

SIZES = [1, 3, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5, 0]
VIEWS = [(1, 1), (2, C + 1), (C + 3, 67)]  # (element offset in the flat buffer, length)
FLAT = C + 3 + 67
N = len(SIZES) + len(VIEWS)
G_VIEW = SIZES.index(C + 1)  # this tensor's gradient is a view at element offset 1
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _values(seed=0):
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(FLAT, generator=g)
    return [torch.randn(n, generator=g) for n in SIZES] + [flat[o:o + n].clone() for o, n in VIEWS]


def _device_params(values, dev):
    flat = torch.zeros(FLAT, device=dev)
    ps = [torch.nn.Parameter(v.to(dev)) for v in values[:len(SIZES)]]
    for (o, n), v in zip(VIEWS, values[len(SIZES):]):
        flat[o:o + n] = v.to(dev)
        ps.append(torch.nn.Parameter(flat[o:o + n]))
    assert [p.data_ptr() % 16 for p in ps[len(SIZES):]] == [4, 8, 12]
    assert all(p.data_ptr() % 16 == 0 for p in ps[:len(SIZES)] if p.numel())
    return ps


def _grads(step, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(1000 * (seed + 1) + step)
    return [torch.randn(n, generator=g) * scale for n in SIZES + [n for _, n in VIEWS]]


def _set_device_grads(ps, grads, dev):
    for i, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
        elif i == G_VIEW:
            buf = torch.zeros(g.numel() + 1, device=dev)
            buf[1:] = g.to(dev)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = g.to(dev)


class Truth:
    """torch's single-tensor Adam rule (and clip_grad_norm_'s, and the EMA recurrence) in fp64."""

    def __init__(self, values, hp, ema=None, state=None):
        self.p = [v.double().clone() for v in values]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.step = [0] * len(self.p)
        self.hp = hp  # per tensor: dict(lr, wd, decoupled)
        self.ema_d = ema
        self.ema = [p.clone() for p in self.p]
        if state is not None:
            for i, st in state.items():
                self.m[i], self.v[i] = st["exp_avg"].double().cpu().clone(), st["exp_avg_sq"].double().cpu().clone()
                self.step[i] = int(st["step"])

    def update(self, grads, max_norm=None):
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))
        coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm is not None else 1.0
        b1, b2 = BETAS
        for i, g in enumerate(grads):
            if g is None:
                continue
            h = self.hp[i]
            g = g.double() * coef
            self.step[i] += 1
            if h["wd"] != 0 and h["decoupled"]:
                self.p[i] *= 1 - h["lr"] * h["wd"]
            elif h["wd"] != 0:
                g = g + h["wd"] * self.p[i]
            self.m[i] += (g - self.m[i]) * (1 - b1)
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            bc1, bc2 = 1 - b1 ** self.step[i], 1 - b2 ** self.step[i]
            self.p[i] -= (h["lr"] / bc1) * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + EPS)
            if self.ema_d is not None:
                self.ema[i] = self.ema_d * self.ema[i] + (1 - self.ema_d) * self.p[i]
        return norm


def _max_err(xs, truth):
    return max([float((x.detach().double().cpu() - t).abs().max()) for x, t in zip(xs, truth) if t.numel()] or [0.0])


def _check(what, kind, native, ref, truth):
    en, er = _max_err(native, truth), _max_err(ref, truth)
    print(f"[optim {what}] {kind}: native max|err| vs fp64 = {en:.3e}, fp32 reference = {er:.3e}")
    assert er > 0.0, (what, kind)
    assert en <= 4.0 * er, (what, kind, en, er)


def _state(opt, ps, key):
    return [opt.state[p][key] if key in opt.state.get(p, {}) else torch.zeros_like(p) for p in ps]


def _run(dev, what, steps=10, wd=0.0, decoupled=False, lrs=None, max_norm=None, ema=None, skip=None, gscale=None,
         check=True):
    """`steps` steps of all three evaluations.  lrs: per-tensor lr (two groups); skip: (tensor, steps without a
    gradient); gscale: the global gradient norm as a multiple of max_norm.  Returns what the tests look at."""
    from dmx.optim import Adam
    values = _values()
    lrs = lrs or [LR] * N
    groups = sorted(set(lrs), reverse=True)
    ps = _device_params(values, dev)
    cpu = [torch.nn.Parameter(v.clone()) for v in values]

    def grouped(params):
        return [{"params": [p for p, l in zip(params, lrs) if l == lr], "lr": lr} for lr in groups]
    opt = Adam(grouped(ps), lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, decoupled=decoupled, max_grad_norm=max_norm,
               ema_decay=ema)
    ref = torch.optim.Adam(grouped(cpu), lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, decoupled_weight_decay=decoupled,
                           foreach=False, fused=False)
    truth = Truth(values, [dict(lr=l, wd=wd, decoupled=decoupled) for l in lrs], ema=ema)
    ref_ema = [v.clone() for v in values]
    out = dict(opt=opt, ps=ps, ref=ref, cpu=cpu, truth=truth, norms=[], ref_norms=[], true_norms=[], coefs=[],
               grads_intact=True, frozen=None)
    for s in range(1, steps + 1):
        grads = _grads(s)
        if gscale is not None:
            total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
            grads = [g * (gscale * max_norm / total) for g in grads]
        if skip is not None and s in skip[1]:
            grads[skip[0]] = None
            if out["frozen"] is None:
                p = ps[skip[0]]
                out["frozen"] = [p.detach().clone()] + [opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq")]
        _set_device_grads(ps, grads, dev)
        before = [None if p.grad is None else p.grad.clone() for p in ps]
        opt.step()
        out["grads_intact"] &= all(b is None or torch.equal(b, p.grad) for b, p in zip(before, ps))
        for q, g in zip(cpu, grads):
            q.grad = None if g is None else g.clone()
        if max_norm is not None:
            out["ref_norms"].append(float(torch.nn.utils.clip_grad_norm_(cpu, max_norm, foreach=False)))
            out["norms"].append(opt.grad_norm.clone())
            out["coefs"].append(opt.clip_coef.clone())
        ref.step()
        if ema is not None:
            with torch.no_grad():
                for e, q in zip(ref_ema, cpu):
                    e.mul_(ema).add_(q, alpha=1 - ema)
        out["true_norms"].append(truth.update(grads, max_norm))
    out["norms"] = [float(x) for x in out["norms"]]
    out["coefs"] = [float(x) for x in out["coefs"]]
    if check:
        _check(what, "p", ps, cpu, truth.p)
        for key, t in (("exp_avg", truth.m), ("exp_avg_sq", truth.v)):
            _check(what, key, _state(opt, ps, key), _state(ref, cpu, key), t)
        if ema is not None:
            _check(what, "ema", _state(opt, ps, "ema"), ref_ema, truth.ema)
        if max_norm is not None:
            en = max(abs(a - b) for a, b in zip(out["norms"], out["true_norms"]))
            er = max(abs(a - b) for a, b in zip(out["ref_norms"], out["true_norms"]))
            print(f"[optim {what}] grad_norm: native max|err| vs fp64 = {en:.3e}, fp32 reference = {er:.3e}")
            assert er > 0.0 and en <= 4.0 * er, (en, er)
    return out


# ---- the synthetic list ---------------------------------------------------------------------------------
def test_ten_steps_against_fp64(cuda):
    out = _run(cuda, "plain")
    assert out["opt"].grad_norm is None
    assert [int(out["opt"].state[p]["step"]) for p in out["ps"]] == [10] * N
    assert out["grads_intact"]


@pytest.mark.parametrize("what,kw", [("coupled wd", dict(wd=0.01)), ("decoupled wd", dict(wd=0.01, decoupled=True)),
                                     ("two lrs", dict(lrs=[LR if i % 2 == 0 else 3e-4 for i in range(N)]))])
def test_variants_against_fp64(cuda, what, kw):
    out = _run(cuda, what, **kw)
    assert out["grads_intact"]
    if "lrs" in kw:
        assert len(out["opt"].param_groups) == 2


def test_skipped_tensor_keeps_its_state_and_step(cuda):
    i = SIZES.index(2 * C + 5)
    out = _run(cuda, "grad None on steps 3-5", skip=(i, (3, 4, 5)))
    opt, ps, ref, cpu = out["opt"], out["ps"], out["ref"], out["cpu"]
    assert float(opt.state[ps[i]]["step"]) == float(ref.state[cpu[i]]["step"]) == 7.0
    assert all(float(opt.state[p]["step"]) == 10.0 for j, p in enumerate(ps) if j != i)
    _check("skipped tensor", "p", [ps[i]], [cpu[i]], [out["truth"].p[i]])
    for key, t in (("exp_avg", out["truth"].m), ("exp_avg_sq", out["truth"].v)):
        _check("skipped tensor", key, [opt.state[ps[i]][key]], [ref.state[cpu[i]][key]], [t[i]])
    # while it had no gradient, nothing of it moved: replay steps 1-5 and compare with the snapshot taken after step 2
    again = _run(cuda, "replay", steps=5, skip=(i, (3, 4, 5)), check=False)
    p = again["ps"][i]
    now = [p.detach()] + [again["opt"].state[p][k] for k in ("exp_avg", "exp_avg_sq")]
    assert all(torch.equal(a, b) for a, b in zip(now, again["frozen"]))
    assert float(again["opt"].state[p]["step"]) == 2.0


def test_clipping_above_and_below_the_threshold(cuda):
    hi = _run(cuda, "clip, norm = 10 max_norm", max_norm=1.0, gscale=10.0)
    assert all(abs(n - 10.0) < 1e-3 for n in hi["norms"]) and all(abs(c - 0.1) < 1e-4 for c in hi["coefs"])
    assert hi["grads_intact"]  # the scaled gradient is never stored
    lo = _run(cuda, "clip, norm = 0.1 max_norm", max_norm=1.0, gscale=0.1)
    assert all(abs(n - 0.1) < 1e-5 for n in lo["norms"])
    assert lo["coefs"] == [1.0] * 10  # exactly
    from dmx.optim import Adam  # the unclipped twin on the same scaled gradients
    ps = _device_params(_values(), cuda)
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    for s in range(1, 11):
        grads = _grads(s)
        total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
        _set_device_grads(ps, [g * (0.1 / total) for g in grads], cuda)
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(ps, lo["ps"]))  # coef == 1 changes no bit


def test_ema_against_fp64_and_exact_swap(cuda):
    out = _run(cuda, "ema 0.9", ema=0.9)
    opt, ps = out["opt"], out["ps"]
    emas = [opt.state[p]["ema"] for p in ps]
    p0, e0 = [p.detach().clone() for p in ps], [e.clone() for e in emas]
    assert any(not torch.equal(a, b) for a, b in zip(p0, e0))
    v0 = [p._version for p in ps]
    with opt.ema_weights():
        assert all(torch.equal(p, e) for p, e in zip(ps, e0)) and all(torch.equal(e, p) for e, p in zip(emas, p0))
        assert all(p._version > v for p, v in zip(ps, v0))
    assert all(torch.equal(p, q) for p, q in zip(ps, p0)) and all(torch.equal(e, f) for e, f in zip(emas, e0))
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    assert all(torch.equal(p, q) for p, q in zip(ps, p0)) and all(torch.equal(e, f) for e, f in zip(emas, e0))
    dst = [torch.zeros_like(p) for p in ps]
    opt.copy_ema_to(dst)
    assert all(torch.equal(d, e) for d, e in zip(dst, e0))


def test_same_steps_twice_give_the_same_bits(cuda):
    kw = dict(wd=0.01, max_norm=1.0, gscale=10.0, ema=0.9, check=False)
    a, b = _run(cuda, "first", **kw), _run(cuda, "second", **kw)
    for key in (None, "exp_avg", "exp_avg_sq", "ema"):
        xa = a["ps"] if key is None else _state(a["opt"], a["ps"], key)
        xb = b["ps"] if key is None else _state(b["opt"], b["ps"], key)
        assert all(torch.equal(x, y) for x, y in zip(xa, xb)), key
    assert a["norms"] == b["norms"] and a["coefs"] == b["coefs"]


def test_gradient_buffers_keep_their_bits(cuda):
    out = _run(cuda, "clip + coupled wd + ema", steps=3, wd=0.01, max_norm=1.0, gscale=10.0, ema=0.9, check=False)
    assert out["grads_intact"]


def test_empty_steps_do_nothing(cuda):
    from dmx.optim import Adam
    ps = _device_params(_values(), cuda)
    p0 = [p.detach().clone() for p in ps]
    opt = Adam(ps, max_grad_norm=1.0, ema_decay=0.9)
    v0 = [p._version for p in ps]
    opt.step()  # no tensor has a gradient
    assert all(torch.equal(p, q) for p, q in zip(ps, p0)) and [p._version for p in ps] == v0
    assert float(opt.grad_norm) == 0.0 and float(opt.clip_coef) == 1.0
    assert all(float(opt.state[p]["step"]) == 0.0 and torch.equal(opt.state[p]["ema"], p) for p in ps)
    e = torch.nn.Parameter(torch.zeros(0, device=cuda))
    e.grad = torch.zeros(0, device=cuda)
    only_empty = Adam([e])
    only_empty.step()
    assert float(only_empty.state[e]["step"]) == 1.0


@pytest.mark.parametrize("native_first", [True, False])
def test_checkpoints_move_between_the_optimizers(cuda, native_first):
    """Three steps on one side, its state_dict() into the other, two more steps on each side with the same gradients."""
    from dmx.optim import Adam
    values = _values()
    hp = [dict(lr=LR, wd=0.0, decoupled=False)] * N
    if native_first:
        ps = _device_params(values, cuda)
        first = Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    else:
        ps = [torch.nn.Parameter(v.clone()) for v in values]
        first = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=False, fused=False)
    for s in range(1, 4):
        if native_first:
            _set_device_grads(ps, _grads(s), cuda)
        else:
            for p, g in zip(ps, _grads(s)):
                p.grad = g
        first.step()
    now = [p.detach().cpu().clone() for p in ps]
    sd = first.state_dict()
    dps = ps if native_first else _device_params(now, cuda)
    cps = [torch.nn.Parameter(v.clone()) for v in now] if native_first else ps
    nat = first if native_first else Adam(dps, lr=1.0)
    cpu = torch.optim.Adam(cps, lr=1.0, foreach=False, fused=False) if native_first else first
    (cpu if native_first else nat).load_state_dict(sd)
    assert nat.param_groups[0]["lr"] == cpu.param_groups[0]["lr"] == LR
    truth = Truth(now, hp, state={i: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.items()}
                                  for i, st in sd["state"].items()})
    assert truth.step == [3] * N
    for s in range(4, 6):
        grads = _grads(s)
        _set_device_grads(dps, grads, cuda)
        nat.step()
        for q, g in zip(cps, grads):
            q.grad = g.clone()
        cpu.step()
        truth.update(grads)
    what = "native -> torch" if native_first else "torch -> native"
    assert all(float(nat.state[p]["step"]) == 5.0 for p in dps) and all(float(cpu.state[q]["step"]) == 5.0 for q in cps)
    _check(what, "p", dps, cps, truth.p)
    for key, t in (("exp_avg", truth.m), ("exp_avg_sq", truth.v)):
        _check(what, key, _state(nat, dps, key), _state(cpu, cps, key), t)


def test_refused_gradients_on_the_device(cuda):
    from dmx.optim import Adam
    p = torch.nn.Parameter(torch.zeros(4, 6, device=cuda))
    opt = Adam([p])
    p.grad = torch.zeros(6, 4, device=cuda).t()  # not contiguous
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    h = torch.nn.Parameter(torch.zeros(4, device=cuda, dtype=torch.float16))
    with pytest.raises(ValueError, match="fp32"):
        h.grad = torch.zeros(4, device=cuda, dtype=torch.float16)
        Adam([h]).step()
    s = torch.nn.Parameter(torch.zeros(4, 6, device=cuda))
    s.grad = torch.zeros(4, 6, device=cuda).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        Adam([s]).step()
    assert opt.state_dict()["state"] == {}


# ---- the real networks ------------------------------------------------------------------------------------
def _model(tag, dev):
    from models.unet_cond_geom import UnetCondWithGeomHead
    sd, geom, shallow = case_weights(tag)
    assert geom and not shallow
    m = UnetCondWithGeomHead()
    m.load_state_dict(sd)
    return m.to(dev).train()


def _loss(m, inputs, dev, lam):
    from losses.geom_losses import masked_geom_mse
    x, t, y, vals, mask, noise, gt = (v.to(dev) if v is not None else None for v in inputs)
    eps, g = m(x, t, y, cond_vals=vals, cond_mask=mask)
    return F.mse_loss(eps, noise) + lam * masked_geom_mse(g, gt, mask)


def test_two_native_adam_steps_match_reference(cuda):
    """test_gpu_train.py's test_two_adam_steps_match_reference with the native optimizer: the same golden
    parameters and the same bounds (they are dominated by the gradients, not the optimizer)."""
    from dmx.optim import Adam
    tag = "g"
    m = _model(tag, cuda)
    lam = float(GOLD[f"{tag}_lam"])
    opt = Adam(m.parameters(), lr=1e-4)
    for second in (False, True):
        loss = _loss(m, case_inputs(tag, second), cuda, lam)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    names = [n for n, _ in m.named_parameters()]
    ps = dict(m.named_parameters())
    idx, after = GOLD[f"{tag}_idx"], GOLD[f"{tag}_p_after"]
    got = np.stack([ps[n].detach().cpu().reshape(-1)[torch.from_numpy(i)].numpy() for n, i in zip(names, idx)])
    d = np.abs(got - after)
    bulk = float((d <= 1e-6 + 1e-5 * np.abs(after)).mean())
    print("[optim unet] max |dp| vs reference:", float(d.max()), "bulk:", bulk)
    assert d.max() <= 2.1e-4
    assert bulk >= 0.97


def test_refresh_after_native_step_and_under_ema_weights(cuda):
    """The kernels write the parameters through raw pointers; the version bump makes the next forward repack
    them (dmx_model_refresh): after step(), inside ema_weights() and after leaving it, the eval forward equals
    that of a fresh module holding the same weights, and the native model is refreshed, not rebuilt."""
    from dmx.optim import Adam
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = _model("g", cuda)
    nm0 = m.native()
    opt = Adam(m.parameters(), lr=1e-3, ema_decay=0.5)
    loss = _loss(m, case_inputs("g"), cuda, 0.5)
    opt.zero_grad()
    loss.backward()
    opt.step()
    x, t, y, vals, mask, _, _ = (v.to(cuda) if v is not None else None for v in case_inputs("g"))
    m.eval()

    def fwd(mod):
        with torch.no_grad():
            return mod(x, t, y, cond_vals=vals, cond_mask=mask)
    e1, g1 = fwd(m)
    assert m.native() is nm0  # refreshed, not rebuilt
    fresh = UnetCondWithGeomHead().to(cuda).eval()
    fresh.load_state_dict(m.state_dict())
    e2, g2 = fwd(fresh)
    assert torch.equal(e1, e2) and torch.equal(g1, g2)
    averaged = UnetCondWithGeomHead().to(cuda).eval()
    averaged.load_state_dict(m.state_dict())
    opt.copy_ema_to(averaged)
    e3, g3 = fwd(averaged)
    assert not torch.equal(e3, e1)
    with opt.ema_weights():
        e4, g4 = fwd(m)
        assert m.native() is nm0
    assert torch.equal(e4, e3) and torch.equal(g4, g3)
    e5, g5 = fwd(m)
    assert m.native() is nm0
    assert torch.equal(e5, e1) and torch.equal(g5, g1)


def test_vae_step_matches_torch_adam(cuda):
    """One step of the VAE at the smallest shape test_gpu_vae_train.py uses; both sides take the gradients of
    one native backward, cloned."""
    from dmx import synth
    from dmx.optim import Adam
    from models.vae import VAE
    sd = synth.vae_weights(0)
    v = VAE()
    v.load_state_dict(sd)
    v.to(cuda).train()
    x = torch.rand((3, 3, 24, 16), generator=torch.Generator().manual_seed(7)).to(cuda)
    torch.manual_seed(11)
    loss = v(x)[2]
    v.zero_grad(set_to_none=True)
    loss.backward()
    ps = list(v.parameters())
    values = [p.detach().cpu().clone() for p in ps]
    grads = [p.grad.detach().cpu().clone() for p in ps]
    cpu = [torch.nn.Parameter(t.clone()) for t in values]
    for q, g in zip(cpu, grads):
        q.grad = g.clone()
    ref = torch.optim.Adam(cpu, lr=LR, betas=BETAS, eps=EPS, foreach=False, fused=False)
    ref.step()
    truth = Truth(values, [dict(lr=LR, wd=0.0, decoupled=False)] * len(ps))
    truth.update(grads)
    nm0 = v.native()
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    opt.step()
    _check("vae", "p", ps, cpu, truth.p)
    for key, t in (("exp_avg", truth.m), ("exp_avg_sq", truth.v)):
        _check("vae", key, _state(opt, ps, key), _state(ref, cpu, key), t)
    v.eval()
    with torch.no_grad():
        v(x)
    assert v.native() is nm0
