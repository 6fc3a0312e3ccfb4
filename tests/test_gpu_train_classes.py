"""GPU: the training backward (include/dmx.h dmx_train_forward / dmx_train_backward / dmx_train_backward_input)
against the float64 training oracle, over the shapes at which the backward's plan changes and over the
cotangent magnitudes its operand scales see.

Every comparison uses the bound of tests/test_train_oracle_f64.py: with g64 / g32 the float64 / fp32
oracle's gradients of the same case, E32 = max over tensors |g32 - g64| / |g64| is the reference's own
rounding noise, and a native tensor passes when |native - g64| / |g64| <= 8 E32 (8 E32 <= 5e-5 asserted).
A tensor whose float64 gradient is exactly zero or None must be exactly zero in what
NativeModel.train_backward returns (the drop-in module turns an unused branch's tensor into None).

The native side is driven through NativeModel.train_forward / train_backward / input_grad with the
cotangents computed in torch from the native eps and geom:
  d_eps = w_eps r_n 2 (eps - noise) / numel,   d_geom = w_geom r_n 2 mask (geom - gt) / max(sum mask, 1e-6),
the derivative of  w_eps mse(eps, noise) + w_geom masked_geom_mse(geom, gt, mask)  with row weights r_n,
times the loss scale c — so every scale below is exact.

Homogeneity.  Every operand scale of the backward is ldexpf(1, e) with e from ilogbf of a maximum of |dY|
(common.h amax_exp, clamped at +-100, 0 for a zero or non-finite maximum), the backward is linear in the
cotangents, and multiplying by a power of two commutes with every rounding short of under- or overflow:
the gradients of c times the cotangents are c times the gradients, bit for bit (test_loss_scale).

Measured on an MI355X: DESIGN.md §6b, "Float64 parity over the plan classes"."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_train_oracle_f64 import (CAP, FACTOR, LAM, e32, is_zero, make_case, oracle_pair, rel_l2,  # noqa: E402
                                   row_errs, tensor_errs, weights)

LOSS_TOL = 2e-5

# (B, H = W): the smallest shapes that reach each decision of the taped forward and the backward
# (engine.hip conv_plan / dec_n, train_engine.h wgrad / gn_bwd / colsum / ln_bwd launches).
CLASSES = {
    (1, 8): "maps 8/4/2/1: attention forward and adjoint at L = 1, GroupNorm adjoint with HW = 1 (gn_bwd chunks "
            "= 1), weight gradients with M = 1 (one split, rps = 16), ln_bwd with one token, W < 16 so inc's "
            "first conv leaves conv_in_kernel",
    (2, 12): "maps 12/6/3/1: the Up pad and its adjoint at 1->2 into 3 (one-sided pad), none at 3->6",
    (5, 20): "maps 20/10/5/2: conv_in_kernel<16>, L = 400/100/25/4 (no multiple of 64 or 16), pad at 2->4 into 5, "
             "ragged batch",
    (3, 36): "W > 32, the general input conv; L = 1296 (21 key chunks, the last of 16) and 324/81/16; pad at "
             "4->8 into 9",
    (1, 32): "single sample: gn_bwd chunks = min(512, HW/16) = 64, weight-gradient splits from M alone",
    (17, 32): "M = 17408 at the top: two-pass colsum (rows > 256), ln_bwd block cap 512 (1088 wanted), "
              "weight-gradient splits limited by the 512 / 1024 block targets",
    (64, 16): "the >= 64-sample class (dec_n = 128): 128-row GEMM tiles (tiles128 >= 256) in the taped forward and "
              "in dgrad, gn_bwd chunks = min(512/N, HW/16)",
    (65, 8): "the same class, ragged, on 8/4/2/1 maps: the last tile holds one sample",
}
EDGE_SHAPES = [(3, 16), (2, 28)]
SCALES = [2.0 ** -24, 2.0 ** -12, 2.0 ** 12, 2.0 ** 24]
INPUT_GRAD_SHAPES = [(1, 8), (5, 20), (3, 36), (64, 16)]


@pytest.fixture(scope="module")
def nm(cuda, unet_sd):
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(unet_sd)
    m.to(cuda).train()
    return m, m.native()


def cotangents(c, eps, geom, w_eps=1.0, w_geom=LAM, row_w=None, scale=1.0):
    """The loss's derivative at the native outputs (the module docstring's formulas), on the device."""
    dev = eps.device
    r = torch.ones(c.B, device=dev) if row_w is None else row_w.to(dev)
    d_eps = (w_eps * scale) * r.view(-1, 1, 1, 1) * 2.0 * (eps - c.noise.to(dev)) / eps.numel()
    d_geom = None
    if geom is not None:
        mask = c.mask.to(dev)
        d_geom = (w_geom * scale) * r.view(-1, 1) * 2.0 * mask * (geom - c.gt.to(dev)) / mask.sum().clamp_min(1e-6)
    return d_eps, d_geom


def native_loss(c, eps, geom, w_eps=1.0, w_geom=LAM):
    eps, loss = eps.double().cpu(), 0.0
    if w_eps:
        loss = w_eps * float(((eps - c.noise.double()) ** 2).mean())
    if geom is not None and w_geom:
        m = c.mask.double()
        loss += w_geom * float(((geom.double().cpu() - c.gt.double()) ** 2 * m).sum() / m.sum().clamp_min(1e-6))
    return loss


def run(model, c, **kw):
    """Taped forward and parameter backward of case c -> (grads, eps, geom, tape, d_eps, d_geom)."""
    dev = model.device
    dv = [None if v is None else v.to(dev) for v in (c.x, c.t, c.y, c.vals, c.mask)]
    eps, geom, tape = model.train_forward(*dv)
    d_eps, d_geom = cotangents(c, eps, geom, **kw)
    return model.train_backward(tape, d_eps, d_geom), eps, geom, tape, d_eps, d_geom


def check(what, grads, o32, o64, scale=1.0):
    """The module docstring's bound, per tensor; prints E32, the worst five and their ratio to E32."""
    E = e32(o32.grads, o64.grads)
    assert set(grads) == set(o64.grads)
    for n, g in o64.grads.items():
        assert bool(torch.isfinite(grads[n]).all()), n
        if is_zero(g):
            assert not bool(grads[n].any()), f"{n}: the float64 gradient is exactly zero, the native one is not"
    errs = tensor_errs(grads, o64.grads, scale)
    worst = ", ".join(f"{n} {e:.2e} ({e / E:.2f})" for e, n in errs[:5])
    print(f"[{what}] E32 = {E:.2e}, bound {FACTOR * E:.2e}; native worst (x E32): {worst}")
    assert FACTOR * E <= CAP, E
    assert errs[0][0] <= FACTOR * E, errs[:5]
    return E, errs


SPREAD_MIN_B = 16  # batches from which a median over the samples means something
SPREAD = 2.0


def check_dx(what, dx, o32, o64):
    """The input gradient, per sample, E32 taken per sample: sample n passes when its rel-L2 against the
    float64 oracle is within 8 x the fp32 oracle's own error for that sample (8 x the worst of those <= CAP);
    a sample whose float64 gradient is exactly zero must be exactly zero.
    From SPREAD_MIN_B samples on, also the spread: worst / median of the native errors <= SPREAD x worst /
    median of the fp32 oracle's.  The samples of a batch go through the same launches with the same operand
    scales, so their rounding errors are draws of one distribution, as the fp32 oracle's are; the oracle's
    own worst / median says how far the worst of that many draws stands from the middle, and 2 is the
    allowance for a different summation order that the bound itself makes.  One sample at several times its
    neighbours is a defect in what only that sample's values reach (the query split of
    test_attention_query_split_at_an_f16_tie stood at 10.2 here against the oracle's 1.27, and stands at 1.16 since), even where its
    own 8 E32 still holds it (it did: 7.0)."""
    assert bool(torch.isfinite(dx).all())
    own, errs = row_errs(o32.dx, o64.dx), row_errs(dx, o64.dx)
    zero = [not bool(r.any()) for r in o64.dx.flatten(1)]
    live = [n for n in range(len(errs)) if not zero[n]]
    E = max(own[n] for n in live)
    worst = max(live, key=lambda n: errs[n] / own[n])
    print(f"[{what}] d_x per sample: E32 worst {E:.2e}; native worst {max(errs[n] for n in live):.2e}, worst ratio "
          f"to its own E32 {errs[worst] / own[worst]:.2f} (sample {worst})")
    assert FACTOR * E <= CAP, E
    for n in range(len(errs)):
        if zero[n]:
            assert errs[n] == 0.0, (n, errs[n])
        else:
            assert errs[n] <= FACTOR * own[n], (n, errs[n], own[n])
    if len(live) >= SPREAD_MIN_B:
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        nat, ref = [errs[n] for n in live], [own[n] for n in live]
        s_nat, s_ref = max(nat) / med(nat), max(ref) / med(ref)
        print(f"[{what}] d_x spread worst / median: native {s_nat:.2f}, fp32 oracle {s_ref:.2f}")
        assert s_nat <= SPREAD * s_ref, (s_nat, s_ref)
    return E, errs


# ---- the plan classes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hw", list(CLASSES), ids=[f"{b}x{h}" for b, h in CLASSES])
def test_plan_class(nm, unet_sd, B, hw):
    """CLASSES says which decision each shape is there for."""
    c = make_case(B, hw)
    o32, o64 = oracle_pair((B, hw), unet_sd, c)
    grads, eps, geom, _, _, _ = run(nm[1], c)
    loss = native_loss(c, eps, geom)
    assert abs(loss - float(o64.loss)) <= LOSS_TOL * float(o64.loss), (loss, float(o64.loss))
    assert rel_l2(eps, o64.eps) <= 1e-4 and rel_l2(geom, o64.geom) <= 1e-4
    check(f"class B={B} {hw}x{hw}", grads, o32, o64)


def test_shallow_class(cuda):
    """UnetCond(remove_deep_conv=True) without vals / mask at (4, 20): no bot2, no condition MLP (its
    gradients exactly zero), no GeomHead."""
    from models.unet_cond import UnetCond
    B, hw = 4, 20
    sd, c = weights(shallow=True), make_case(B, hw, shallow=True)
    m = UnetCond(cfg_drop_prob=0.0, remove_deep_conv=True)
    m.load_state_dict(sd)
    model = m.to(cuda).train().native()
    o32, o64 = oracle_pair((B, hw, "shallow"), sd, c)
    assert all(o64.grads[n] is None for n in sd if n.startswith("cond_mlp."))
    grads, eps, geom, _, _, _ = run(model, c)
    assert geom is None
    loss = native_loss(c, eps, None)
    assert abs(loss - float(o64.loss)) <= LOSS_TOL * float(o64.loss), (loss, float(o64.loss))
    check(f"shallow B={B} {hw}x{hw}", grads, o32, o64)


# ---- cotangent edge cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hw", EDGE_SHAPES)
def test_zero_d_eps(nm, unet_sd, B, hw):
    """A geometry-only loss, d_eps a tensor of zeros: max|dY| = 0 on every eps-only path (amax_exp's
    zero case).  out.* are exactly zero, everything is finite and within the bound of that loss's oracle."""
    c = make_case(B, hw)
    o32, o64 = oracle_pair((B, hw, "geom only"), unet_sd, c, w_eps=0.0)
    assert is_zero(o64.grads["out.weight"]) and is_zero(o64.grads["out.bias"])
    grads, _, _, tape, d_eps, d_geom = run(nm[1], c, w_eps=0.0)
    assert not bool(d_eps.any()) and bool(d_geom.any())
    check(f"zero d_eps B={B} {hw}x{hw}", grads, o32, o64)
    check_dx(f"zero d_eps B={B} {hw}x{hw}", nm[1].input_grad(tape, d_eps, d_geom), o32, o64)


@pytest.mark.parametrize("B,hw", EDGE_SHAPES)
def test_zero_d_geom(nm, unet_sd, B, hw):
    """geom_lambda = 0, d_geom a tensor of zeros: the GeomHead's gradients are exactly zero."""
    c = make_case(B, hw)
    o32, o64 = oracle_pair((B, hw, "eps only"), unet_sd, c, w_geom=0.0)
    assert all(is_zero(g) for n, g in o64.grads.items() if n.startswith("geom_head."))
    grads, _, _, _, d_eps, d_geom = run(nm[1], c, w_geom=0.0)
    assert d_geom is not None and not bool(d_geom.any())
    check(f"zero d_geom B={B} {hw}x{hw}", grads, o32, o64)
    assert all(not bool(g.any()) for n, g in grads.items() if n.startswith("geom_head."))


def native_geom_seed(model, geom, target, mask):
    """include/dmx.h dmx_geom_seed: L_n = sum_j m_nj (geom_nj - v_nj)^2 / max(sum_j m_nj, 1e-6) and its
    derivative in geom, row by row, on the device -> (loss (n,), seed (n, geom_dim))."""
    from dmx.engine import _ptr, _stream, check as dmx_check
    n = geom.shape[0]
    loss = torch.empty((n,), device=geom.device, dtype=torch.float32)
    seed = torch.empty_like(geom)
    with torch.cuda.device(geom.device):
        dmx_check(model.lib.dmx_geom_seed(_ptr(geom), _ptr(target), _ptr(mask), n, model.geom_dim, _ptr(loss),
                                          _ptr(seed), ctypes.c_void_p(_stream(geom.device))))
    return loss, seed


@pytest.mark.parametrize("B,hw", EDGE_SHAPES)
def test_all_zero_mask_row(nm, unet_sd, B, hw):
    """The last row keeps its label and vals but has an all-zero mask.  The native geometry seed
    (dmx_geom_seed, what a geometry-guided step seeds the backward with) of that row and its loss are
    exactly zero, the other rows are 2 m (geom - gt) / sum m; that row's share of the input gradient of the
    native seed is exactly zero; and the parameter gradients of the training loss stay within the bound."""
    c = make_case(B, hw, zero_mask_row=B - 1)
    o32, o64 = oracle_pair((B, hw, "zero mask row"), unet_sd, c)
    grads, _, geom, tape, d_eps, d_geom = run(nm[1], c)
    check(f"zero mask row B={B} {hw}x{hw}", grads, o32, o64)
    dev = geom.device
    gt, mask = c.gt.to(dev).contiguous(), c.mask.to(dev).contiguous()
    loss, seed = native_geom_seed(nm[1], geom, gt, mask)
    assert not bool(seed[-1].any()) and float(loss[-1]) == 0.0
    want = 2.0 * mask.double() * (geom.double() - gt.double()) / mask.double().sum(-1, keepdim=True).clamp_min(1e-6)
    live = [n for n in range(B) if bool(c.mask[n].any())]
    assert live and all(rel_l2(seed[n], want[n]) <= 1e-6 for n in live)
    assert all(not bool(seed[n].any()) for n in range(B) if n not in live)
    dx = nm[1].input_grad(tape, None, seed)
    assert not bool(dx[-1].any()) and bool(dx[live[0]].any())


# ---- loss scales ----------------------------------------------------------------------------------------
_BASE = {}


def base_run(model, c):
    """The unscaled forward, parameter backward and input gradient of a shape, once (the runs repeat bit for
    bit: test_gpu_train.py test_backward_bits_do_not_depend_on_what_ran_before)."""
    if (c.B, c.hw) not in _BASE:
        grads, _, _, tape, d_eps, d_geom = run(model, c)
        _BASE[(c.B, c.hw)] = (grads, model.input_grad(tape, d_eps, d_geom), d_eps, d_geom)
    return _BASE[(c.B, c.hw)]


@pytest.mark.parametrize("B,hw", EDGE_SHAPES)
@pytest.mark.parametrize("k", [-24, -12, 12, 24])
def test_loss_scale(nm, unet_sd, B, hw, k):
    """Both cotangents times c = 2^k: (a) the gradients meet the bound against c g64, (b) times 1/c they
    equal the unscaled run's bit for bit (the module docstring's homogeneity property)."""
    c, s = make_case(B, hw), 2.0 ** k
    o32, o64 = oracle_pair((B, hw), unet_sd, c)
    base, dx1, d_eps, d_geom = base_run(nm[1], c)
    grads, _, _, tape, d_eps_s, d_geom_s = run(nm[1], c, scale=s)
    dxs = nm[1].input_grad(tape, d_eps_s, d_geom_s)
    assert torch.equal(d_eps_s * (1.0 / s), d_eps) and torch.equal(d_geom_s * (1.0 / s), d_geom)
    check(f"loss scale 2^{k} B={B} {hw}x{hw}", grads, o32, o64, scale=s)                  # (a)
    differ = [n for n in base if not torch.equal(grads[n] * (1.0 / s), base[n])]          # (b)
    assert differ == [], differ
    assert torch.equal(dxs * (1.0 / s), dx1)


# ---- the finding: hi and lo of the attention query from two different roundings ---------------------------
def test_attention_query_split_at_an_f16_tie(cuda, unet_sd):
    """Found through test_input_grad_class at (64, 16): sample 35's d_x sat at 1.6e-5 (4.75 E32) where its
    neighbours sat at 1.5e-6, whatever the batch around it.  Cause (igemm_x3.h attention_x3_kernel /
    attention16_kernel, the forward core of the default mode and of the taped forward): the query operand
    q log2(e) / sqrt(D) was split in plain C and the compiler took hi from the fp32-rounded product and lo
    from the unrounded one (common.h split4_scaled).  In sa3 of that sample, head 0, token 0, channel 39,
    the product lies at an f16 tie, hi and lo came from different neighbours, the element was off by 2^-11
    and that query's softmax weights by 3e-5: its output 6.4e-5 wrong, carried on into every gradient below
    sa3.  Of the slices compared below that one stood at 3.6e-5 and the other fifteen at 4.9e-7 .. 7.4e-7
    before the fix; after it the sixteen stand at 4.0e-7 .. 6.7e-7, that one at 5.6e-7.

    Here: that sample alone, sa3 with out_proj = identity and a zero second FF layer, so the block returns
    its attention output plus xl, the output of its first LayerNorm (the block's residual is that LayerNorm
    output, not the block's input: oracle/ref.py attention, models/unet_cond.py:48), and a (token, head)
    slice of it shows one query's weights.  Each slice within
    1e-5 rel-L2 of the float64 oracle: the split carries a product to 2^-22 = 2.4e-7, a score is 64 products
    of |q| |k| / 8 = 8, which bounds a weight's error near 1e-6 and the slice's below that; one element with
    mismatched halves costs 2^-11 of itself and puts the slice 3.6 times over the bound."""
    from oracle import ref
    from models.unet_cond_geom import UnetCondWithGeomHead
    c, i = make_case(64, 16), 35
    sd = dict(unet_sd)
    sd["sa3.mha.out_proj.weight"] = torch.eye(256)
    for k in ("sa3.mha.out_proj.bias", "sa3.ff_self.3.weight", "sa3.ff_self.3.bias"):
        sd[k] = torch.zeros_like(unet_sd[k])
    x, t, y, vals, mask = (v[i:i + 1] for v in (c.x, c.t, c.y, c.vals, c.mask))
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        emb = ref.cond_embedding(sd64, t, y, vals.double(), mask.double())
        h = ref.resblock(sd64, "inc", x.double(), False)
        h = ref.attention(sd64, "sa1", ref.down(sd64, "down1", h, emb))
        h = ref.attention(sd64, "sa2", ref.down(sd64, "down2", h, emb))
        want = ref.attention(sd64, "sa3", ref.down(sd64, "down3", h, emb))      # (1, 256, 2, 2)
    want = want.permute(0, 2, 3, 1).reshape(4, 4, 64)                           # [token][head][d]
    m = UnetCondWithGeomHead()
    m.load_state_dict(sd)
    nat = m.to(cuda).eval().native()
    with torch.no_grad():
        got = nat.forward_taps(*(v.to(cuda) for v in (x, t, y, vals, mask)))["sa3"]
    got = got.double().cpu().reshape(4, 4, 64)
    errs = (got - want).norm(dim=-1) / want.norm(dim=-1)
    print(f"[attention split] (token, head) rel-L2 of sa3's attention output + xl:\n{errs.numpy()}")
    assert float(errs.max()) <= 1e-5, errs


# ---- the input gradient ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hw", INPUT_GRAD_SHAPES)
def test_input_grad_class(nm, unet_sd, B, hw):
    """The data-only backward that geometry guidance runs, on the classes' tapes: check_dx's per-sample bound
    (each sample within 8 x its own E32) and, at (64, 16), its spread check."""
    c = make_case(B, hw)
    o32, o64 = oracle_pair((B, hw), unet_sd, c)
    dv = [v.to(nm[1].device) for v in (c.x, c.t, c.y, c.vals, c.mask)]
    eps, geom, tape = nm[1].train_forward(*dv)
    check_dx(f"input_grad B={B} {hw}x{hw}", nm[1].input_grad(tape, *cotangents(c, eps, geom)), o32, o64)


def test_input_grad_mixed_magnitude(nm, unet_sd):
    """Row 1's cotangents are 2^-10 of the others' at (3, 16); every row, the small one included, stays
    within the bound.  The limit this pins: the backward scales a whole tensor by one power of two that
    puts its largest |dY| in [2^12, 2^13), and an element keeps a normal f16 lo part (so the split's full
    precision) down to 2^-16 of that largest value.  A sample 2^-10 below its neighbours is inside that
    range; a coarser scaling (a narrower lo range, or no lo part for small elements) would lose it."""
    B, hw = 3, 16
    c = make_case(B, hw, zero_mask_row=None)
    c.mask[1] = (torch.arange(12) % 2).float()  # the small row takes part in the geometry term too
    row_w = torch.tensor([1.0, 2.0 ** -10, 1.0])
    o32, o64 = oracle_pair((B, hw, "mixed"), unet_sd, c, row_w=row_w)
    dv = [v.to(nm[1].device) for v in (c.x, c.t, c.y, c.vals, c.mask)]
    eps, geom, tape = nm[1].train_forward(*dv)
    d_eps, d_geom = cotangents(c, eps, geom, row_w=row_w)
    assert bool(d_geom[1].any()) and float(d_eps[1].abs().max()) < 2.0 ** -8 * float(d_eps[0].abs().max())
    _, errs = check_dx(f"input_grad mixed B={B} {hw}x{hw}", nm[1].input_grad(tape, d_eps, d_geom), o32, o64)
    print(f"[input_grad mixed B={B} {hw}x{hw}] native per sample {[f'{e:.2e}' for e in errs]}")
    check(f"mixed magnitude B={B} {hw}x{hw}", nm[1].train_backward(tape, d_eps, d_geom), o32, o64)
