"""GPU: the VAE training step (include/dmx.h dmx_vae_train_forward / dmx_vae_train_backward) against the float64
VAE training oracle, over the shapes at which the taped forward's and the backward's plan changes, over the
cotangent edge cases and over the cotangent magnitudes its operand scales see.

Gradients use the bound of tests/test_train_oracle_f64.py through tests/test_vae_train_oracle_f64.py: with g64 /
g32 the float64 / fp32 oracle's gradients of the same case and loss, E32 = max over tensors |g32 - g64| / |g64|,
and a native tensor passes when |native - g64| / |g64| <= 8 E32 (8 E32 <= 5e-5 asserted).  A tensor whose float64
gradient is exactly zero or None must be exactly zero in what NativeModel.vae_train_backward returns.

The taped forward is held per sample by the rule of tests/test_forward_oracle_f64.py: x_recon[n] and z[n] within
8 x the fp32 oracle's own error of that sample, the scalar kl[n] within 8 x the fp32 oracle's worst sample
(relative difference), from 16 samples on the worst / median spread of x_recon and z within 2 x the oracle's; the
loss within LOSS_TOL of the float64 loss.

The native side is driven through NativeModel.vae_train_forward / vae_train_backward with the cotangents computed
in torch from the native outputs:
  d_recon = w_recon c r_n 2 (x_recon - x) / numel(x),   d_z = w_z c r_n 2 z / numel(z),   d_kl = w_kl c r_n / N,
the derivative of the oracle's loss (test_vae_train_oracle_f64.py) with row weights r_n and loss scale c — so
every scale below is exact.  A weight of 0 passes None (or, where a test says so, a tensor of zeros).

Homogeneity.  The backward is linear in the cotangents.  Every x3 operand scale is ldexpf(1, e) with e from
amax_exp of a maximum of |dY| (gn8_bwd's AbsMax for each stage's weight and data gradient); the kernels that are the
VAE's own are plain fp32 and homogeneous term by term: vae_sigmoid_bwd_kernel (d s (1 - s)), vae_tail_wgrad_kernel /
vae_tail_dgrad_kernel / vae_dec0_dgrad_kernel (fmaf chains), gn8_bwd_reduce_kernel / gn8_bwd_apply_kernel (dy =
dout GELU'(y), float and double sums, a division by the element count, dr = rstd (gamma dy - m1 - xhat m2)) and
vae_heads_bwd_kernel (g = (d_z + dzin / s) s, dmu = g + d_kl mu / hw, dlogvar = g eps std / 2 + d_kl (e^lv - 1) /
2hw).  Multiplying by a power of two commutes with every rounding short of under- or overflow, so the gradients of
c times the cotangents are c times the gradients, bit for bit (test_loss_scale).

Which kernels each class reaches: profiles/vae_train_class_kernels.txt (one rocprofv3 kernel trace of
tools/vae_train_class_trace.py).  Measured on an MI355X: DESIGN.md §6b2, "Float64 parity over the plan classes"."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_train_oracle_f64 import CAP, FACTOR, e32, is_zero, tensor_errs  # noqa: E402
from test_forward_oracle_f64 import check_rows_own, check_spread, median, spread  # noqa: E402
from test_gpu_train_classes import LOSS_TOL, SPREAD, SPREAD_MIN_B  # noqa: E402
from test_vae_train_oracle_f64 import (CLASS_SHAPES, EDGE_SHAPES, FWD_LOSS, LIVE_SHAPE, THREE_LOSS, THREE_SHAPES,  # noqa: E402
                                       kl_errs, make_case, oracle_pair, rows_pair, upper_clamp_weights, weights)

# (n, h, w): the smallest shapes that reach each decision of the taped forward and of the backward (engine.hip
# conv_plan / dec_n with prec 0, plain sources and device-scaled weights; vae_train_engine.h gn8_bwd and the tail /
# heads launches; train_engine.h wgrad / colsum).  The kernel names and template arguments are those of
# profiles/vae_train_class_kernels.txt (igemm_x3_kernel<BM, BN, EPI, ...>: EPI 0 = EPI_STATS, 1 = EPI_BIAS, 4 =
# EPI_PARTIAL, the split-K slabs).  Every class runs wgrad_x3_kernel<64 | 128, 0 | 1 | 2> and the fp32 wgrad_kernel<0>
# (enc.0, dec.0); no class reaches wgrad_kernel<1>: all six stride-2 layers have their channels on the 64 grid.
CLASSES = {
    (1, 8, 8): "maps 8/4/2/1, a 1x1 latent: GEMMs and weight gradients with M = 1 (one split, rows_per_split 16 > M), "
               "ConvT and its adjoint from a 1x1 map, the stride-2 gathers of wgrad_x3_kernel<., 1> / <., 2> on a 2x2 "
               "map (12 of 16 taps are padding), gn8_bwd with HW = 1 (one chunk), vae_dec0_dgrad_kernel and the heads "
               "kernels with one pixel, vae_tail_kernel with 64 of a block's 256 pixels",
    (5, 40, 24): "non-square, odd batch, odd maps 5x3 under 10x6: every GEMM ends in a partial row tile, gn8_bwd with "
                 "15 pixels in one chunk at the latent, 75 latent pixels over vae_dec0_dgrad_kernel's 4-pixel blocks "
                 "(the last with 3)",
    (2, 56, 48): "the workload's map widths 28/14/7 (56 / 8 = 7); a latent of 42 pixels: two heads blocks, the second "
                 "with 10 of 32 pixels; a ragged last gn8_bwd chunk on the 14x12 maps (168 pixels = 10 x 16 + 8)",
    (17, 16, 16): "16 or more samples, for the spread rule; two-level colsum (17 x 256 rows > 256); the shape of the "
                  "single-live-sample test",
    (17, 32, 32): "gn8_bwd chunks limited by cdiv(512, 17) = 31 with a ragged last chunk (1024 pixels = 30 x 34 + 4), "
                  "vae_tail_wgrad_kernel at its 1024-block cap with 17 pixels per block, weight-gradient splits that "
                  "do not divide M",
    (64, 16, 16): "the class of 64 or more samples (dec_n = 128): 128-row tiles (tiles128 >= 256) in enc.0 "
                  "(igemm_f32_kernel<128, 64>), in dec.15 (igemm_x3_kernel<128, 64, EPI_STATS>) and in enc.3's data "
                  "gradient (the 4-phase ConvT GEMM, igemm_x3_kernel<128, 64, EPI_BIAS>), gn8_bwd chunks = cdiv(512, 64) "
                  "= 8",
    (65, 8, 8): "the same class, ragged, on 8/4/2/1 maps: no layer reaches 256 tiles, so dec_n = 128 decides the split "
                "counts of the 64-row kernels only (the trace shows the small classes' instances); M = 65 on the 1x1 "
                "maps, a second row tile that holds one sample; vae_train_kl_kernel's second block (n > 64)",
    (64, 32, 32): "the benchmarked step's plan for its large layers: unsplit 128-row x3 GEMMs with EPI_STATS for "
                  "conv4x4 s2 (enc.3), conv3x3 (enc.6, dec.12) and ConvT (dec.9, dec.15) — igemm_x3_kernel<128, 64, 0> x "
                  "3 and the 8-wave <128, 128, 0> x 2 — beside the split-K ones, seven unsplit data gradients (<128, 64, "
                  "1> x 3, <128, 128, 1> x 2, <64, 128, 1> x 2) beside split ones, the fp32 wgrad_kernel<0> and the tail "
                  "weight gradient at 1024 blocks of 64 pixels",
    (1, 128, 128): "one sample on large maps: gn8_bwd at its 512-chunk cap and 64 apply chunks, 8 heads blocks",
}
assert list(CLASSES) == CLASS_SHAPES
SCALES = [-24, -12, 12, 24]
IDS = lambda s: "x".join(str(v) for v in s)  # noqa: E731


@pytest.fixture(scope="module")
def sd0():
    return weights()


def _native(sd, dev):
    from models.vae import VAE
    v = VAE()
    v.load_state_dict(sd)
    v.to(dev).train()
    return v, v.native()


@pytest.fixture(scope="module")
def nm(cuda, sd0):
    return _native(sd0, cuda)


def cotangents(c, x_recon, z, w_recon=1.0, w_z=0.0, w_kl=1e-6, row_w=None, scale=1.0, zeros=False):
    """The loss's derivative at the native outputs (the module docstring's formulas), on the device.  A weight
    of 0: None, or a tensor of zeros with zeros=True."""
    dev = x_recon.device
    r = torch.ones(c.n, device=dev) if row_w is None else row_w.to(dev)
    d_recon = (w_recon * scale) * r.view(-1, 1, 1, 1) * 2.0 * (x_recon - c.x.to(dev)) / x_recon.numel()
    d_z = (w_z * scale) * r.view(-1, 1, 1, 1) * 2.0 * z / z.numel()
    d_kl = (w_kl * scale) * r / c.n
    return tuple(d if (w != 0.0 or zeros) else None for d, w in ((d_recon, w_recon), (d_z, w_z), (d_kl, w_kl)))


def native_loss(c, x_recon, z, kl, w_recon=1.0, w_z=0.0, w_kl=1e-6):
    x_recon, z, kl = (v.double().cpu() for v in (x_recon, z, kl))
    return (w_recon * float(((x_recon - c.x.double()) ** 2).mean()) + w_z * float((z ** 2).mean())
            + w_kl * float(kl.mean()))


def forward(model, c):
    dev = model.device
    return model.vae_train_forward(c.x.to(dev), c.eps.to(dev))


def run(model, c, zeros=False, **kw):
    """Taped forward and backward of case c -> (grads, x_recon, z, kl, cotangents)."""
    x_recon, z, kl, tape = forward(model, c)
    cot = cotangents(c, x_recon, z, zeros=zeros, **kw)
    return model.vae_train_backward(tape, *cot), x_recon, z, kl, cot


def check(what, grads, o32, o64, scale=1.0):
    """The module docstring's gradient bound, per tensor; prints E32, the worst five and their ratio to E32."""
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


def check_forward(what, x_recon, z, o32, o64):
    """The module docstring's per-sample bound and spread rule for x_recon and z."""
    for name, got, r32, r64 in (("x_recon", x_recon, o32.x_recon, o64.x_recon), ("z", z, o32.z, o64.z)):
        own, errs = check_rows_own(f"{what} {name}", got, r32, r64)
        check_spread(f"{what} {name}", own, errs)


def check_kl(what, kl, o32, o64):
    """The module docstring's bound for the scalar kl[n]: the relative difference within FACTOR x the fp32
    oracle's worst sample."""
    assert bool(torch.isfinite(kl).all())
    own, errs = kl_errs(o32.kl, o64.kl), kl_errs(kl, o64.kl)
    E = max(own)
    print(f"[{what} kl] per sample: E32 worst {E:.2e}; native worst {max(errs):.2e} ({max(errs) / E:.2f} E32, "
          f"sample {errs.index(max(errs))})")
    assert FACTOR * E <= CAP, E
    bad = [(n, e) for n, e in enumerate(errs) if not e <= FACTOR * E]
    assert bad == [], (what, E, bad[:5])


# ---- the plan classes -----------------------------------------------------------------------------------
_CASES = [(s, "fwd") for s in CLASSES] + [(s, "three") for s in THREE_SHAPES]
_FWD = {}


def class_forward(model, shape):
    """The taped forward's outputs of a class, once (the forward does not depend on the loss)."""
    if shape not in _FWD:
        _FWD[shape] = forward(model, make_case(*shape))[:3]
    return _FWD[shape]


@pytest.mark.parametrize("shape,loss", _CASES, ids=[f"{IDS(s)}-{l}" for s, l in _CASES])
def test_plan_class(nm, sd0, shape, loss):
    """The gradients and the loss.  CLASSES says which decision each shape is there for.  fwd: VAE.forward's loss,
    weights (1, 0, 1e-6), d_z absent; three: (1, 0.3, 0.5), all three cotangents at O(1) weights."""
    kw = FWD_LOSS if loss == "fwd" else THREE_LOSS
    c = make_case(*shape)
    o32, o64 = oracle_pair((shape, loss), sd0, c, **kw)
    grads, x_recon, z, kl, _ = run(nm[1], c, **kw)
    _FWD.setdefault(shape, (x_recon, z, kl))
    got = native_loss(c, x_recon, z, kl, **kw)
    print(f"[class {shape} {loss}] loss {got:.8e}, float64 {float(o64.loss):.8e}")
    assert abs(got - float(o64.loss)) <= LOSS_TOL * float(o64.loss), (got, float(o64.loss))
    check(f"class {shape} {loss}", grads, o32, o64)


@pytest.mark.parametrize("shape", list(CLASSES), ids=IDS)
def test_plan_class_forward(nm, sd0, shape):
    """The taped forward's x_recon and z of every class, per sample, and their spread from 16 samples on."""
    o32, o64 = oracle_pair((shape, "fwd"), sd0, make_case(*shape), **FWD_LOSS)
    x_recon, z, _ = class_forward(nm[1], shape)
    check_forward(f"class {shape}", x_recon, z, o32, o64)


@pytest.mark.parametrize("shape", list(CLASSES), ids=IDS)
def test_plan_class_kl(nm, sd0, shape):
    """The taped forward's per-sample KL of every class: each kl[n] within 8 x the fp32 oracle's worst sample.

    The finding of this file: at (1, 128, 128) the batch has one sample, so the noise estimate is
    one draw of one fp32 scalar's rounding, and where the fp32 oracle's kl is the float64 value's nearest fp32
    number (9.47e-9 from it, bound 7.6e-8) the native kl, summed in fp32 by vae_train_heads_kernel /
    vae_enc_kl_kernel, was the next fp32 number: 1.22e-7, 12.9 E32.  The training forward now takes the KL terms
    and their sums in double and rounds once (vae_train_kl_kernel): kl[n] is the nearest fp32 number to its own
    double sum, which no fp32 oracle can beat by more than the heads' own error."""
    o32, o64 = oracle_pair((shape, "fwd"), sd0, make_case(*shape), **FWD_LOSS)
    check_kl(f"class {shape}", class_forward(nm[1], shape)[2], o32, o64)


def test_kl_is_rounded_once(nm, sd0):
    """The directed pin of test_plan_class_kl's finding, without a tolerance: at (1, 128, 128) the native kl[0] is
    the float64 oracle's kl rounded to fp32, bit for bit.  The float64 value lies 9.5e-9 (relative) from that fp32
    number and 5e-8 from the tie with its neighbour; the native double sum differs from it by the x3 error of mu /
    logvar averaged over 1024 terms (1e-8), so a KL summed in double lands on it; the fp32 tree of before landed
    on the neighbour (1.22e-7 off)."""
    shape = (1, 128, 128)
    _, o64 = oracle_pair((shape, "fwd"), sd0, make_case(*shape), **FWD_LOSS)
    kl = class_forward(nm[1], shape)[2]
    want = o64.kl.float()
    print(f"[kl rounded once] native {float(kl[0]):.9e}, float64 {float(o64.kl[0]):.12e}, its fp32 rounding "
          f"{float(want[0]):.9e}")
    assert torch.equal(kl.cpu(), want)


# ---- cotangent edge cases -------------------------------------------------------------------------------
ONLY = {"d_recon": dict(w_recon=1.0, w_z=0.0, w_kl=0.0), "d_z": dict(w_recon=0.0, w_z=0.3, w_kl=0.0),
        "d_kl": dict(w_recon=0.0, w_z=0.0, w_kl=0.5)}


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=IDS)
@pytest.mark.parametrize("only", list(ONLY))
def test_single_cotangent(nm, sd0, shape, only):
    """One cotangent alone, the others None: within the bound of that loss's oracle.  d_z only and d_kl only do not
    reach the decoder: max|dY| = 0 is every decoder stage's scale (amax_exp's zero case) and every dec.* gradient
    is exactly zero.  The same run with tensors of zeros in place of None gives the same bits."""
    c = make_case(*shape)
    o32, o64 = oracle_pair((shape, only), sd0, c, **ONLY[only])
    grads, _, _, _, cot = run(nm[1], c, **ONLY[only])
    assert [d is None for d in cot] == [k != only for k in ONLY]
    check(f"{only} only {shape}", grads, o32, o64)
    dec = [n for n in grads if n.startswith("dec.")]
    assert len(dec) == 26
    if only != "d_recon":
        assert all(is_zero(o64.grads[n]) for n in dec) and not any(bool(grads[n].any()) for n in dec)
    else:
        assert not any(is_zero(o64.grads[n]) for n in dec)
    gz, _, _, _, cz = run(nm[1], c, zeros=True, **ONLY[only])
    assert all(d is not None for d in cz) and sum(bool(d.any()) for d in cz) == 1
    assert [n for n in grads if not torch.equal(gz[n], grads[n])] == []


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=IDS)
def test_no_cotangent(nm, shape):
    """All three cotangents absent, and all three tensors of zeros: every gradient is exactly zero (and finite)."""
    c = make_case(*shape)
    for zeros in (False, True):
        grads, _, _, _, cot = run(nm[1], c, zeros=zeros, w_recon=0.0, w_z=0.0, w_kl=0.0)
        assert all((d is not None and not bool(d.any())) if zeros else d is None for d in cot)
        for n, g in grads.items():
            assert bool(torch.isfinite(g).all()) and not bool(g.any()), n


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=IDS)
@pytest.mark.parametrize("rows", ["zero row", "mixed"])
def test_row_weights(nm, sd0, shape, rows):
    """zero row: the last sample's cotangents are zero.  mixed: row weights 1, 2^-10, 1 — one sample's cotangents
    2^-10 of its neighbours' under the one per-tensor power-of-two scale of every stage (an element keeps a
    normal f16 lo part down to 2^-16 of the tensor's largest)."""
    c = make_case(*shape)
    r = torch.ones(c.n)
    r[-1 if rows == "zero row" else 1] = 0.0 if rows == "zero row" else 2.0 ** -10
    o32, o64 = oracle_pair((shape, rows), sd0, c, row_w=r, **THREE_LOSS)
    grads, _, _, _, cot = run(nm[1], c, row_w=r, **THREE_LOSS)
    if rows == "zero row":
        assert all(not bool(d[-1].any()) and bool(d[0].any()) for d in cot)
    else:
        assert float(cot[0][1].abs().max()) < 2.0 ** -8 * float(cot[0][0].abs().max()) and bool(cot[0][1].any())
    check(f"{rows} {shape}", grads, o32, o64)


# ---- loss scales ----------------------------------------------------------------------------------------
_BASE = {}


def base_run(model, c, shape):
    """The unscaled three-cotangent run of a shape, once (two runs give the same bits:
    tests/test_gpu_vae_train.py test_step_is_deterministic)."""
    if shape not in _BASE:
        grads, _, _, _, cot = run(model, c, **THREE_LOSS)
        _BASE[shape] = (grads, cot)
    return _BASE[shape]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=IDS)
@pytest.mark.parametrize("k", SCALES)
def test_loss_scale(nm, sd0, shape, k):
    """All three cotangents times c = 2^k: (a) the gradients meet the bound against c g64, (b) times 1 / c they
    equal the unscaled run's bit for bit (the module docstring's homogeneity property)."""
    c, s = make_case(*shape), 2.0 ** k
    o32, o64 = oracle_pair((shape, "three"), sd0, c, **THREE_LOSS)
    base, cot1 = base_run(nm[1], c, shape)
    grads, _, _, _, cots = run(nm[1], c, scale=s, **THREE_LOSS)
    assert all(torch.equal(a * (1.0 / s), b) for a, b in zip(cots, cot1))
    check(f"loss scale 2^{k} {shape}", grads, o32, o64, scale=s)                           # (a)
    differ = [n for n in base if not torch.equal(grads[n] * (1.0 / s), base[n])]          # (b)
    assert differ == [], differ


# ---- one live sample ------------------------------------------------------------------------------------
def test_single_live_sample(nm, sd0):
    """LIVE_SHAPE, one backward per sample with only that sample's cotangents non-zero (one tape: the backward only
    reads it), against the float64 gradient of that sample's loss term: each sample within 8 x its own E32 (the
    maximum over tensors), and the samples' worst / median within 2 x the fp32 oracle's.  The VAE returns no input
    gradient; this is its stand-in for the U-Net's per-sample d_x check: one sample at several times its neighbours
    is a defect in what only that sample's values reach."""
    c = make_case(*LIVE_SHAPE)
    r32, r64 = rows_pair((LIVE_SHAPE, "fwd"), sd0, c, **FWD_LOSS)
    x_recon, z, kl, tape = forward(nm[1], c)
    own, errs = [], []
    for n in range(c.n):
        r = torch.zeros(c.n)
        r[n] = 1.0
        grads = nm[1].vae_train_backward(tape, *cotangents(c, x_recon, z, row_w=r, **FWD_LOSS))
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        own.append(e32(r32[n], r64[n]))
        errs.append(tensor_errs(grads, r64[n])[0])
    ratio = [e[0] / o for e, o in zip(errs, own)]
    w = max(range(c.n), key=lambda n: ratio[n])
    nat = [e[0] for e in errs]
    print(f"[single live sample {LIVE_SHAPE}] E32 per sample {min(own):.2e} .. {max(own):.2e} (median {median(own):.2e}); "
          f"native {min(nat):.2e} .. {max(nat):.2e}; worst ratio to its own E32 {ratio[w]:.2f} (sample {w}, "
          f"{errs[w][1]}); spread worst / median: native {spread(nat):.2f}, fp32 oracle {spread(own):.2f}")
    assert FACTOR * max(own) <= CAP
    assert [(n, nat[n], own[n]) for n in range(c.n) if not nat[n] <= FACTOR * own[n]] == []
    assert c.n >= SPREAD_MIN_B and spread(nat) <= SPREAD * spread(own), (spread(nat), spread(own))


# ---- the upper clamp ------------------------------------------------------------------------------------
def test_upper_clamp_gradient(cuda):
    """to_logvar.bias = 40 on channel 2 (the value test_vae_train_oracle_f64.test_upper_clamp_case holds the cap
    with): the unclamped logvar exceeds 20 everywhere on it, so that channel's rows of to_logvar.weight / .bias are
    exactly zero where the oracle's are; std = e^10 on that channel reaches z and the decoder; everything finite
    and within the bound.  (The lower clamp: tests/test_gpu_vae_train.py test_clamp_gradient.)"""
    sd, c = upper_clamp_weights(), make_case(2, 32, 32)
    o32, o64 = oracle_pair(((2, 32, 32), "upper clamp"), sd, c, **THREE_LOSS)
    _, model = _native(sd, cuda)
    grads, x_recon, z, kl, _ = run(model, c, **THREE_LOSS)
    for k in ("to_logvar.weight", "to_logvar.bias"):
        assert float(o64.grads[k][2].abs().max()) == 0.0 and float(grads[k][2].abs().max()) == 0.0, k
        assert bool(grads[k][[0, 1, 3]].any())
    assert all(bool(torch.isfinite(v).all()) for v in (x_recon, z, kl))
    got = native_loss(c, x_recon, z, kl, **THREE_LOSS)
    assert abs(got - float(o64.loss)) <= LOSS_TOL * float(o64.loss), (got, float(o64.loss))
    check("upper clamp (2, 32, 32)", grads, o32, o64)
