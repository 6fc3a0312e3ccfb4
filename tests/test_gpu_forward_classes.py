"""GPU: the inference forward (include/dmx.h dmx_unet_forward, NativeModel.forward) against the float64
forward oracle, per sample, over the shapes at which its conv plan changes (engine.hip conv_plan / dec_n)
and in every GEMM arithmetic; and the layer taps (NativeModel.forward_taps) against oracle/taps.py in
float64.

The bounds are those of tests/test_forward_oracle_f64.py (its docstring states and argues them):
  eps    each sample within 8 x its own E32, E32 the fp32 oracle's error of that sample against float64;
  geom   each row within 8 x the fp32 oracle's worst row;  taps: each sample within 8 x the fp32 oracle's
         worst sample of that tap;  8 x the worst E32 <= 5e-5 asserted everywhere;
  spread from 16 samples on, worst / median of the native per-sample errors <= 2 x the fp32 oracle's.
They apply to the production plan (test_forward_class) and to the materialised plan the taps run
(test_taps_class: with the debug taps on, resblock() turns off GroupNorm-on-load, plane outputs, deferred
norms and the fused split-K reduce, so forward_taps' eps is a second route to the same numbers).
The fp16-operand mode has no reference of its own arithmetic: test_forward_class_f16 holds each sample
and each geom row to test_gpu_f16.py's stated TOL_FWD and reports the spread without asserting it.

Which kernel a shape reaches is guarded on the labels of NativeModel.step_profile
(test_class_reaches_its_kernels).  Measured on an MI355X: DESIGN.md §6, "Float64 parity of the inference
forward over the plan classes"."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_forward_oracle_f64 import (CASES, TAP_CASES, check_rows_own, check_rows_worst, check_spread,  # noqa: E402
                                     forward_pair, make_case, median, rel_l2, row_errs, spread, taps_pair)
from test_gpu_f16 import TOL_FWD  # noqa: E402
from test_gpu_kernel_plan import record_plan  # noqa: E402

# (B, H = W): the smallest shapes that reach each decision of the inference forward's plan
CLASSES = {
    (1, 8): "maps 8/4/2/1: attention at L = 1, W < 16 so inc's first conv leaves conv_in_kernel, "
            "igemm_halo_cs_kernel with one sample in a 256-pixel tile",
    (2, 12): "maps 12/6/3/1: the one-sided Up pad at 1->2 into 3",
    (3, 16): "both igemm_halo_cs_kernel widths (8 and 4); attention16_kernel<8>",
    (5, 20): "conv_in_kernel<16>; L = 400/100/25/4 (no multiple of 64 or 16); ragged batch",
    (3, 36): "W > 32: the general input conv; L = 1296",
    (5, 32): "the small class at the workload's width: split-K x3 GEMMs with splitk_reduce_kernel; "
             "attention16_kernel<16>",
    (34, 32): "the 32..63-sample class: igemm_halo_kernel<64, .., 32, GNA> at up3.0, GNA 0 and 1",
    (42, 40): "maps wider than 32 with cdiv(N 1600, 256) >= 256 and a plane source: igemm_pp_kernel, its last "
              "256-row tile half empty",
    (64, 16): "the >= 64-sample class (dec_n = 128) in the 16-, 8- and 4-wide Winograd geometries; a 2 x 2 map "
              "in the 4-wide geometry",
    (65, 8): "the same class, ragged: the last Winograd block holds one sample",
    (64, 20): "20/10/5/2 maps in the 32/16/8/4 geometries, with bands",
    (66, 28): "the 28-wide path (28/14/7/3 maps, zero-padded rows and columns), ragged",
    (64, 32): "the benchmark's class, per sample",
}
assert list(CLASSES) == CASES
IDS = [f"{b}x{h}" for b, h in CASES]
TAP_IDS = [f"{b}x{h}" for b, h in TAP_CASES]
# oracle taps the native forward does not materialise in the split-precision modes (the fused token
# kernels keep the first LayerNorm's output in registers); the fp32 mode taps every name
NOT_TAPPED = {"x3": {f"sa{i}.xl" for i in range(1, 7)}, "fp32": set()}


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(unet_sd)
    return m.to(cuda).eval()


@pytest.fixture(params=["x3", "fp32"])
def prec(request, model):
    nm = model.native()
    old = nm.precision
    nm.set_precision(request.param)
    yield request.param
    nm.set_precision(old)


def inputs(c, dev):
    return [v.to(dev) for v in (c.x, c.t, c.y, c.vals, c.mask)]


@pytest.mark.parametrize("B,hw", CASES, ids=IDS)
def test_forward_class(model, unet_sd, cuda, prec, B, hw):
    """CLASSES says which decision each shape is there for.  In order: finite, eps per sample, geom per row,
    the spread from 16 samples on."""
    c = make_case(B, hw)
    (e32, g32), (e64, g64) = forward_pair((B, hw), unet_sd, c)
    with torch.no_grad():
        eps, geom = model.native().forward(*inputs(c, cuda), want_geom=True)
    what = f"forward {prec} B={B} {hw}x{hw}"
    assert bool(torch.isfinite(eps).all()) and bool(torch.isfinite(geom).all())
    own, errs = check_rows_own(f"{what} eps", eps, e32, e64)
    check_rows_worst(f"{what} geom", geom, g32, g64)
    check_spread(f"{what} eps", own, errs)


# (65, 8) in the fp16-operand mode: the worst of the 65 samples stands at 2.09e-3 against TOL_FWD = 2e-3
# (sample 11; median 1.21e-3).  Cause: batches of >= 64 samples run the 3x3 convs as Winograd
# F(2x2, 3x3), whose fp16 instance rounds the transformed operands to fp16; one such conv carries 1.4 .. 2.0
# times the rounding of the direct fp16 conv of the small-batch class (4.1e-4 .. 5.7e-4 against 2.8e-4 ..
# 3.1e-4 on the same inputs, every sample alike; 1.00 on the 1 x 1 maps, which run one kernel in both classes;
# 0.84 .. 1.19 in x3, whose transformed operands keep hi and lo).  The same 65 samples in batches of 13 stand
# at 1.21e-3 worst, 7.7e-4 median (test_f16_open_case_by_the_small_batch_route).  That is the arithmetic of
# the mode, not a defect of a launch; the bound stays and only the per-sample eps assertion of this case is
# expected to fail: everything else below is asserted for it too.
F16_OPEN = {(65, 8): "fp16 Winograd class at 8 x 8: worst sample 2.09e-3 > TOL_FWD 2e-3 (DESIGN.md §6v)"}


@pytest.mark.parametrize("B,hw", CASES, ids=IDS)
def test_forward_class_f16(model, unet_sd, cuda, record_property, B, hw):
    """The fp16-operand mode (BASELINE config 4).  Asserted for every case: finite outputs; each geom row
    within TOL_FWD of the float64 oracle; the whole batch's eps within TOL_FWD (the bound as test_gpu_f16.py
    states it); each sample's eps within TOL_FWD x the fp32 oracle's own worst / median of that batch (the
    gross-error guard: TOL_FWD was stated for a batch, and the worst of B draws stands above their middle by
    what the oracle's own draws show, 1.0 .. 1.63 here; the lost key mask stood 40 times above it); the mode
    is applied.  Then each sample's eps within TOL_FWD itself, the one assertion a case of F16_OPEN is expected
    to fail (strictly: such a case inside the bound fails the test, so the entry cannot outlive its reason).
    The spread is printed and recorded, not asserted (no fp16-operand reference exists to hold it against)."""
    c = make_case(B, hw)
    (e32, _), (e64, g64) = forward_pair((B, hw), unet_sd, c)
    with model.native().precision_override("f16"), torch.no_grad():
        eps, geom = model.native().forward(*inputs(c, cuda), want_geom=True)
    assert bool(torch.isfinite(eps).all()) and bool(torch.isfinite(geom).all())
    errs, gerrs, own = row_errs(eps, e64), row_errs(geom, g64), row_errs(e32, e64)
    batch = rel_l2(eps, e64)
    line = (f"eps batch {batch:.2e}, worst sample {max(errs):.2e} (sample {errs.index(max(errs))}) median "
            f"{median(errs):.2e}, geom worst row {max(gerrs):.2e}")
    if B >= 16:
        line += f", spread native {spread(errs):.2f} / fp32 oracle {spread(own):.2f}"
        record_property("spread", spread(errs))
    print(f"[forward f16 B={B} {hw}x{hw}] {line}")
    record_property("eps_worst", max(errs))
    assert max(gerrs) <= TOL_FWD and batch <= TOL_FWD, line
    assert max(errs) <= TOL_FWD * spread(own), line
    assert max(errs) > 1e-6, "f16 mode should not be fp32-exact (is the mode applied?)"
    if (B, hw) in F16_OPEN:
        assert max(errs) > TOL_FWD, f"within the bound now: take {(B, hw)} out of F16_OPEN ({line})"
        pytest.xfail(F16_OPEN[(B, hw)] + ": " + line)
    assert max(errs) <= TOL_FWD, line


def test_f16_open_case_by_the_small_batch_route(model, unet_sd, cuda):
    """The 65 samples of F16_OPEN's case in five batches of 13, which run the direct fp16 convs
    (igemm_halo_cs_kernel at 8 x 8 and 4 x 4) instead of the Winograd ones: every sample's eps and every geom
    row within TOL_FWD (measured: worst sample 1.21e-3, median 7.7e-4).  Together with the case itself this
    pins where its excess comes from."""
    B, hw = 65, 8
    assert (B, hw) in F16_OPEN
    c = make_case(B, hw)
    _, (e64, g64) = forward_pair((B, hw), unet_sd, c)
    outs = []
    with model.native().precision_override("f16"), torch.no_grad():
        for s in range(0, B, 13):
            outs.append(model.native().forward(*(v[s:s + 13] for v in inputs(c, cuda)), want_geom=True))
    eps, geom = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    errs, gerrs = row_errs(eps, e64), row_errs(geom, g64)
    print(f"[forward f16 B=65 8x8 as 5 x 13] eps worst sample {max(errs):.2e} median {median(errs):.2e}, geom worst "
          f"row {max(gerrs):.2e}")
    assert max(errs) <= TOL_FWD and max(gerrs) <= TOL_FWD


@pytest.mark.parametrize("B,hw", TAP_CASES, ids=TAP_IDS)
def test_taps_class(model, unet_sd, cuda, prec, B, hw):
    """forward_taps against oracle/taps.py in float64: every tap the oracle names, per sample, within 8 x the
    fp32 oracle's worst sample of that tap, the spread per tap from 16 samples on; the eps of this
    materialised plan within the production eps' per-sample bound; the taps without an oracle counterpart
    (.ao, .av, the second ResBlocks' .r1) finite.  The native forward materialises no .xl in the
    split-precision modes (NOT_TAPPED): exactly those names may be missing."""
    c = make_case(B, hw)
    t32, t64 = taps_pair((B, hw), unet_sd, c)
    with torch.no_grad():
        nat = model.native().forward_taps(*inputs(c, cuda))
    assert set(t64) - set(nat) == NOT_TAPPED[prec], sorted(set(t64) - set(nat))
    what = f"taps {prec} B={B} {hw}x{hw}"
    worst = (0.0, None)
    for k, v in nat.items():
        assert bool(torch.isfinite(v).all()), k
        if k == "eps" or k not in t64:
            continue
        assert v.numel() == t64[k].numel(), (k, v.numel(), t64[k].numel())
        own, errs = check_rows_worst(f"{what} {k}", v.reshape(B, -1), t32[k], t64[k])
        check_spread(f"{what} {k}", own, errs)
        worst = max(worst, (max(errs) / max(own), k))
    print(f"[{what}] worst tap {worst[1]}: {worst[0]:.2f} x its E32")
    own, errs = check_rows_own(f"{what} eps", nat["eps"].reshape(B, -1), t32["eps"], t64["eps"])
    check_spread(f"{what} eps", own, errs)


# ---- the finding: the key mask of attention16_kernel's fp16 instance on maps of fewer than 32 tokens -----
@pytest.mark.parametrize("hw", [8, 10])
@pytest.mark.parametrize("mode", ["f16", "x3"])
def test_attention16_masks_the_keys_past_a_short_map(model, cuda, mode, hw):
    """Found through test_forward_class_f16 at (1, 8) and (65, 8): every sample's eps 8e-2 .. 1.7e-1 off in
    the fp16-operand mode, 5e-7 in the others.  The f16 taps put it at sa5, the one block whose head-
    resident core (igemm_x3.h attention16_kernel, D = 16) sees L = 16 < 32 keys: sa5.qkv stood at 1.0e-3,
    sa5 at 1.4e-1.  Cause: the kernel's first QK^T MFMA of a chunk was an inline-asm instruction
    (mfma_untied).  In the split-precision instance its result feeds the next MFMA as C, which needs no wait
    states; in the fp16 instance the VALU reads it next, and nothing pads an MFMA inside an asm string.
    With L < 32 the first chunk is the ragged one, whose -inf masking of the keys >= L came directly after
    the MFMA and was overwritten when the MFMA's result landed: the 32 - L padding keys (zero K rows, score
    0) entered the softmax denominator.  (A ragged chunk later in the key loop has the mask compares between
    the MFMA and the masking, which happened to be wait states enough.)  The fp16 instance now uses the
    builtin, which the compiler pads.

    Here: the attention core alone, at 8 x 8 (sa5 L = 16, sa6 L = 64) and 10 x 10 (L = 25, 100).  The native
    .ao tap against float64 softmax(q k^T / 4) v of the native .qkv tap, per (sample, head): the x3 mode
    within 1e-5 (the bound and the argument of test_attention_query_split_at_an_f16_tie), the fp16 mode within
    test_gpu_f16.py's TOL_FWD (q, k, v and the weights are each rounded to fp16, 2^-11 = 4.9e-4).  Measured
    after the fix: x3 8e-8 .. 1.3e-7, fp16 7e-5 .. 1.5e-4; the lost mask stood at 1e-1 and more.  These two
    bounds pin this defect (a mask, a key or a chunk lost); they stand 80 and 13 times above the measured
    figures and are no parity bound of the attention core, which test_forward_class and test_taps_class hold
    through sa5 / sa6 and eps."""
    B = 2
    c = make_case(B, hw)
    with model.native().precision_override(mode), torch.no_grad():
        nat = model.native().forward_taps(*inputs(c, cuda))
    for name, L in (("sa5", (hw // 2) ** 2), ("sa6", hw * hw)):
        qkv = nat[name + ".qkv"].double().cpu().reshape(B, L, 3, 4, 16)      # [n][token][q k v][head][d]
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))           # (B, 4, L, 16)
        want = torch.softmax(q @ k.transpose(-1, -2) / 4.0, dim=-1) @ v
        got = nat[name + ".ao"].double().cpu().reshape(B, L, 4, 16).transpose(1, 2)
        errs = (got - want).flatten(2).norm(dim=-1) / want.flatten(2).norm(dim=-1)
        print(f"[attention16 {mode} {hw}x{hw}] {name} L = {L}: (sample, head) rel-L2 worst {float(errs.max()):.2e}")
        assert float(errs.max()) <= (TOL_FWD if mode == "f16" else 1e-5), (name, errs)


def labels_of(model, cuda, prec, B, hw):
    import diff
    return record_plan(model, diff.Diffuser(1000, device=cuda), prec, B, hw, cuda)


@pytest.mark.parametrize("mode", ["x3", "f16"])
def test_class_reaches_its_kernels(model, cuda, mode):
    """A shape must not silently stop covering its kernel after a plan change.  The labels are those of one
    eager CFG step (NativeModel.step_profile) at B = N / 2, whose trunk runs 2 B = N samples.  This is
    indirect: the step's shared prefix (inc, down1's ResBlocks) runs B samples where a forward of N runs N,
    so only launches below that prefix are asserted (up3.0 and the Winograd geometries are; the igemm_pp
    launches counted are the up path's)."""
    x1 = 1 if mode == "f16" else 0
    lab = labels_of(model, cuda, mode, 17, 32)                                    # (34, 32)
    up30 = [k for k, layer in lab if layer == "up3.0" and k.startswith("igemm_halo_kernel<64, ")]
    assert any(k.endswith(f", {x1}, 32, 0>") for k in up30) and any(k.endswith(f", {x1}, 32, 1>") for k in up30), \
        [k for k, layer in lab if layer == "up3.0"]
    lab = labels_of(model, cuda, mode, 21, 40)                                    # (42, 40)
    pp = [(k, layer) for k, layer in lab if k.startswith("igemm_pp_kernel<") and layer.startswith("up3.")]
    assert pp and all(k.endswith(f", 1, {x1}>") for k, _ in pp), sorted({(k, layer) for k, layer in lab
                                                                          if layer.startswith("up3.")})
    lab = labels_of(model, cuda, mode, 32, 16)                                    # (64, 16)
    for g in (16, 8, 4):
        assert any(k.startswith(f"wino_kernel<{g}, ") for k, _ in lab), g
