"""The float64 mode of the forward oracle (oracle/train_ref.py forward, oracle/taps.py) and the per-sample
bounds the GPU inference-forward tests derive from it.  CPU only; tests/test_gpu_forward_classes.py imports
the helpers.  The case builder, the error measures and FACTOR / CAP are those of test_train_oracle_f64.py.

With e64 / e32 the float64 / fp32 oracle's eps of one case (no code under test in either):

  own[n] = |e32[n] - e64[n]| / |e64[n]|     the fp32 oracle's rounding noise of sample n (E32 per sample)

eps     a native sample passes when |eps[n] - e64[n]| / |e64[n]| <= FACTOR own[n], FACTOR = 8 = 4 x 2 (the
        split carries a product to 2^-22 where fp32 carries 2^-24; a different, fixed summation order).
        FACTOR max(own) <= CAP is asserted so that a noisy reference cannot open the bound.
geom    12 numbers per row: one row's own error is too few draws to bound anything, so a native row passes
        within FACTOR x the batch's worst geom row of the fp32 oracle (same cap).
taps    a tap's sample passes within FACTOR x the fp32 oracle's worst sample of that tap (same cap).
spread  from SPREAD_MIN_B samples on: worst / median of the native per-sample errors <= SPREAD x worst /
        median of the fp32 oracle's (the rule and the argument of test_gpu_train_classes.py check_dx: the
        samples of a batch go through the same launches, so their errors are draws of one distribution).

Measured here (16 threads), per-sample eps E32 worst / median, geom worst row: test_cap_and_spread prints
them; DESIGN.md §6, "Float64 parity of the inference forward over the plan classes", tabulates them."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_train_oracle_f64 import CAP, F64_VS_F32, FACTOR, make_case, rel_l2, row_errs, threads, weights  # noqa: E402
from oracle import ref, train_ref  # noqa: E402
from oracle.taps import oracle_taps  # noqa: E402

SPREAD_MIN_B = 16  # batches from which a median over the samples means something
SPREAD = 2.0

# (B, H = W) of the GPU module's plan classes (its CLASSES dict says what each is there for)
CASES = [(1, 8), (2, 12), (3, 16), (5, 20), (3, 36), (5, 32), (34, 32), (42, 40), (64, 16), (65, 8), (64, 20),
         (66, 28), (64, 32)]
TAP_CASES = [(1, 8), (5, 20), (34, 32), (64, 16), (66, 28)]
# the shapes the bound was first measured at that are no GPU case
CPU_ONLY_CASES = [(32, 32), (64, 28)]

_PAIR, _TAPS = {}, {}


def forward_pair(key, sd, c):
    """((eps32, geom32), (eps64, geom64)) of oracle/train_ref.py forward on one case, under no_grad, computed
    once per key and not modified."""
    if key not in _PAIR:
        threads()
        with torch.no_grad():
            _PAIR[key] = tuple(train_ref.forward(sd, c.x, c.t, c.y, c.vals, c.mask, dtype=d)
                               for d in (torch.float32, torch.float64))
    return _PAIR[key]


def taps_pair(key, sd, c):
    """(fp32 taps, float64 taps) of oracle/taps.py on one case, each {name: (B, -1) tensor}, once per key."""
    if key not in _TAPS:
        threads()
        out = []
        with torch.no_grad():
            for d in (torch.float32, torch.float64):
                w = {k: v.to(d) for k, v in sd.items()}
                T = oracle_taps(w, c.x.to(d), c.t, c.y, c.vals.to(d), c.mask.to(d))
                out.append({k: v.reshape(c.B, -1) for k, v in T.items()})
        _TAPS[key] = tuple(out)
    return _TAPS[key]


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    """Worst / median of a list of per-sample errors."""
    return max(v) / median(v)


def check_rows_own(what, got, r32, r64):
    """The eps bound: every sample within FACTOR x its own E32 -> (own, errs)."""
    assert bool(torch.isfinite(got).all()), what
    own, errs = row_errs(r32, r64), row_errs(got, r64)
    E = max(own)
    worst = max(range(len(errs)), key=lambda n: errs[n] / own[n])
    print(f"[{what}] per sample: E32 worst {E:.2e} median {median(own):.2e}; native worst {max(errs):.2e} "
          f"({max(errs) / E:.2f} E32), worst ratio to its own E32 {errs[worst] / own[worst]:.2f} (sample {worst})")
    assert FACTOR * E <= CAP, (what, E)
    bad = [(n, errs[n], own[n]) for n in range(len(errs)) if not errs[n] <= FACTOR * own[n]]
    assert bad == [], (what, bad[:5])
    return own, errs


def check_rows_worst(what, got, r32, r64):
    """The geom / tap bound: every row within FACTOR x the fp32 oracle's worst row -> (own, errs)."""
    assert bool(torch.isfinite(got).all()), what
    own, errs = row_errs(r32, r64), row_errs(got, r64)
    E = max(own)
    print(f"[{what}] per row: E32 worst row {E:.2e}; native worst {max(errs):.2e} ({max(errs) / E:.2f} E32, "
          f"row {errs.index(max(errs))})")
    assert FACTOR * E <= CAP, (what, E)
    bad = [(n, e) for n, e in enumerate(errs) if not e <= FACTOR * E]
    assert bad == [], (what, E, bad[:5])
    return own, errs


def check_spread(what, own, errs):
    """The spread rule from SPREAD_MIN_B samples on -> (native, oracle) worst / median, or None below."""
    if len(errs) < SPREAD_MIN_B:
        return None
    s_nat, s_ref = spread(errs), spread(own)
    print(f"[{what}] spread worst / median: native {s_nat:.2f} (sample {errs.index(max(errs))}), fp32 oracle "
          f"{s_ref:.2f}")
    assert s_nat <= SPREAD * s_ref, (what, s_nat, s_ref, errs.index(max(errs)))
    return s_nat, s_ref


# ---- the CPU pins ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hw", [(2, 12), (3, 16)])
def test_float64_forward_agrees_with_fp32_oracle(B, hw):
    """forward_pair's two results are the fp32 oracle itself (bit for bit unet_cond_geom_forward) and a
    float64 run of it within F64_VS_F32."""
    sd, c = weights(), make_case(B, hw)
    (e32, g32), (e64, g64) = forward_pair((B, hw), sd, c)
    assert e32.dtype == g32.dtype == torch.float32 and e64.dtype == g64.dtype == torch.float64
    assert not e64.requires_grad and e64.shape == c.x.shape and g64.shape == (B, 12)
    with torch.no_grad():
        e, g = ref.unet_cond_geom_forward(sd, c.x, c.t, c.y, c.vals, c.mask)
    assert torch.equal(e, e32) and torch.equal(g, g32)
    assert 1e-8 < rel_l2(e32, e64) <= F64_VS_F32 and rel_l2(g32, g64) <= F64_VS_F32
    assert forward_pair((B, hw), sd, c)[1][0] is e64  # cached per key


@pytest.mark.parametrize("B,hw", CASES + CPU_ONLY_CASES, ids=lambda v: str(v))
def test_cap_and_spread(B, hw):
    """Every case: FACTOR x the worst per-sample eps E32 and FACTOR x the worst geom row stay under CAP (so
    the GPU module's bounds are tighter than CAP everywhere), and from SPREAD_MIN_B samples on the oracle's
    own worst / median is below 2: the spread rule then holds a native batch to less than 4."""
    sd, c = weights(), make_case(B, hw)
    (e32, g32), (e64, g64) = forward_pair((B, hw), sd, c)
    own, gown = row_errs(e32, e64), row_errs(g32, g64)
    print(f"[forward f64 B={B} {hw}x{hw}] eps E32 worst {max(own):.2e} median {median(own):.2e} "
          f"w/m {spread(own):.2f}; geom worst row {max(gown):.2e}")
    assert rel_l2(e32, e64) <= F64_VS_F32 and rel_l2(g32, g64) <= F64_VS_F32
    assert min(own) > 0.0 and FACTOR * max(own) <= CAP and FACTOR * max(gown) <= CAP
    if B >= SPREAD_MIN_B:
        assert spread(own) < 2.0, spread(own)


@pytest.mark.parametrize("B,hw", [(2, 12), (3, 16)])
def test_oracle_taps_end_in_the_oracle_eps(B, hw):
    """oracle/taps.py recomputes the trunk block by block: its eps is unet_cond_geom_forward's bit for bit in
    fp32, and with float64 weights and inputs it is the float64 forward's."""
    sd, c = weights(), make_case(B, hw)
    with torch.no_grad():
        T = oracle_taps(sd, c.x, c.t, c.y, c.vals, c.mask)
        e, _ = ref.unet_cond_geom_forward(sd, c.x, c.t, c.y, c.vals, c.mask)
    assert T["eps"].dtype == torch.float32 and torch.equal(T["eps"], e.flatten())
    t32, t64 = taps_pair((B, hw), sd, c)
    e64 = forward_pair((B, hw), sd, c)[1][0]
    assert set(t32) == set(t64) == set(T) and all(v.dtype == torch.float64 for v in t64.values())
    assert torch.equal(t32["eps"], e.reshape(B, -1)) and torch.equal(t64["eps"], e64.reshape(B, -1))
    assert all(v.shape[0] == B for v in t64.values())


@pytest.mark.parametrize("B,hw", [(1, 8), (5, 20)])
def test_tap_caps(B, hw):
    """Every tap's own noise: FACTOR x the fp32 oracle's worst sample stays under CAP, and no tap has a sample
    that is exactly zero in float64 (a zero row would have no relative error)."""
    sd, c = weights(), make_case(B, hw)
    t32, t64 = taps_pair((B, hw), sd, c)
    for k in t64:
        assert bool(t64[k].any(dim=1).all()), k
        assert FACTOR * max(row_errs(t32[k], t64[k])) <= CAP, k
