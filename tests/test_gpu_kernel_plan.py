"""The conv plan, pinned: which kernel runs for which layer (MI355X only).

Model.step_profile returns the ordered (kernel, layer) labels of one eager CFG step.  The fixture
tests/golden/kernel_plan.json holds that sequence for the default conditional U-Net in the three
precision modes, at batches and maps that cover every batch class and low-resolution split
(tests/golden/make_kernel_plan.py: recorded with the library built from the commit BEFORE the
conv-plan refactor; the (17, 32) and (21, 40) plans, added later, from the commit before their addition,
whose library reproduced the earlier plans exactly; never from the code under test).  The library must reproduce each sequence
exactly; timings are ignored.  Arithmetic is pinned elsewhere (test_gpu_parity.py, goldens)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_plan.json")
PRECISIONS = ["x3", "fp32", "f16"]
# (B, H = W): single sample; small class, ragged; the >= 64-sample class after CFG doubling on the
# 32- and 28-wide latents; small maps (the low-resolution paths split differently); the 32..63-sample
# class after CFG doubling (igemm_halo_kernel at up3.0); 42 samples on 40-wide maps (igemm_pp_kernel)
SHAPES = [(1, 32), (5, 32), (32, 32), (32, 28), (3, 16), (17, 32), (21, 40)]


def case_id(prec, B, hw):
    return f"{prec}-B{B}-{hw}x{hw}"


def record_plan(model, diffuser, prec, B, hw, dev):
    """[[kernel, layer], ...] of one eager CFG step (seeded inputs; the plan depends on shapes only)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((B, 4, hw, hw), generator=g).to(dev)
    y = torch.tensor([1 + i % 3 for i in range(B)], dtype=torch.long, device=dev)
    vals = torch.rand((B, 12), generator=g).to(dev)
    mask = torch.ones((B, 12), device=dev)
    t = torch.full((B,), 500, dtype=torch.long, device=dev)
    nm = model.native()
    with nm.precision_override(prec):
        recs = nm.step_profile(x, x.clone(), t, y, 0, vals, mask, 3.0, diffuser.coef_tables(dev, True), None, seed=1)
    torch.cuda.synchronize(dev)
    return [[r["kernel"], r["layer"]] for r in recs]


def model_and_diffuser(dev, sd):
    import diff
    from support import make_model
    return make_model(dev, sd), diff.Diffuser(1000, device=dev)


@pytest.fixture(scope="module")
def plan_model(cuda, unet_sd):
    return model_and_diffuser(cuda, unet_sd)


@pytest.fixture(scope="module")
def fixture_plans():
    with open(FIXTURE) as f:
        return json.load(f)["plans"]


@pytest.mark.parametrize("B,hw", SHAPES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_kernel_plan_matches_parent(plan_model, fixture_plans, cuda, prec, B, hw):
    model, diffuser = plan_model
    want = fixture_plans[case_id(prec, B, hw)]
    got = record_plan(model, diffuser, prec, B, hw, cuda)
    assert len(want) > 50  # a whole U-Net step, not a stub
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}: {g} != recorded {w}"
    assert len(got) == len(want)
