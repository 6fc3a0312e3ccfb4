"""CPU-only: geometry guidance — the argument rules of the samplers' geom_scale keyword, the signatures,
the ABI of the new entries, the graph key's rules with the geometry member (stand-alone, under the host
sanitizers) and the loss / seed formula against losses.geom_losses.masked_geom_mse row by row."""
import inspect
import os
import shutil
import subprocess

import pytest
import torch

from conftest import REPO

Y = [1, 2, 3]


def setup():
    import diff
    d = diff.Diffuser(1000, device="cpu")
    g = torch.Generator().manual_seed(3)
    vals = torch.rand((3, 12), generator=g)
    mask = (torch.rand((3, 12), generator=g) > 0.3).float()
    return d, vals, mask


class _Geom:  # stands for a dmx network with a GeomHead / without one (the rules read the kind only)
    _dmx_kind = 1

    def native(self):
        raise AssertionError("the argument rules must not touch the model")


class _NoGeom(_Geom):
    _dmx_kind = 2


# ---- argument rules ---------------------------------------------------------------------------------
def test_zero_is_the_plain_call():
    d, vals, mask = setup()
    assert d._geom_args(0.0, 3) is None
    assert d._geom_args(0, 3, _NoGeom(), guidance_scale=0.0, guidance_rescale=0.5, base="dropped") is None
    assert d._geom_args([0.0, 0.0, 0.0], 3) is None
    assert inspect.signature(d.sample_latent_cond).parameters["geom_scale"].default == 0.0
    x = torch.zeros((3, 4, 8, 8))
    for mode in (None, ("ddim", 5, 0.0), ("dpm", 5, "logsnr")):
        plan = d._plan(x, mode, 3.0)
        assert plan.geom is None
        for guided in (True, False):
            assert "geom" not in plan.kwargs(guided, seed=1, use_graph=True)


def test_scale_row_and_plan():
    d, vals, mask = setup()
    ok = dict(model=_Geom(), guidance_scale=3.0, cond=vals)
    row = d._geom_args(1000.0, 3, **ok)
    assert row.dtype == torch.float32 and row.tolist() == [1000.0] * 3
    row = d._geom_args([1.0, 0.0, 2.5], 3, **ok)
    assert row.tolist() == [1.0, 0.0, 2.5]
    assert d._geom_args(torch.tensor([0.0, 0.0, 7.0]), 3, **ok).tolist() == [0.0, 0.0, 7.0]
    assert d._geom_args(1.0, 3, object(), 3.0, cond=vals) is not None      # a foreign model is asked at its first step
    x = torch.zeros((3, 4, 8, 8))
    # the plan carries the rows and the rule's sig table: sqrt(1 - ab) per timestep / per position
    plan = d._plan(x, None, 3.0, geom=row)
    assert torch.equal(plan.geom[0], row) and plan.geom[1] is d.geom_sig("cpu")
    assert torch.equal(plan.geom[1], torch.sqrt(1 - d._host[1])) and plan.geom[1].numel() == 1000
    assert plan.kwargs(True, seed=1)["geom"] is plan.geom and "geom" not in plan.kwargs(False, seed=1)
    for mode in (("ddim", 5, 0.5), ("dpm", 5, "logsnr")):
        plan = d._plan(x, mode, 3.0, geom=row)
        assert plan.geom[1] is plan.sched[1] and plan.geom[1].numel() == 5
        tau = torch.tensor(d._mode_timesteps(mode))
        assert torch.allclose(plan.geom[1], torch.sqrt(1 - d._host[1].double()[tau - 1]).float(), rtol=1e-6, atol=0)
    shard = d._plan(x[1:], ("ddim", 5, 0.0), 3.0, rows=(1, 3), geom=row)     # a shard takes its rows
    assert shard.geom[0].tolist() == [0.0, 2.5] and shard.geom[0].is_contiguous()


@pytest.mark.parametrize("bad", [
    dict(geom_scale=-1.0), dict(geom_scale=[1.0, -0.5, 0.0]), dict(geom_scale=float("nan")),
    dict(geom_scale=[1.0, float("inf"), 0.0]), dict(geom_scale=[1.0, 2.0]), dict(geom_scale="much"),
    dict(model=_NoGeom()), dict(guidance_scale=0.0), dict(guidance_scale=-1.0), dict(guidance_scale=None),
    dict(guidance_scale=[3.0, 3.0, 3.0]), dict(guidance_interval=(1, 500)), dict(guidance_rescale=0.5),
    dict(base="dropped"), dict(base=dict(classes=1)), dict(also=[dict(classes=1, weight=1.0)]), dict(cond=None),
])
def test_refusals(bad):
    d, vals, mask = setup()
    kw = dict(geom_scale=1000.0, model=_Geom(), guidance_scale=3.0, guidance_interval=None, guidance_rescale=0.0,
              base="null", also=None, cond=vals)
    kw.update(bad)
    with pytest.raises(ValueError):
        d._geom_args(kw.pop("geom_scale"), 3, **kw)


def test_all_masks_zero_is_allowed():
    d, vals, mask = setup()
    assert d._geom_args(5.0, 3, _Geom(), 3.0, cond=vals * 0) is not None   # (the mask is not an argument rule)


def test_samplers_raise_before_touching_the_model():
    from dmx import distributed
    d, vals, mask = setup()
    state = torch.get_rng_state()
    bads = (dict(geom_scale=-1.0), dict(geom_scale=[1.0, 2.0]), dict(geom_scale=1.0, guidance_scale=0.0),
            dict(geom_scale=1.0, guidance_rescale=0.5), dict(geom_scale=1.0, guidance_interval=(1, 12)),
            dict(geom_scale=1.0, base="dropped"), dict(geom_scale=1.0, guidance_scale=[3.0, 3.0, 3.0]),
            dict(geom_scale=1.0, cond=None))
    for bad in bads:
        kw = dict(cond=vals, cond_mask=mask)
        kw.update(bad)
        with pytest.raises(ValueError):
            d.sample_latent_cond(_Geom(), {1: 2, 2: 1}, z_shape=(4, 8, 8), vae=None, progress=False, **kw)
        with pytest.raises(ValueError):
            distributed.ShardedCondSampler(d, _Geom(), None).sample({1: 2, 2: 1}, z_shape=(4, 8, 8), decode=False, **kw)
    with pytest.raises(ValueError):
        d.sample_latent_cond(_NoGeom(), {1: 2, 2: 1}, z_shape=(4, 8, 8), vae=None, progress=False, cond=vals,
                             cond_mask=mask, geom_scale=1.0)
    assert torch.equal(torch.get_rng_state(), state)  # nothing was drawn


def test_foreign_model_without_geometry_is_refused():
    import diff
    x = torch.zeros((2, 4, 8, 8))
    t = torch.ones(2, dtype=torch.long)
    v = torch.rand((2, 12))
    with pytest.raises(ValueError):
        diff.Diffuser._geom_loss_grad(lambda x, t, y, cond_vals=None, cond_mask=None: x * 2, x, t, t, v, v)
    # a differentiable stand-in: geom = per-sample mean of x broadcast to 12 columns
    g = diff.Diffuser._geom_loss_grad(
        lambda x, t, y, cond_vals=None, cond_mask=None: (x, x.mean((1, 2, 3))[:, None].expand(-1, 12)), x + 1.0, t, t,
        v, torch.ones((2, 12)))
    exp = (2 * (1.0 - v).sum(-1) / 12 / 256).view(2, 1, 1, 1).expand_as(x)
    assert g.shape == x.shape and not g.requires_grad and torch.allclose(g, exp, rtol=1e-5, atol=1e-8)


# ---- signatures ----------------------------------------------------------------------------------------
def test_keywords_and_signatures():
    import diff
    from dmx import distributed, engine
    from entityCsvSampler import EntityCsvSampler
    from models.unet_cond_geom import UnetCondWithGeomHead
    for fn in (diff.Diffuser.sample_latent_cond, distributed.ShardedCondSampler.sample, EntityCsvSampler.sample):
        assert inspect.signature(fn).parameters["geom_scale"].default == 0.0
    for fn in (engine.NativeModel.step, engine.NativeModel.sample_loop):
        assert inspect.signature(fn).parameters["geom"].default is None
    assert list(inspect.signature(engine.geom_mix).parameters) == ["eps", "grad", "scale", "sig", "pos"]
    assert list(inspect.signature(engine.NativeModel.input_grad).parameters) == ["self", "tape_id", "d_eps", "d_geom"]
    assert list(inspect.signature(engine.NativeModel.geom_grad).parameters) == ["self", "x", "t", "y", "vals", "mask"]
    assert list(inspect.signature(UnetCondWithGeomHead.geom_grad).parameters) == ["self", "x", "t", "y", "cond_vals",
                                                                                  "cond_mask"]
    # the public one-step calls keep their signatures
    for fn in (diff.Diffuser.denoise_cond, diff.Diffuser.ddim_step, diff.Diffuser.dpm_step):
        ps = inspect.signature(fn).parameters
        assert "geom" not in ps and "geom_scale" not in ps
    assert list(inspect.signature(diff.Diffuser.denoise_cond).parameters) == [
        "self", "model", "x", "t", "y", "guidance_scale", "null_label", "cond_vals", "cond_mask"]


def test_geom_grad_needs_a_condition_and_a_gpu(unet_sd):
    from dmx import DmxUnavailable
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead().eval()
    x, t = torch.zeros((1, 4, 8, 8)), torch.ones(1, dtype=torch.long)
    with pytest.raises(ValueError):
        m.geom_grad(x, t, t, None, None)
    with pytest.raises(DmxUnavailable):
        m.geom_grad(x, t, t, torch.zeros((1, 12)), torch.zeros((1, 12)))


# ---- ABI -------------------------------------------------------------------------------------------------
def test_header_and_bindings_name_the_new_symbols():
    from dmx import _lib
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    bound = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for sym in ("dmx_train_backward_input", "dmx_step_geom", "dmx_sample_loop_geom", "dmx_geom_mix", "dmx_geom_seed"):
        assert sym + "(" in hdr and sym in bound, sym
    assert "typedef struct dmx_geom_guide" in hdr and "No gradient for x. */\nint dmx_train_forward" not in hdr
    assert [f[0] for f in _lib.GeomGuide._fields_] == ["scale", "sig", "S"]
    assert len(bound["dmx_train_backward_input"][1]) == 6
    assert len(bound["dmx_step_geom"][1]) == 7 and len(bound["dmx_sample_loop_geom"][1]) == 9
    assert len(bound["dmx_geom_mix"][1]) == 13 and len(bound["dmx_geom_seed"][1]) == 8
    lib = _lib.load()
    assert lib.dmx_abi_version() == 1
    # argument checks that need no device
    assert lib.dmx_train_backward_input(None, 1, None, None, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_step_geom(None, None, None, None, None, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_sample_loop_geom(None, None, None, None, None, None, 1, 0, None) == _lib.DMX_E_ARG
    assert lib.dmx_geom_mix(None, None, None, None, 1, None, 0, None, 1, 4, 8, 8, None) == _lib.DMX_E_ARG
    assert lib.dmx_geom_seed(None, None, None, 1, 12, None, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_last_error()


# ---- the graph key's rules with the geometry member, stand-alone under the host sanitizers ------------------
def test_step_mode_key_standalone_with_geometry(tmp_path):
    from dmx import build
    src = os.path.join(REPO, "tools", "step_mode_check.cpp")
    text = open(src).read()
    for rule in ("in.geom.scale =", "in.geom.sig =", "in.geom.S = 4", "k.geom", "use_geom ? &geom : nullptr",
                 "StepMode{}.geom == nullptr"):
        assert rule in text, rule
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or build.HIPCC  # (host code only)
    exe = str(tmp_path / "step_mode_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "step_mode_check: ok" in out.stdout


# ---- the seed formula -------------------------------------------------------------------------------------
def seed_ref(geom, vals, mask):
    """The torch restatement of dmx_geom_seed: (L (n,), dL/dgeom (n,12))."""
    den = mask.sum(-1, keepdim=True).clamp_min(1e-6)
    loss = (mask * (geom - vals).pow(2)).sum(-1) / den[:, 0]
    return loss, 2 * mask * (geom - vals) / den


def test_seed_formula_is_masked_geom_mse_row_by_row():
    from losses.geom_losses import masked_geom_mse
    g = torch.Generator().manual_seed(9)
    geom, vals = torch.randn((5, 12), generator=g), torch.rand((5, 12), generator=g)
    mask = (torch.rand((5, 12), generator=g) > 0.4).float()
    mask[2] = 0.0
    mask[3] = 1.0
    loss, seed = seed_ref(geom, vals, mask)
    leaf = geom.clone().requires_grad_(True)
    rows = torch.stack([masked_geom_mse(leaf[i:i + 1], vals[i:i + 1], mask[i:i + 1]) for i in range(5)])
    assert torch.allclose(loss, rows.detach(), rtol=1e-6, atol=1e-7)
    grad, = torch.autograd.grad(rows.sum(), leaf)
    assert torch.allclose(seed, grad, rtol=1e-6, atol=1e-8)
    assert float(loss[2]) == 0.0 and bool((seed[2] == 0).all())      # an empty mask: no loss, an exactly zero seed
    assert float(seed[3].abs().min()) > 0
