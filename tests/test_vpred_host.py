"""CPU-only: v-prediction's host side — the Diffuser keyword and its refusals, the conversion tables, the
v-form of the min-SNR weights, geom_sig in both modes, the torch-op training loss on the v-target, the
algebra of the torch restatement that tests/test_gpu_vpred.py compares the GPU against, the new ABI
symbols, and the argument rules of the new entries as a stand-alone program under the host sanitizers.

Definitions, with sa = sqrt(ab_t), s1 = sqrt(1 - ab_t) at row t - 1:
  x_t = sa z + s1 noise;   v = sa noise - s1 z;   eps = sa v + s1 x_t   (= noise, since sa^2 + s1^2 = 1)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest
import torch
from torch import nn

import diff
from conftest import REPO


# ---- the keyword ------------------------------------------------------------------------------------------
def test_keyword_default_and_refusals():
    sig = inspect.signature(diff.Diffuser.__init__)
    names = list(sig.parameters)
    assert names[:5] == ["self", "num_timesteps", "beta_start", "beta_end", "device"]  # the reference's four
    p = sig.parameters["prediction"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "eps"
    assert diff.Diffuser().prediction == "eps" and diff.Diffuser(12, prediction="v").prediction == "v"
    assert diff.Diffuser(1000, 0.0001, 0.02, "cpu").prediction == "eps"
    with pytest.raises(TypeError):
        diff.Diffuser(1000, 0.0001, 0.02, "cpu", "v")
    for bad in ("x0", "V", "epsilon", "", None, 1, b"v", ["v"]):
        with pytest.raises(ValueError):
            diff.Diffuser(prediction=bad)


@pytest.mark.parametrize("T", [1000, 12])
def test_tables_are_noise_tables(T):
    for kind in ("eps", "v"):
        d = diff.Diffuser(T, prediction=kind)
        p_o, p_x = d.pred_tables("cpu")
        sa, s1 = d.noise_tables("cpu")
        assert p_o is sa and p_x is s1  # the same values, not a second evaluation
        ab = torch.cumprod(1 - torch.linspace(0.0001, 0.02, T), dim=0)
        assert torch.equal(p_o, torch.sqrt(ab)) and torch.equal(p_x, torch.sqrt(1 - ab))
        assert p_o.dtype == torch.float32 and tuple(p_o.shape) == (T,) and p_o.is_contiguous()


# ---- min-SNR-gamma, v form -------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1000, 12])
def test_min_snr_v_weights(T):
    dv, de = diff.Diffuser(T, prediction="v"), diff.Diffuser(T)
    ab = torch.cumprod(1 - torch.linspace(0.0001, 0.02, T), dim=0).double()
    snr = ab / (1 - ab)
    for gamma in (5.0, float(snr[T // 2])):
        w = dv.loss_weights("min_snr", snr_gamma=gamma)
        assert w.dtype == torch.float32 and tuple(w.shape) == (T,)
        assert torch.equal(w, (torch.minimum(snr, torch.tensor(gamma, dtype=torch.float64)) / (snr + 1)).float())
        assert bool((w > 0).all()) and bool((w < 1).all())
        # the eps form is untouched, and is the v form times (SNR + 1) / SNR
        we = de.loss_weights("min_snr", snr_gamma=gamma)
        assert torch.equal(we, (torch.minimum(snr, torch.tensor(gamma, dtype=torch.float64)) / snr).float())
    if T == 1000:  # gamma = 5: below 1 at small t (SNR >> gamma) and at large t (SNR << 1)
        w = dv.loss_weights("min_snr", snr_gamma=5.0)
        assert float(w[0]) < 1e-3 and float(w[-1]) < 1e-3 and float(w.max()) > 0.5
    assert torch.equal(dv.loss_weights("uniform"), torch.ones(T))
    # one Diffuser per kind: the cached tables do not leak from one to the other
    assert not torch.equal(dv.loss_weights("min_snr"), de.loss_weights("min_snr"))


# ---- geometry guidance's sig table -------------------------------------------------------------------------
def test_geom_sig_both_modes():
    T = 1000
    ab = torch.cumprod(1 - torch.linspace(0.0001, 0.02, T), dim=0)
    de, dv = diff.Diffuser(T), diff.Diffuser(T, prediction="v")
    assert torch.equal(de.geom_sig("cpu"), torch.sqrt(1 - ab))
    assert torch.equal(dv.geom_sig("cpu"), torch.sqrt(1 - ab) / torch.sqrt(ab))
    assert dv.geom_sig("cpu") is dv.geom_sig("cpu") and dv.geom_sig("cpu").dtype == torch.float32
    # the strided rules: k_e per position, over k_a for a v-model
    x = torch.zeros((2, 4, 8, 8))
    row = torch.tensor([1.5, 0.0])
    for mode, sched_of in ((("ddim", 7, 0.0), lambda d: d.ddim_tables(7, 0.0, "cpu")),
                           (("dpm", 6, "logsnr"), lambda d: d.dpm_tables(6, "logsnr", "cpu"))):
        pe = de._plan(x, mode, 3.0, geom=row)
        pv = dv._plan(x, mode, 3.0, geom=row)
        sched = sched_of(dv)
        assert torch.equal(pe.geom[1], sched[1]) and torch.equal(pv.geom[1], sched[1] / sched[2])
        assert torch.equal(pv.geom[0], row) and pv.geom[1].is_contiguous()
        tau = sched[0]
        # the same quantity per position, up to the roundings of the two ways to tabulate it
        assert torch.allclose(pv.geom[1], dv.geom_sig("cpu")[tau - 1], rtol=1e-6, atol=0)
    assert dv._plan(x, None, 3.0, geom=row).geom[1] is dv.geom_sig("cpu")


# ---- the algebra of the restatement, in float64 ----------------------------------------------------------
def test_target_converted_at_the_noised_latent_is_the_noise():
    d = diff.Diffuser(1000, prediction="v")
    g = torch.Generator().manual_seed(3)
    z = torch.randn((6, 4, 8, 8), generator=g, dtype=torch.float64)
    noise = torch.randn((6, 4, 8, 8), generator=g, dtype=torch.float64)
    t = torch.tensor([1, 2, 500, 999, 1000, 37])
    ab = d._host[1].double()[t - 1].view(-1, 1, 1, 1)
    sa, s1 = torch.sqrt(ab), torch.sqrt(1 - ab)
    x_t = sa * z + s1 * noise                      # add_noise(z, t) with the draw given
    v = sa * noise - s1 * z                        # the target
    eps = sa * v + s1 * x_t                        # the conversion
    assert float((eps - noise).abs().max()) < 1e-13
    x0 = sa * x_t - s1 * v                         # and the direct data prediction
    assert float((x0 - z).abs().max()) < 1e-13
    # add_noise itself draws: its output obeys the same identity with its own noise
    torch.manual_seed(4)
    x_t32, n32 = diff.Diffuser(1000).add_noise(z.float(), t)
    sa32, s132 = (k[t - 1].view(-1, 1, 1, 1) for k in d.pred_tables("cpu"))
    v32 = sa32 * n32 - s132 * z.float()
    assert float((sa32 * v32 + s132 * x_t32 - n32).abs().max()) < 1e-5


# ---- the torch-op training loss ---------------------------------------------------------------------------
class TinyNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(4, 4, 3, padding=1)
        self.emb = nn.Embedding(4, 4)

    def forward(self, x, t, y, cond_vals=None, cond_mask=None):
        e = self.emb(y) + torch.sin(t.float() / 100.0).unsqueeze(1)
        return self.conv(x) * (1 + e[:, :, None, None])


@pytest.mark.parametrize("weighting", ["uniform", "min_snr"])
def test_training_loss_torch_path_regresses_on_v(weighting):
    torch.manual_seed(0)
    net = TinyNet()
    g = torch.Generator().manual_seed(1)
    z = torch.randn((3, 4, 8, 8), generator=g)
    noise = torch.randn((3, 4, 8, 8), generator=g)
    y = torch.tensor([1, 2, 3])
    t = torch.tensor([1000, 40, 1])
    drop = torch.zeros(3, dtype=torch.bool)
    dv, de = diff.Diffuser(1000, prediction="v"), diff.Diffuser(1000)
    rv = dv.training_loss(net, z, y, weighting=weighting, t=t, noise=noise, drop=drop)
    re = de.training_loss(net, z, y, weighting=weighting, t=t, noise=noise, drop=drop)
    ab = dv._host[1][t - 1].view(-1, 1, 1, 1)
    target = torch.sqrt(ab) * noise - torch.sqrt(1 - ab) * z
    assert torch.equal(rv.target, target) and not rv.target.requires_grad
    assert re.target is noise or torch.equal(re.target, noise)
    assert torch.equal(rv.eps, re.eps)  # the network saw the same noised latent
    w = dv.loss_weights(weighting)[t - 1]
    exp = (w * (rv.eps - target).pow(2).flatten(1).mean(1)).mean()
    assert torch.allclose(rv.loss.detach(), exp, rtol=1e-6, atol=0)
    assert torch.equal(rv.per_sample, w * (rv.eps - target).pow(2).flatten(1).mean(1))
    we = de.loss_weights(weighting)[t - 1]
    assert torch.allclose(re.loss.detach(), (we * (re.eps - noise).pow(2).flatten(1).mean(1)).mean(), rtol=1e-6, atol=0)
    rv.loss.backward()
    assert all(p.grad is not None for p in net.parameters())
    assert [f.name for f in __import__("dataclasses").fields(diff.TrainingLoss)][-1] == "target"


# ---- ABI -------------------------------------------------------------------------------------------------
NEW = {"dmx_model_set_prediction": 6, "dmx_model_get_prediction": 1, "dmx_pred_to_eps": 13,
       "dmx_train_noise_target": 3}


def test_header_and_bindings_name_the_new_symbols():
    from dmx import _lib
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    bound = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for sym, nargs in NEW.items():
        assert sym + "(" in hdr and sym in bound and len(bound[sym][1]) == nargs, sym
    assert "#define DMX_PRED_EPS 0" in hdr and "#define DMX_PRED_V 1" in hdr
    lib = _lib.load()
    for sym in NEW:
        assert hasattr(lib, sym), sym
    assert lib.dmx_abi_version() == 1  # additive: the version stays
    assert ctypes.sizeof(_lib.NoiseArgs) == 160 and ctypes.sizeof(_lib.ObjectiveArgs) == 128
    assert ctypes.sizeof(_lib.StepArgs) == 144
    # argument checks that need no device
    assert lib.dmx_model_set_prediction(None, 1, None, None, 1000, None) == _lib.DMX_E_ARG
    assert lib.dmx_model_get_prediction(None) == -1
    assert lib.dmx_pred_to_eps(None, None, None, 1, None, None, 1000, 1, 4, 8, 8, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_train_noise_target(None, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_last_error()


def test_python_entries_refuse_without_a_device():
    from dmx import engine
    from dmx._lib import DmxUnavailable
    x = torch.zeros((2, 4, 8, 8))
    t = torch.ones(2, dtype=torch.long)
    d = diff.Diffuser(1000, prediction="v")
    with pytest.raises(DmxUnavailable):
        engine.pred_to_eps(x, x, t, *d.pred_tables("cpu"))
    assert "target" in inspect.signature(engine.train_noise).parameters
    assert inspect.signature(engine.train_noise).parameters["target"].default is None
    assert callable(engine.NativeModel.set_prediction) and engine.NativeModel.PREDICTIONS == {"eps": 0, "v": 1}


# ---- the argument rules, stand-alone under the host sanitizers --------------------------------------------
def test_prediction_args_standalone(tmp_path):
    from dmx import build
    src = os.path.join(REPO, "tools", "prediction_args_check.cpp")
    text = open(src).read()
    for rule in ("set_prediction_error(", "pred_to_eps_error(", "prediction_range_error(",
                 "sizeof(dmx_noise_args) == 160", "sizeof(dmx_objective_args) == 128", "sizeof(dmx_step_args) == 144"):
        assert rule in text, rule
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or build.HIPCC  # (host code only)
    exe = str(tmp_path / "prediction_args_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "prediction_args_check: ok" in out.stdout


def test_bench_tools_take_the_keyword():
    for tool in ("sampler_bench.py", "objective_bench.py"):
        text = open(os.path.join(REPO, "tools", tool)).read()
        assert '"--prediction"' in text and 'choices=["eps", "v"]' in text, tool
