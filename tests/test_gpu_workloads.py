"""Whole-workload parity on the GPU: the drivers' loops, chunked decode, the CSV entry point,
the range guard and the input-normalisation edges (MI355X only).

Fixtures: tests/golden/steps_T12.npz and csv_sample_T20.npz were produced by running the
reference's own generate_steps.save_reverse_steps_for_csv_row and EntityCsvSampler.sample on
the CPU (tests/golden/make_golden_r2.py).  Tolerances as tests/test_gpu_parity.py: latents
rel-L2 <= 1e-4 after a trajectory, 2e-5 per step; uint8 frames |diff| <= 1 on <= 0.1 %.
"""
import glob
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN
from oracle import ref
from oracle.rules import rel
from support import make_model, make_vae

pytestmark = pytest.mark.gpu

CSV = os.path.join(GOLDEN, "entities.csv")


def u8_close(a, b, frac=1e-3, lsb=1):
    d = np.abs(np.asarray(a, np.int32) - np.asarray(b, np.int32))
    return d.max() <= lsb and (d > 0).mean() <= frac, (int(d.max()), float((d > 0).mean()))


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    return make_model(cuda, unet_sd)


@pytest.fixture(scope="module")
def vae(cuda, vae_sd):
    return make_vae(cuda, vae_sd)


# ---- config 5 / a16: generate_steps.py -----------------------------------------------------------
def _read_run(out_dir, T):
    pix = np.stack([np.asarray(Image.open(os.path.join(out_dir, "pixel", f"t{i}.png"))) for i in range(T, 0, -1)])
    lat = np.stack([np.stack([np.asarray(Image.open(os.path.join(out_dir, "latent", f"ch{c:02d}", f"t{i}.png")))
                              for c in range(4)]) for i in range(T, 0, -1)])
    return pix, lat


def test_generate_steps_dropin_vs_reference(golden, model, vae, cuda, tmp_path):
    """Our save_reverse_steps_for_csv_row (async PNG pipeline) vs the reference function's own files."""
    import generate_steps as gs
    g = golden("steps_T12.npz")
    T = int(g["T"])
    torch.manual_seed(int(g["seed"]))
    out_dir = gs.save_reverse_steps_for_csv_row(csv_path=CSV, row_index=int(g["row"]), class_id=int(g["class_id"]),
                                                model=model, vae=vae, device="cuda", num_timesteps=T,
                                                z_shape=(1, 4, 28, 28), out_root=str(tmp_path), run_name="run",
                                                progress=False)
    assert len(glob.glob(os.path.join(out_dir, "**", "*.png"), recursive=True)) == int(g["n_files"])
    pix, lat = _read_run(out_dir, T)
    ok, info = u8_close(pix, g["pixel"])
    assert ok, ("pixel", info)
    ok, info = u8_close(lat, g["latent_png"], frac=2e-3)
    assert ok, ("latent", info)
    assert rel(gs.save_reverse_steps_for_csv_row.last_latent, g["x_final"]) < 1e-4


def test_generate_steps_loop_body_per_step(golden, model, vae, cuda):
    """generate_steps.py:158-189 driven by hand on the drop-in surface: Diffuser.denoise_cond +
    VAE.decode + reverse_to_img, host draws; every x_t and every frame vs the reference's."""
    import diff
    from generate_steps import latent_frames_u8
    g = golden("steps_T12.npz")
    T = int(g["T"])
    d = diff.Diffuser(T, device=cuda)
    vals, mask = torch.from_numpy(g["vals"]).to(cuda), torch.from_numpy(g["mask"]).to(cuda)
    y = torch.tensor([int(g["class_id"])], device=cuda)
    torch.manual_seed(int(g["seed"]))
    x = torch.randn((1, 4, 28, 28)).to(cuda)
    for k, i in enumerate(range(T, 0, -1)):
        assert rel(x, g["x_t"][k:k + 1]) < 2e-5 * (k + 1), i
        img = vae.decode(x).clamp(0, 1)
        frame = np.asarray(d.reverse_to_img(img[0]))
        ok, info = u8_close(frame, g["pixel"][k])
        assert ok, (i, info)
        ok, info = u8_close(latent_frames_u8(x).cpu().numpy()[0], g["latent_png"][k], frac=2e-3)
        assert ok, (i, info)
        t = torch.full((1,), i, dtype=torch.long, device=cuda)
        x = d.denoise_cond(model, x, t, y=y, guidance_scale=3.0, null_label=0, cond_vals=vals, cond_mask=mask)
    assert rel(x, g["x_final"]) < 1e-4


def test_latent_frames_kernel_bit_exact(cuda):
    """dmx_latent_frames_u8 == the reference's torch/numpy min-max -> *255 -> uint8, byte for byte
    (including a constant channel)."""
    from generate_steps import latent_frames_u8
    z = torch.randn((3, 4, 28, 28), generator=torch.Generator().manual_seed(8))
    z[1, 2] = 0.75
    got = latent_frames_u8(z.to(cuda)).cpu()
    assert torch.equal(got, latent_frames_u8(z))


def test_generate_steps_device_noise_runs_and_is_deterministic(model, vae, cuda, tmp_path):
    import generate_steps as gs
    outs = []
    for r in range(2):
        torch.manual_seed(3)
        d = gs.save_reverse_steps_for_csv_row(csv_path=CSV, row_index=1, class_id=1, model=model, vae=vae,
                                              device="cuda", num_timesteps=8, out_root=str(tmp_path),
                                              run_name=f"dev{r}", progress=False, noise_source="device",
                                              save_every=3)
        outs.append((_read_run_sparse(d), gs.save_reverse_steps_for_csv_row.last_latent.cpu()))
    assert torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[1][0])


def _read_run_sparse(out_dir):
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*.png"), recursive=True))
    return np.concatenate([np.asarray(Image.open(f)).ravel() for f in files])


# ---- sample_latent_cond: decode chunk loop, CSV entry point -------------------------------------
def test_sample_latent_cond_b40_decode_chunks_vs_oracle(model, vae, cuda, unet_sd, vae_sd):
    """B = 40 crosses dmx_vae_decode's chunk loop three times (16 + 16 + 8)."""
    import diff
    T, B = 3, 40
    d = diff.Diffuser(T, device=cuda)
    g = torch.Generator().manual_seed(12)
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.4).float()
    torch.manual_seed(13)
    img = d.sample_latent_cond(model, {1: 15, 2: 15, 3: 10}, z_shape=(4, 16, 16), vae=vae, to_pil=False,
                               progress=False, cond=vals.to(cuda), cond_mask=mask.to(cuda))
    torch.manual_seed(13)
    pil = d.sample_latent_cond(model, {1: 15, 2: 15, 3: 10}, z_shape=(4, 16, 16), vae=vae, to_pil=True,
                               progress=False, cond=vals.to(cuda), cond_mask=mask.to(cuda))
    y = torch.tensor([1] * 15 + [2] * 15 + [3] * 10)
    torch.manual_seed(13)
    lat, _ = ref.sample_latent_cond(unet_sd, y, vals, mask, (4, 16, 16), T=T)
    with torch.no_grad():
        exp = ref.vae_decode(vae_sd, lat)
    assert img.shape == (B, 3, 128, 128)
    assert rel(img, exp) < 1e-4
    u8 = np.stack([np.asarray(p) for p in pil])
    ok, info = u8_close(u8, ref.to_uint8(exp).permute(0, 2, 3, 1).numpy())
    assert ok, info


def test_entity_csv_sampler_sample_vs_reference(golden, model, vae, cuda):
    """EntityCsvSampler.sample end to end (28x28 latents via the replayed encode draw)."""
    import diff
    from entityCsvSampler import EntityCsvSampler
    g = golden("csv_sample_T20.npz")
    d = diff.Diffuser(int(g["T"]), device=cuda)
    s = EntityCsvSampler(d, model, vae, class_id=int(g["class_id"]), base_wh=(400, 400), device=cuda)
    torch.manual_seed(int(g["seed"]))
    imgs = s.sample(CSV, count=int(g["count"]), start=int(g["start"]), guidance_scale=3.0)
    u8 = np.stack([np.asarray(im) for im in imgs])
    ok, info = u8_close(u8, g["u8"])
    assert ok, info


# ---- input normalisation --------------------------------------------------------------
def test_ddpm_update_fp16_and_noncontiguous_eps(cuda):
    import diff
    from dmx import engine
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(31)
    B = 3
    x, eu, ec, nz = (torch.randn((B, 4, 8, 8), generator=g) for _ in range(4))
    t = torch.tensor([1, 400, 1000])
    eu16, ec16 = eu.half(), ec.half()
    out = engine.ddpm_update(x.to(cuda).transpose(2, 3).contiguous().transpose(2, 3), eu16.to(cuda),
                             ec16.to(cuda).transpose(2, 3).contiguous().transpose(2, 3), 3.0, t.to(cuda),
                             d.coef_tables(cuda, True), nz.to(cuda)[:, :, :, :]).cpu()
    _, a, ab = ref.schedule(1000)
    eps = eu16.float() + 3.0 * (ec16.float() - eu16.float())
    assert torch.equal(out, ref.ddpm_update(x, eps, t, a, ab, nz))


def test_denoise_cond_bool_mask_and_sliced_cond(model, cuda, unet_sd):
    """A bool cond_mask and a column-sliced (non-contiguous) float64 cond: converted like torch.cat would."""
    import diff
    d = diff.Diffuser(1000, device=cuda)
    g = torch.Generator().manual_seed(32)
    B = 2
    x = torch.randn((B, 4, 16, 16), generator=g)
    wide = torch.rand((B, 24), generator=g, dtype=torch.float64)
    vals = wide[:, ::2]
    mask = torch.rand((B, 12), generator=g) > 0.5
    y = torch.tensor([2, 3])
    t = torch.tensor([700, 700])
    torch.manual_seed(5)
    out = d.denoise_cond(model, x.to(cuda), t.to(cuda), y=y.to(cuda), guidance_scale=3.0, cond_vals=vals.to(cuda),
                         cond_mask=mask.to(cuda))
    torch.manual_seed(5)
    _, a, ab = ref.schedule(1000)
    with torch.no_grad():
        exp = ref.cfg_step(unet_sd, x, t, y, a, ab, 3.0, 0, vals.float(), mask.float(), torch.randn(x.shape))
    assert rel(out, exp) < 2e-5


# ---- split-precision range: trained-like magnitudes, and the overflow guard --------------------
def _stressed(sd):
    """Trained-like magnitudes: GN / LN gammas in U(0.5, 8), conv weights x4."""
    g = torch.Generator().manual_seed(77)
    out = {}
    for k, v in sd.items():
        if ("double_conv.1." in k or "double_conv.4." in k or ".ln." in k or "ff_self.0." in k) and k.endswith("weight"):
            out[k] = 0.5 + 7.5 * torch.rand(v.shape, generator=g)
        elif v.dim() == 4:
            out[k] = v * 4.0
        else:
            out[k] = v.clone()
    return out


def _fp64(sd):
    return {k: v.double() for k, v in sd.items()}


def _fp32_semantics(ours, ref32, ref64):
    """Such a network amplifies rounding (the reference's own fp32 result sits e32 away from the
    fp64 one), so "fp32 semantics" means: no further from fp64 than 4x the reference's fp32 error
    (plus the 2e-5 floor of the well-conditioned tests)."""
    e32, e = rel(ref32, ref64), rel(ours, ref64)
    assert e <= 4 * e32 + 2e-5, (e, e32)
    return e, e32


@pytest.fixture(scope="module")
def stressed(cuda, unet_sd):
    from models.unet_cond_geom import UnetCondWithGeomHead
    sd = _stressed(unet_sd)
    m = UnetCondWithGeomHead()
    m.load_state_dict(sd)
    return m.to(cuda).eval(), sd


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_stress_magnitudes_cfg_step_b64(stressed, cuda, prec):
    import diff
    m, sd = stressed
    nm = m.native()
    with nm.precision_override(prec):
        d = diff.Diffuser(1000, device=cuda)
        g = torch.Generator().manual_seed(33)
        B = 64
        x = 3.0 * torch.randn((B, 4, 32, 32), generator=g)
        y = torch.tensor([1 + i % 3 for i in range(B)])
        vals = torch.rand((B, 12), generator=g)
        mask = (torch.rand((B, 12), generator=g) > 0.5).float()
        t = torch.full((B,), 321, dtype=torch.long)
        torch.manual_seed(8)
        out = d.denoise_cond(m, x.to(cuda), t.to(cuda), y=y.to(cuda), guidance_scale=3.0, cond_vals=vals.to(cuda),
                             cond_mask=mask.to(cuda))
        assert not nm.range_tripped()
    torch.manual_seed(8)
    noise = torch.randn(x.shape)
    _, a, ab = ref.schedule(1000)
    with torch.no_grad():
        exp = ref.cfg_step(sd, x, t, y, a, ab, 3.0, 0, vals, mask, noise)
        exp64 = ref.cfg_step(_fp64(sd), x.double(), t, y, a.double(), ab.double(), 3.0, 0, vals.double(),
                             mask.double(), noise.double())
    _fp32_semantics(out, exp, exp64)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_stress_magnitudes_forward_28(stressed, cuda, prec):
    m, sd = stressed
    g = torch.Generator().manual_seed(34)
    x = 3.0 * torch.randn((3, 4, 28, 28), generator=g)
    t = torch.tensor([1000, 517, 1])
    y = torch.tensor([0, 2, 3])
    vals = torch.rand((3, 12), generator=g)
    mask = (torch.rand((3, 12), generator=g) > 0.5).float()
    with m.native().precision_override(prec), torch.no_grad():
        eps, geom = m(x.to(cuda), t.to(cuda), y.to(cuda), cond_vals=vals.to(cuda), cond_mask=mask.to(cuda))
        e2, g2 = ref.unet_cond_geom_forward(sd, x, t, y, vals, mask)
        e64, g64 = ref.unet_cond_geom_forward(_fp64(sd), x.double(), t, y, vals.double(), mask.double())
    _fp32_semantics(eps, e2, e64)
    _fp32_semantics(geom, g2, g64)


def test_range_guard_replays_overflowing_chunk_in_fp32(cuda, unet_sd):
    """A GroupNorm gamma of 1e5 pushes the f16 hi plane of inc's mid activation past 65504: the x3
    step goes non-finite, the output kernels raise the flag, and the sampler replays the chunk in
    exact-fp32 mode — the result matches the oracle and the model is back in x3 mode."""
    import diff
    from models.unet_cond_geom import UnetCondWithGeomHead
    sd = {k: v.clone() for k, v in unet_sd.items()}
    sd["inc.double_conv.1.weight"] = sd["inc.double_conv.1.weight"] * 1e5
    m = UnetCondWithGeomHead()
    m.load_state_dict(sd)
    m.to(cuda).eval()
    nm = m.native()
    assert nm.precision == "x3"
    d = diff.Diffuser(4, device=cuda)
    g = torch.Generator().manual_seed(35)
    vals = torch.rand((2, 12), generator=g)
    mask = torch.ones((2, 12))
    torch.manual_seed(36)
    lat = d.sample_latent_cond(m, {1: 1, 2: 1}, z_shape=(4, 16, 16), vae=None, progress=False,
                               cond=vals.to(cuda), cond_mask=mask.to(cuda))
    assert d.range_fallbacks == 1 and nm.precision == "x3"
    torch.manual_seed(36)
    exp, _ = ref.sample_latent_cond(sd, torch.tensor([1, 2]), vals, mask, (4, 16, 16), T=4)
    assert torch.isfinite(lat).all()
    assert rel(lat, exp) < 1e-4


def test_time_table_growth_recaptures_graphs(model, cuda):
    """Growing the context's time table (a forward at t > 1000) must not leave a captured step graph
    pointing at the freed table (graph key carries the table generation)."""
    import diff
    nm = model.native()
    d = diff.Diffuser(1000, device=cuda)
    tables = d.coef_tables(cuda, True)
    B = 2
    g = torch.Generator().manual_seed(37)
    x0 = torch.randn((B, 4, 16, 16), generator=g).to(cuda)
    y = torch.tensor([1, 3], device=cuda)
    vals = torch.rand((B, 12), generator=g).to(cuda)
    mask = torch.ones((B, 12), device=cuda)

    def run(use_graph):
        x = x0.clone()
        t = torch.full((1,), 1000, dtype=torch.long, device=cuda)
        nm.sample_loop(x, t, y, 0, vals, mask, 3.0, tables, 3, seed=5, use_graph=use_graph)
        torch.cuda.synchronize()
        return x.cpu()

    first = run(True)
    with torch.no_grad():
        model(x0, torch.tensor([1500, 3000], device=cuda), y)  # grows the table to >= 3000
    assert nm.ctx.tmax >= 3000
    assert torch.equal(run(True), first) and torch.equal(run(False), first)
