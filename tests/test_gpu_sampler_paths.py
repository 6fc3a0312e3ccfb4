"""GPU: the single-process sampler and the sharded sampler at world size 1 walk one plan
(diff._SamplerPlan), so with the same seed they return the same bytes: for every sampler and both noise
sources, plain, with a guidance interval plus rescale, and with a known region (init_latent + mask +
strength).  No tolerance applies.  Diffuser(40) with GUARD_CHUNK = 4, B = 3, latents 4 x 8 x 8: every loop
runs as several guard chunks, and the interval cuts chunks into segments."""
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = {1: 2, 3: 1}
Z = (4, 8, 8)


@pytest.fixture(scope="module")
def model(cuda, unet_sd):
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(unet_sd)
    return m.to(cuda).eval()


def _variant(name):
    if name == "plain":
        return {}
    if name == "interval_rescale":
        return dict(guidance_interval=(8, 30), guidance_rescale=0.5)
    g = torch.Generator().manual_seed(2)
    return dict(init_latent=torch.randn((3,) + Z, generator=g), strength=0.5,
                mask=(torch.rand(Z[1:], generator=g) > 0.5).float())


@pytest.mark.parametrize("variant", ["plain", "interval_rescale", "known"])
@pytest.mark.parametrize("noise_source", ["host", "device"])
@pytest.mark.parametrize("sampler", [dict(), dict(sampler="ddim", steps=6, eta=0.5),
                                     dict(sampler="dpmpp_2m", steps=6)], ids=["ddpm", "ddim", "dpmpp_2m"])
def test_sharded_world1_equals_single_process(model, cuda, sampler, noise_source, variant):
    import diff
    from dmx.distributed import ShardedCondSampler
    d = diff.Diffuser(40, device=cuda)
    d.GUARD_CHUNK = 4
    d.noise_source = noise_source
    kw = dict(guidance_scale=3.0, **sampler, **_variant(variant))
    g = torch.Generator().manual_seed(4)
    cond = torch.rand((3, 12), generator=g)
    torch.manual_seed(21)
    single = d.sample_latent_cond(model, COUNTS, z_shape=Z, vae=None, progress=False, cond=cond, **kw)
    torch.manual_seed(21)
    sharded = ShardedCondSampler(d, model, None).sample(COUNTS, z_shape=Z, decode=False, cond=cond, **kw)
    assert single.shape == (3,) + Z and bool(torch.isfinite(single).all())
    assert torch.equal(sharded, single)
