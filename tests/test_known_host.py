"""CPU-only: the host side of known-region sampling (img2img start, masked inpainting) — the blend's
tables, the truncated DPM-Solver++ start, the start position and the samplers' argument rules.

Restated here in float64 from the Diffuser's fp32 alpha_bars (ab[0] := 1), for ascending timesteps tau
(tau_p at index p-1, tau_0 = 0):
  row p-1: q_a = sqrt(ab[tau_{p-1}]), q_e = sqrt(1 - ab[tau_{p-1}]);  row 0 = (1, 0)
  p0 = S for strength None, else min(S, max(1, floor(strength S + 0.5)))
  dpm_tables(S, sp, start=p0 < S): row p0 first-order (k_c = m, k_p = 0), every other row unchanged."""
import math

import pytest
import torch

import diff


def ab64(d):
    return [1.0] + [float(v) for v in d._host[1].double()]


@pytest.mark.parametrize("T,mode", [(1000, None), (1000, ("ddim", 50, 0.0)), (1000, ("dpm", 20, "logsnr")),
                                    (40, ("dpm", 7, "uniform")), (40, None), (40, ("ddim", 1, 0.0))])
def test_known_tables_match_float64_restatement(T, mode):
    d = diff.Diffuser(T)
    tau = d._mode_timesteps(mode)
    assert tau == (list(range(1, T + 1)) if mode is None else d.ddim_timesteps(mode[1]) if mode[0] == "ddim"
                   else d.dpm_timesteps(mode[1], mode[2]))
    q_a, q_e = d.known_tables(tau)
    ab = ab64(d)
    s = [0] + list(tau[:-1])
    assert q_a.dtype == q_e.dtype == torch.float32 and q_a.shape == q_e.shape == (len(tau),)
    assert torch.equal(q_a, torch.tensor([math.sqrt(ab[v]) for v in s], dtype=torch.float64).float())
    assert torch.equal(q_e, torch.tensor([math.sqrt(1 - ab[v]) for v in s], dtype=torch.float64).float())
    assert float(q_a[0]) == 1.0 and float(q_e[0]) == 0.0  # row 0: the known latent itself
    assert d.known_tables(tuple(tau)) is d.known_tables(list(tau))  # cached per (tau, device)


def test_known_tables_reject_bad_timesteps():
    d = diff.Diffuser(40)
    for bad in ([], [0, 3], [3, 3], [5, 4], [1, 41]):
        with pytest.raises(ValueError):
            d.known_tables(bad)


@pytest.mark.parametrize("S,spacing", [(11, "logsnr"), (8, "uniform"), (3, "logsnr"), (2, "logsnr")])
def test_dpm_tables_truncated_start(S, spacing):
    d = diff.Diffuser(1000)
    base = d.dpm_tables(S, spacing)
    assert d.dpm_tables(S, spacing, start=None) is base
    assert d.dpm_tables(S, spacing, "cpu", None) is base
    assert d.dpm_tables(S, spacing, start=S) is base  # position S is first-order already
    ab = ab64(d)
    tau = d.dpm_timesteps(S, spacing)
    for p0 in range(1, S):
        tr = d.dpm_tables(S, spacing, start=p0)
        assert tr is d.dpm_tables(S, spacing, start=p0) and tr is not base
        assert type(tr) is type(base) and len(tr) == 6
        for a, b in zip(tr[:4], base[:4]):
            assert torch.equal(a, b)
        rows = torch.arange(S) != p0 - 1
        assert torch.equal(tr[4][rows], base[4][rows]) and torch.equal(tr[5][rows], base[5][rows])
        assert float(tr[5][p0 - 1]) == 0.0
        t, s = tau[p0 - 1], (tau[p0 - 2] if p0 > 1 else 0)
        k_x = math.sqrt(1 - ab[s]) / math.sqrt(1 - ab[t])
        m = math.sqrt(ab[s]) - k_x * math.sqrt(ab[t])
        assert float(tr[4][p0 - 1]) == float(torch.tensor(m, dtype=torch.float64).float())
        if 1 < p0:  # a second-order row of the full schedule: the truncated one differs there
            assert float(base[5][p0 - 1]) != 0.0
    assert torch.equal(d.dpm_tables(S, spacing)[5], base[5])  # the default object was not written
    for bad in (0, S + 1, -1):
        with pytest.raises(ValueError):
            d.dpm_tables(S, spacing, start=bad)


def test_start_position_formula_and_edges():
    f = diff.Diffuser._known_start
    for S in (1, 4, 11, 50, 1000):
        assert f(None, S) == S
        assert f(1.0, S) == S
        assert f(0.5 / S, S) == 1
        assert f(math.nextafter(1.0, 0.0), S) == S
        assert f(1e-9, S) == 1
        for strength in (0.1, 0.25, 0.5, 0.64, 0.75, 0.999):
            assert f(strength, S) == min(S, max(1, math.floor(strength * S + 0.5)))
    assert f(0.64, 11) == 7 and f(0.75, 4) == 3 and f(0.5, 11) == 6 and f(0.04, 11) == 1
    for bad in (0.0, -0.1, 1.0000001, 2, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            f(bad, 10)


def test_known_inputs_normalisation():
    f = diff.Diffuser._known_inputs
    assert f(None, None, None, 3, (4, 8, 8)) is None
    z = torch.randn(4, 6, 5)
    z0, m, s, shape = f(z, None, None, 3, None)
    assert m is None and s is None and shape == (4, 6, 5)
    assert z0.shape == (3, 4, 6, 5) and z0.is_contiguous() and all(torch.equal(z0[i], z) for i in range(3))
    z0, m, s, shape = f(z.double().unsqueeze(0), torch.ones(6, 5, dtype=torch.bool), 0.5, 2, (4, 6, 5))
    assert z0.dtype == m.dtype == torch.float32 and z0.shape == (2, 4, 6, 5) and s == 0.5
    assert m.shape == (2, 1, 6, 5) and m.is_contiguous() and bool((m == 1).all())
    zb = torch.randn(2, 4, 6, 5)
    mb = torch.rand(2, 1, 6, 5)
    z0, m, _, _ = f(zb, mb, None, 2, None)
    assert torch.equal(z0, zb) and torch.equal(m, mb)
    _, m, _, _ = f(zb, mb[:1], 1.0, 2, None)
    assert torch.equal(m[0], mb[0]) and torch.equal(m[1], mb[0])


def test_every_argument_rule_raises_value_error():
    d = diff.Diffuser(40)
    z = torch.randn(2, 4, 6, 5)
    ok = dict(model=None, class_counts=(1, 2), z_shape=(4, 6, 5), progress=False)
    bad_calls = [
        dict(mask=torch.ones(6, 5)),                                  # mask needs init_latent
        dict(strength=0.5),                                           # strength needs init_latent
        dict(init_latent=z, strength=0.0),
        dict(init_latent=z, strength=-0.5),
        dict(init_latent=z, strength=1.5),
        dict(init_latent=z, strength=float("nan")),
        dict(init_latent=z[:, :, :, 0]),                              # (2,4,6): a (C,h,w) that is not z_shape
        dict(init_latent=torch.randn(3, 4, 6, 5)),                    # 3 samples for a batch of 2
        dict(init_latent=torch.randn(4, 6, 6)),                       # disagrees with z_shape
        dict(init_latent=torch.randn(6, 5)),                          # not 3-D / 4-D
        dict(init_latent=[[1.0]]),                                    # not a tensor
        dict(init_latent=z, mask=torch.ones(2, 6, 5)),                # (B,h,w) is not an accepted mask shape
        dict(init_latent=z, mask=torch.ones(3, 1, 6, 5)),
        dict(init_latent=z, mask=torch.ones(2, 4, 6, 5)),             # per-channel masks are not supported
        dict(init_latent=z, mask=torch.ones(5, 6)),
        dict(init_latent=z, mask=torch.full((6, 5), 1.5)),
        dict(init_latent=z, mask=torch.full((6, 5), -0.25)),
        dict(init_latent=z, mask=torch.full((6, 5), float("nan"))),
    ]
    for kw in bad_calls:
        for sampler in (dict(), dict(sampler="ddim", steps=4), dict(sampler="dpmpp_2m", steps=4)):
            with pytest.raises(ValueError):
                d.sample_latent_cond(**ok, **sampler, **kw)
    # the rules hold before anything is drawn
    torch.manual_seed(3)
    before = torch.get_rng_state()
    with pytest.raises(ValueError):
        d.sample_latent_cond(**ok, init_latent=z, strength=2.0)
    assert torch.equal(torch.get_rng_state(), before)


def test_shape_comes_from_init_latent_without_the_vae():
    """z_shape None with init_latent: _latent_shape (and its encode draw) is not consulted."""
    d = diff.Diffuser(40)

    def boom(*a, **k):
        raise AssertionError("_latent_shape called")

    d._latent_shape = boom
    seen = {}

    def loop(model, x, *a, **k):
        seen["x"], seen["known"] = x, k.get("known")
        return x

    d._run_cond_loop = loop
    z = torch.randn(4, 6, 5)
    torch.manual_seed(11)
    out = d.sample_latent_cond(None, (1, 3), z_shape=None, vae=None, progress=False, init_latent=z, strength=0.5)
    torch.manual_seed(11)
    assert torch.equal(out, torch.randn(3, 4, 6, 5))  # the one draw of the call, at x_T's place: e0
    z0, m, s = seen["known"]
    assert z0.shape == (3, 4, 6, 5) and m is None and s == 0.5


def test_sharded_and_csv_samplers_take_the_keywords():
    import inspect
    from dmx.distributed import ShardedCondSampler
    from entityCsvSampler import EntityCsvSampler
    for fn in (diff.Diffuser.sample_latent_cond, ShardedCondSampler.sample, EntityCsvSampler.sample):
        ps = inspect.signature(fn).parameters
        for name in ("init_latent", "mask", "strength"):
            assert ps[name].default is None
