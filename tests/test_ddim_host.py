"""CPU-only: the strided (DDIM) schedule, its coefficient tables and the samplers' argument rules.

The tables are restated here in float64 from the definitions (position p = 1..S at index p-1, step
from t = tau_p to s = tau_{p-1}, tau_0 = 0 with alpha_bar 1):
  k_e = sqrt(1-ab[t]), k_a = sqrt(ab[t]), k_s = sqrt(ab[s]),
  k_n = eta sqrt((1-ab[s])/(1-ab[t])) sqrt(1-ab[t]/ab[s]), k_d = sqrt(max(1-ab[s]-k_n^2, 0))."""
import math

import pytest
import torch

import diff


def ceil_schedule(T, S):
    return [-((-i * T) // S) for i in range(1, S + 1)]


def tables64(d, S, eta):
    """float64 restatement, entry by entry, from the Diffuser's fp32 alpha_bars."""
    ab = [1.0] + [float(v) for v in d._host[1].double()]
    tau = ceil_schedule(d.num_timesteps, S)
    rows = []
    for p in range(1, S + 1):
        t, s = tau[p - 1], (tau[p - 2] if p > 1 else 0)
        sigma = eta * math.sqrt((1 - ab[s]) / (1 - ab[t])) * math.sqrt(1 - ab[t] / ab[s])
        rows.append((math.sqrt(1 - ab[t]), math.sqrt(ab[t]), math.sqrt(ab[s]),
                     math.sqrt(max(1 - ab[s] - sigma * sigma, 0.0)), sigma))
    return tau, [torch.tensor(c, dtype=torch.float64) for c in zip(*rows)]


@pytest.mark.parametrize("T,S", [(1000, 50), (1000, 7), (10, 10), (1000, 1)])
def test_ddim_timesteps(T, S):
    d = diff.Diffuser(T)
    tau = d.ddim_timesteps(S)
    assert tau == ceil_schedule(T, S) == [math.ceil(i * T / S) for i in range(1, S + 1)]
    assert len(tau) == S and tau[-1] == T and tau[0] >= 1
    assert all(b > a for a, b in zip(tau, tau[1:]))
    if S == T:
        assert tau == list(range(1, T + 1))
    for bad in (0, T + 1):
        with pytest.raises(ValueError):
            d.ddim_timesteps(bad)


def test_ddim_timesteps_stride_20():
    assert diff.Diffuser(1000).ddim_timesteps(50) == list(range(20, 1001, 20))


@pytest.mark.parametrize("T,S", [(1000, 50), (1000, 7), (10, 10), (1000, 1), (1000, 1000)])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_tables_vs_float64(T, S, eta):
    d = diff.Diffuser(T)
    got = d.ddim_tables(S, eta, "cpu")
    assert len(got) == 6
    tau, exp = tables64(d, S, eta)
    assert got[0].dtype == torch.long and got[0].tolist() == tau
    for name, g, e in zip(("k_e", "k_a", "k_s", "k_d", "k_n"), got[1:], exp):
        assert g.dtype == torch.float32 and g.shape == (S,) and g.is_contiguous()
        # both sides round one float64 value to fp32: within one fp32 ulp
        err = ((g.double() - e).abs() / e.abs().clamp_min(1e-300)).max().item()
        assert err <= 1.2e-7, (name, err)
        assert torch.equal(g == 0, e == 0), name
    k_s, k_n = got[3], got[5]  # (t_map, k_e, k_a, k_s, k_d, k_n)
    assert float(k_s[0]) == 1.0 and float(k_n[0]) == 0.0  # position 1 steps to alpha_bar 1: no noise
    if eta == 0.0:
        assert bool((k_n == 0).all())
    elif S > 1:
        assert bool((k_n[1:] > 0).all())
    assert d.ddim_tables(S, eta, "cpu") is got  # cached per (steps, eta, device)


def test_ddim_tables_argument_errors():
    d = diff.Diffuser(1000)
    for eta in (1.5, -0.1):
        with pytest.raises(ValueError):
            d.ddim_tables(50, eta, "cpu")
    for steps in (0, 1001):
        with pytest.raises(ValueError):
            d.ddim_tables(steps, 0.0, "cpu")


class _NeverCalled:
    """A model that fails the test if the sampler gets as far as running it."""

    def __call__(self, *a, **k):
        raise AssertionError("the sampler ran the model before checking its arguments")

    def eval(self):
        raise AssertionError("the sampler touched the model before checking its arguments")


@pytest.mark.parametrize("kw", [dict(sampler="euler", steps=10), dict(sampler="ddpm", steps=10),
                                dict(sampler="ddim"), dict(sampler="ddim", steps=0),
                                dict(sampler="ddim", steps=41), dict(sampler="ddim", steps=10, eta=1.5)])
def test_sample_latent_cond_argument_errors(kw):
    d = diff.Diffuser(40)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        d.sample_latent_cond(_NeverCalled(), {1: 2}, z_shape=(4, 8, 8), progress=False, **kw)
    assert torch.equal(torch.get_rng_state(), state)  # raised before x_T was drawn


def test_sharded_sampler_argument_errors():
    from dmx import distributed as dd
    d = diff.Diffuser(40)
    s = dd.ShardedCondSampler(d, _NeverCalled(), None)
    state = torch.get_rng_state()
    for kw in (dict(sampler="euler", steps=10), dict(sampler="ddpm", steps=10), dict(sampler="ddim", steps=41)):
        with pytest.raises(ValueError):
            s.sample({1: 2}, z_shape=(4, 8, 8), decode=False, **kw)
    assert torch.equal(torch.get_rng_state(), state)
