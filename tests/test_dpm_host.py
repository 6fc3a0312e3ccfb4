"""CPU-only: the DPM-Solver++(2M) schedule (timesteps uniform in log-SNR, or the DDIM stride), its
coefficient tables and the samplers' argument rules.

Everything is restated here in float64 from the Diffuser's fp32 alpha_bars (ab[0] := 1):
  lam[t] = 0.5 ln(ab[t] / (1 - ab[t]))
  "logsnr" timesteps: grid g_i = lam[1] + (i-1)/(S-1) (lam[T] - lam[1]); c_i the nearest t (ties to the
  smaller); tau_1 = c_1, tau_i = max(c_i, tau_{i-1} + 1); tau_S = T; tau_i = min(tau_i, tau_{i+1} - 1).
  tables, position p = 1..S at index p-1, t = tau_p, s = tau_{p-1} (tau_0 = 0), u = tau_{p+1}:
  k_e = sqrt(1-ab[t]), k_a = sqrt(ab[t]), k_x = sqrt(1-ab[s]) / sqrt(1-ab[t]), m = sqrt(ab[s]) - k_x sqrt(ab[t]),
  first-order rows (p = S, p = 1): k_c = m, k_p = 0; else r = (lam[t]-lam[u]) / (lam[s]-lam[t]),
  k_c = m (1 + 1/(2r)), k_p = -m / (2r)."""
import math

import pytest
import torch

import diff

CASES = [(T, S) for T in (1000, 40) for S in (1, 2, 7, 10, 20, T)]
SPACINGS = ("logsnr", "uniform")


def ab64(d):
    return [1.0] + [float(v) for v in d._host[1].double()]


def lam64(ab, t):
    return 0.5 * math.log(ab[t] / (1 - ab[t]))


def timesteps64(d, S, spacing):
    T = d.num_timesteps
    if spacing == "uniform":
        return [-((-i * T) // S) for i in range(1, S + 1)]
    if S == 1:
        return [T]
    ab = ab64(d)
    lam = [None] + [lam64(ab, t) for t in range(1, T + 1)]
    tau = []
    for i in range(1, S + 1):
        g = lam[1] + (i - 1) / (S - 1) * (lam[T] - lam[1])
        best, c = None, None
        for t in range(1, T + 1):
            dist = abs(lam[t] - g)
            if best is None or dist < best:  # strict: ties stay with the smaller t
                best, c = dist, t
        tau.append(c if not tau else max(c, tau[-1] + 1))
    tau[-1] = T
    for i in range(S - 2, -1, -1):
        tau[i] = min(tau[i], tau[i + 1] - 1)
    return tau


def tables64(d, S, spacing):
    ab = ab64(d)
    tau = timesteps64(d, S, spacing)
    rows = []
    for p in range(1, S + 1):
        t, s = tau[p - 1], (tau[p - 2] if p > 1 else 0)
        k_e, k_a = math.sqrt(1 - ab[t]), math.sqrt(ab[t])
        k_x = math.sqrt(1 - ab[s]) / math.sqrt(1 - ab[t])
        m = math.sqrt(ab[s]) - k_x * math.sqrt(ab[t])
        if p == 1 or p == S:
            k_c, k_p = m, 0.0
        else:
            u = tau[p]
            r = (lam64(ab, t) - lam64(ab, u)) / (lam64(ab, s) - lam64(ab, t))
            k_c, k_p = m * (1 + 1 / (2 * r)), -m / (2 * r)
        rows.append((k_e, k_a, k_x, k_c, k_p))
    return tau, [torch.tensor(c, dtype=torch.float64) for c in zip(*rows)]


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("T,S", CASES)
def test_dpm_timesteps(T, S, spacing):
    d = diff.Diffuser(T)
    tau = d.dpm_timesteps(S, spacing)
    assert tau == timesteps64(d, S, spacing)
    assert len(tau) == S and tau[-1] == T and tau[0] >= 1
    assert all(b > a for a, b in zip(tau, tau[1:]))
    if spacing == "logsnr":
        if S >= 2:
            assert tau[0] == 1
        if S == T:
            assert tau == list(range(1, T + 1))
    else:
        assert tau == d.ddim_timesteps(S)


def test_dpm_timesteps_logsnr_T1000_S10():
    d = diff.Diffuser(1000)
    tau = d.dpm_timesteps(10, "logsnr")
    print(f"[dpm timesteps T=1000 S=10 logsnr] {tau}")
    assert tau == timesteps64(d, 10, "logsnr")  # the restatement decides
    assert tau == [1, 6, 23, 74, 203, 411, 604, 758, 887, 1000]


def test_dpm_timesteps_argument_errors():
    d = diff.Diffuser(40)
    for bad in (0, 41):
        for spacing in SPACINGS:
            with pytest.raises(ValueError):
                d.dpm_timesteps(bad, spacing)
    with pytest.raises(ValueError):
        d.dpm_timesteps(10, "karras")
    with pytest.raises(ValueError):
        d.dpm_tables(10, "karras", "cpu")


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("T,S", CASES)
def test_dpm_tables_vs_float64(T, S, spacing):
    d = diff.Diffuser(T)
    got = d.dpm_tables(S, spacing, "cpu")
    assert isinstance(got, tuple) and len(got) == 6
    tau, exp = tables64(d, S, spacing)
    assert got[0].dtype == torch.long and got[0].tolist() == tau and got[0].device.type == "cpu"
    for name, g, e in zip(("k_e", "k_a", "k_x", "k_c", "k_p"), got[1:], exp):
        assert g.dtype == torch.float32 and g.shape == (S,) and g.is_contiguous() and g.device.type == "cpu"
        assert torch.equal(g, e.float()), name  # the float64 value, rounded to fp32 once
    _, k_e, k_a, k_x, k_c, k_p = got
    first_order = torch.zeros(S, dtype=torch.bool)
    first_order[0] = first_order[S - 1] = True  # p = 1 and p = S
    assert torch.equal(k_p == 0, first_order)
    assert float(k_x[0]) == 0.0 and float(k_c[0]) == 1.0  # position 1 steps to alpha_bar 1: x' = x0
    if spacing == "uniform":
        ddim = d.ddim_tables(S, 0.0, "cpu")
        assert torch.equal(got[0], ddim[0]) and torch.equal(k_e, ddim[1]) and torch.equal(k_a, ddim[2])
    else:  # the same bits as the DDIM rows of the same timesteps (full stride: row t - 1)
        full = d.ddim_tables(T, 0.0, "cpu")
        assert torch.equal(k_e, full[1][got[0] - 1]) and torch.equal(k_a, full[2][got[0] - 1])
    assert d.dpm_tables(S, spacing, "cpu") is got  # cached per (steps, spacing, device)


def test_dpm_tables_are_not_a_plain_tuple():
    """A plain 6-tuple keeps meaning DDIM: the DPM tables carry their own type."""
    from dmx import engine
    d = diff.Diffuser(40)
    assert isinstance(d.dpm_tables(7, "logsnr", "cpu"), engine.DpmSchedule)
    assert type(d.ddim_tables(7, 0.0, "cpu")) is tuple


class _NeverCalled:
    """A model that fails the test if the sampler gets as far as running it."""

    def __call__(self, *a, **k):
        raise AssertionError("the sampler ran the model before checking its arguments")

    def eval(self):
        raise AssertionError("the sampler touched the model before checking its arguments")


BAD = [dict(sampler="dpmpp_2m"), dict(sampler="dpmpp_2m", steps=0), dict(sampler="dpmpp_2m", steps=41),
       dict(sampler="dpmpp_2m", steps=10, eta=0.5), dict(sampler="dpmpp_2m", steps=10, spacing="karras"),
       dict(sampler="ddim", steps=10, spacing="logsnr"), dict(sampler="ddpm", spacing="uniform"),
       dict(sampler="euler", steps=10)]


@pytest.mark.parametrize("kw", BAD)
def test_sample_latent_cond_argument_errors(kw):
    d = diff.Diffuser(40)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        d.sample_latent_cond(_NeverCalled(), {1: 2}, z_shape=(4, 8, 8), progress=False, **kw)
    assert torch.equal(torch.get_rng_state(), state)  # raised before x_T was drawn


@pytest.mark.parametrize("kw", BAD)
def test_sharded_sampler_argument_errors(kw):
    from dmx import distributed as dd
    d = diff.Diffuser(40)
    s = dd.ShardedCondSampler(d, _NeverCalled(), None)
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        s.sample({1: 2}, z_shape=(4, 8, 8), decode=False, **kw)
    assert torch.equal(torch.get_rng_state(), state)
