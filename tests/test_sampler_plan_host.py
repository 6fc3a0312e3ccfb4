"""CPU-only: the calls the samplers make on the native model — which entry, at which position, how many
steps, with which guidance and which keywords — pinned as lists written out by hand.

ShardedCondSampler.sample runs at world size 1 on the CPU against a recording stub (a model with
_dmx_kind = 2 whose native() accepts every keyword).  Diffuser(40), GUARD_CHUNK = 4, z_shape (2, 8, 8),
three samples: a loop of 6 positions runs as the chunks 6..3 and 2..1, the 40 timesteps of DDPM as ten
chunks of four.  A feature that is off passes no keyword."""
import contextlib

import pytest
import torch

import diff
from dmx.distributed import ShardedCondSampler

COUNTS = {1: 2, 3: 1}
Z = (2, 8, 8)
LOOP = ("sample_offset", "seed", "use_graph")  # what every sample_loop call carries


class _RecNative:
    """Records every call; the step halves x (and leaves x in hist), so a restored chunk is visible."""

    def __init__(self, trips=()):
        self.precision = "x3"
        self.flag = False
        self.trips = trips        # positions on entry at which an x3 call raises the range flag
        self.calls, self.seen = [], []

    def _record(self, method, pos, steps, g, kw, x, y, v, m, noise):
        self.calls.append((method, pos, steps, float(g), tuple(sorted(kw))))
        hist = kw.get("hist")
        self.seen.append(dict(x=x.clone(), y=y, v=v, m=m, noise=None if noise is None else noise.clone(),
                              seed=kw.get("seed"), precision=self.precision,
                              hist=None if hist is None else hist.clone()))
        if self.precision == "x3" and pos in self.trips:
            self.flag = True
        if hist is not None:
            hist.copy_(x)

    def step(self, xs, out, tt, y, null_label, v, m, g, tables, noise=None, **kw):
        assert int(tt.min()) == int(tt.max())
        self._record("step", int(tt[0]), 1, g, kw, xs, y, v, m, noise)
        out.copy_(0.5 * xs + (0 if noise is None else 0.1 * noise))

    def sample_loop(self, x, t_dev, y, null_label, v, m, g, tables, steps, **kw):
        self._record("sample_loop", int(t_dev), steps, g, kw, x, y, v, m, None)
        x.mul_(0.5 ** steps)
        t_dev.sub_(steps)

    def range_tripped(self, reset=True):
        f = self.flag
        if reset:
            self.flag = False
        return f

    @contextlib.contextmanager
    def precision_override(self, prec):
        old, self.precision = self.precision, prec
        try:
            yield self
        finally:
            self.precision = old


class _RecModel:
    _dmx_kind = 2

    def __init__(self, trips=()):
        self._n = _RecNative(trips)

    def native(self):
        return self._n


def _sample(noise_source, trips=(), seed=3, **kw):
    d = diff.Diffuser(40)
    d.GUARD_CHUNK = 4
    d.noise_source = noise_source
    model = _RecModel(trips)
    s = ShardedCondSampler(d, model, None)
    torch.manual_seed(seed)
    out = s.sample(COUNTS, z_shape=Z, decode=False, **kw)
    assert out.shape == (3,) + Z
    return d, s, model.native()


def _kw(*names):
    return tuple(sorted(names))


def test_ddim_interval_cuts_the_device_loop_into_segments():
    tau = diff.Diffuser(40).ddim_timesteps(6)
    base = dict(sampler="ddim", steps=6, eta=0.0, guidance_interval=(tau[2], tau[4]))  # positions 3..5 guided
    _, _, nm = _sample("device", **base)
    assert nm.calls == [("sample_loop", 6, 1, 0.0, _kw(*LOOP, "sched")),
                        ("sample_loop", 5, 3, 3.0, _kw(*LOOP, "sched")),
                        ("sample_loop", 2, 2, 0.0, _kw(*LOOP, "sched"))]
    seeds = {c["seed"] for c in nm.seen}
    assert len(seeds) == 1 and seeds != {0}  # one seed per call, drawn even though eta = 0 draws no noise
    _, _, nm = _sample("device", guidance_rescale=0.5, **base)
    assert nm.calls == [("sample_loop", 6, 1, 0.0, _kw(*LOOP, "sched")),
                        ("sample_loop", 5, 3, 3.0, _kw(*LOOP, "sched", "rescale")),
                        ("sample_loop", 2, 2, 0.0, _kw(*LOOP, "sched"))]


def test_ddim_interval_on_the_host_loop():
    tau = diff.Diffuser(40).ddim_timesteps(6)
    base = dict(sampler="ddim", steps=6, eta=0.0, guidance_interval=(tau[2], tau[4]))
    _, _, nm = _sample("host", **base)
    assert nm.calls == [("step", 6, 1, 0.0, _kw("sched")),
                        ("step", 5, 1, 3.0, _kw("sched")),
                        ("step", 4, 1, 3.0, _kw("sched")),
                        ("step", 3, 1, 3.0, _kw("sched")),
                        ("step", 2, 1, 0.0, _kw("sched")),
                        ("step", 1, 1, 0.0, _kw("sched"))]
    assert all(c["noise"] is None for c in nm.seen)  # eta = 0: nothing is drawn per step
    _, _, nm = _sample("host", guidance_rescale=0.5, **base)
    assert [c[4] for c in nm.calls] == [_kw("sched")] + [_kw("sched", "rescale")] * 3 + [_kw("sched")] * 2


def test_ddpm_defaults_pass_no_optional_keyword():
    _, _, nm = _sample("device")
    assert nm.calls == [("sample_loop", p, 4, 3.0, _kw(*LOOP)) for p in (40, 36, 32, 28, 24, 20, 16, 12, 8, 4)]
    _, _, nm = _sample("host")
    assert nm.calls == [("step", p, 1, 3.0, ()) for p in range(40, 0, -1)]
    assert all(c["noise"] is not None and c["noise"].shape == (3,) + Z for c in nm.seen)


@pytest.mark.parametrize("noise_source", ["device", "host"])
def test_dpm_draws_nothing_after_x_T(noise_source):
    _, _, nm = _sample(noise_source, seed=9, sampler="dpmpp_2m", steps=6)
    after = torch.get_rng_state()
    if noise_source == "device":
        assert nm.calls == [("sample_loop", 6, 4, 3.0, _kw(*LOOP, "sched", "hist")),
                            ("sample_loop", 2, 2, 3.0, _kw(*LOOP, "sched", "hist"))]
        assert [c["seed"] for c in nm.seen] == [0, 0]
    else:
        assert nm.calls == [("step", p, 1, 3.0, _kw("sched", "hist")) for p in (6, 5, 4, 3, 2, 1)]
        assert all(c["noise"] is None for c in nm.seen)
    torch.manual_seed(9)
    torch.randn((3,) + Z)  # x_T alone
    assert torch.equal(after, torch.get_rng_state())


@pytest.mark.parametrize("noise_source", ["device", "host"])
def test_composed_call_passes_compose_and_no_scale(noise_source):
    d, _, nm = _sample(noise_source, base="dropped")
    if noise_source == "device":
        assert nm.calls == [("sample_loop", p, 4, 0.0, _kw(*LOOP, "compose")) for p in range(40, 0, -4)]
    else:
        assert nm.calls == [("step", p, 1, 0.0, _kw("compose")) for p in range(40, 0, -1)]
    vals, msk = d._build_cond([1, 1, 3], None, None, None, None, "cpu")
    for c in nm.seen:  # the call's own labels and condition rows still go along
        assert torch.equal(c["y"], torch.tensor([1, 1, 3]))
        assert torch.equal(c["v"], vals.float()) and torch.equal(c["m"], msk.float())


def _blend_cpu(x, pos, known, out=None):
    """engine.known_blend restated in torch (the kernel needs a GPU)."""
    z0, e0, mask, q_a, q_e = known
    p = pos.reshape(-1).long().clamp(1, q_a.numel()) - 1
    kn = q_a[p].view(-1, 1, 1, 1) * z0 + q_e[p].view(-1, 1, 1, 1) * e0
    r = kn if mask is None else mask * x + (1 - mask) * kn
    if out is None:
        return r.clone()
    out.copy_(r)
    return out


@pytest.mark.parametrize("sampler,extra", [("ddim", ()), ("dpmpp_2m", ("hist",))])
def test_known_region_loop_enters_at_p0(monkeypatch, sampler, extra):
    monkeypatch.setattr(diff._engine, "known_blend", _blend_cpu)
    g = torch.Generator().manual_seed(1)
    z0 = torch.randn((3,) + Z, generator=g)
    mask = (torch.rand((8, 8), generator=g) > 0.5).float()
    kw = dict(sampler=sampler, steps=6, init_latent=z0, mask=mask, strength=0.5)  # p0 = floor(0.5 * 6 + 0.5) = 3
    _, _, nm = _sample("device", **kw)
    assert nm.calls == [("sample_loop", 3, 3, 3.0, _kw(*LOOP, "sched", "known", *extra))]
    _, _, nm = _sample("host", **kw)
    assert nm.calls == [("step", p, 1, 3.0, _kw("sched", "known", *extra)) for p in (3, 2, 1)]
    torch.manual_seed(3)
    e0 = torch.randn((3,) + Z)
    tau = diff.Diffuser(40).ddim_timesteps(6) if sampler == "ddim" else diff.Diffuser(40).dpm_timesteps(6)
    ab = diff.Diffuser(40)._host[1].double()[tau[2] - 1]  # the loop starts from z0 noised to tau_3 under e0
    start = (torch.sqrt(ab) * z0.double() + torch.sqrt(1 - ab) * e0.double()).float()
    assert torch.allclose(nm.seen[0]["x"], start, rtol=0, atol=1e-6)


@pytest.mark.parametrize("noise_source,kw", [("device", dict(sampler="dpmpp_2m", steps=6)),
                                             ("host", dict(sampler="dpmpp_2m", steps=6)),
                                             ("host", dict(sampler="ddim", steps=6, eta=0.5))])
def test_range_trip_replays_the_chunk_in_fp32(noise_source, kw):
    """The second chunk (positions 2, 1) trips: its calls appear twice, the second time in fp32 from the
    same x, solver history and CPU-generator state (hence the same draws); one fallback is counted."""
    d, s, nm = _sample(noise_source, trips=(2,), **kw)
    extra = ("hist",) if kw["sampler"] == "dpmpp_2m" else ()
    if noise_source == "device":
        assert nm.calls == [("sample_loop", 6, 4, 3.0, _kw(*LOOP, "sched", *extra)),
                            ("sample_loop", 2, 2, 3.0, _kw(*LOOP, "sched", *extra)),
                            ("sample_loop", 2, 2, 3.0, _kw(*LOOP, "sched", *extra))]
        first, again = nm.seen[1:2], nm.seen[2:3]
    else:
        assert nm.calls == [("step", p, 1, 3.0, _kw("sched", *extra)) for p in (6, 5, 4, 3, 2, 1, 2, 1)]
        first, again = nm.seen[4:6], nm.seen[6:8]
    assert [c["precision"] for c in nm.seen] == ["x3"] * (len(nm.seen) - len(again)) + ["fp32"] * len(again)
    for a, b in zip(first, again):
        assert torch.equal(a["x"], b["x"])
        if extra:
            assert torch.equal(a["hist"], b["hist"])
        assert (a["noise"] is None) == (b["noise"] is None)
        if a["noise"] is not None:
            assert torch.equal(a["noise"], b["noise"])
    if kw.get("eta"):
        assert all(c["noise"] is not None for c in nm.seen)
    assert s.range_fallbacks == 1 and d.range_fallbacks == 0
    assert nm.precision == "x3" and not nm.flag
