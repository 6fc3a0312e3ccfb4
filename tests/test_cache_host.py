"""CPU-only: feature caching — the oracle of a cached step, the argument rules of the
samplers' cache_interval keyword, the refresh positions under the guard-chunk rule, the header and
bindings, and the graph-key program.

Definitions.  The deep feature D of a forward is the output of sa5, the upsampled input of up3:
(rows, 64, h/2, w/2) here (NCHW, as the oracle works), (rows, h/2, w/2, 64) in the engine.  A refresh
step is the full forward and keeps D; a reuse step runs inc, up3, sa6 and the head on a kept D.
Inside a guard chunk i_from .. i_to + 1 the step at position p refreshes iff (i_from - p) % N == 0.

This module also holds the oracle that tests/test_gpu_cache.py compares the GPU against: full() and
shallow(), restated from oracle.ref's block functions, and the trajectory restatements built on them.

Measured here (synthetic weights, CFG 3.0, fp32 torch CPU): a reuse step at (x_b, t = 431) on the D of
(x_a, t = 731), x_b independent of x_a, B = 2 at 16x16, differs from the full step's eps by rel-L2 0.61;
the GPU tests' cases (t = 440 on the D of t = 740, 28x28 and 32x32, B = 2 .. 32) by 0.28 - 0.54, and their
cached DDIM trajectories (S = 6, N = 2 and 3) differ from the uncached ones by 0.063 - 0.077."""
import inspect
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import diff
from conftest import REPO
from oracle import ref
from oracle.rules import rel


# ---- the oracle of a cached step -------------------------------------------------------------------
def full(sd, x, emb):
    """ref.unet_trunk, also returning what up3 takes as its x -> (eps, D)."""
    x1 = ref.resblock(sd, "inc", x, False)
    x2 = ref.attention(sd, "sa1", ref.down(sd, "down1", x1, emb))
    x3 = ref.attention(sd, "sa2", ref.down(sd, "down2", x2, emb))
    x4 = ref.attention(sd, "sa3", ref.down(sd, "down3", x3, emb))
    x4 = ref.resblock(sd, "bot1", x4, False)
    x4 = ref.resblock(sd, "bot2", x4, False)
    x4 = ref.resblock(sd, "bot3", x4, False)
    h = ref.attention(sd, "sa4", ref.up(sd, "up1", x4, x3, emb))
    D = ref.attention(sd, "sa5", ref.up(sd, "up2", h, x2, emb))
    feat = ref.attention(sd, "sa6", ref.up(sd, "up3", D, x1, emb))
    return F.conv2d(feat, sd["out.weight"], sd["out.bias"]), D


def shallow(sd, x, emb, D):
    """The reuse step's network: inc, up3 and sa6 on the kept D, the head -> eps."""
    x1 = ref.resblock(sd, "inc", x, False)
    feat = ref.attention(sd, "sa6", ref.up(sd, "up3", D, x1, emb))
    return F.conv2d(feat, sd["out.weight"], sd["out.bias"])


class CachedEps:
    """The prediction of a step on the oracle network, CFG halves each with their own D: eps(x, t,
    refresh) runs full() on a refresh step (keeping both D) and shallow() on the kept ones otherwise.
    guidance 0: one conditional forward, one D."""

    def __init__(self, sd, y, vals, mask, guidance=3.0, null_label=0):
        self.sd, self.y, self.vals, self.mask, self.g, self.null = sd, y, vals, mask, float(guidance), null_label
        self.D = None

    def _embs(self, t):
        ec = ref.cond_embedding(self.sd, t, self.y, self.vals, self.mask)
        if not self.g > 0:
            return [ec]
        return [ref.cond_embedding(self.sd, t, torch.full_like(self.y, self.null), self.vals, self.mask), ec]

    def _mix(self, es):
        return es[0] if len(es) == 1 else es[0] + self.g * (es[1] - es[0])

    def __call__(self, x, t, refresh=True):
        with torch.no_grad():
            embs = self._embs(t)
            if refresh:
                outs = [full(self.sd, x, e) for e in embs]
                self.D = [o[1] for o in outs]
                return self._mix([o[0] for o in outs])
            return self._mix([shallow(self.sd, x, e, D) for e, D in zip(embs, self.D)])

    def features(self):
        """The kept D as the engine stores it: (rows, h/2, w/2, 64), null half first."""
        return torch.cat(self.D).permute(0, 2, 3, 1).contiguous()


def refresh_positions(start, n, chunk):
    """The rule, spelled out: the positions start .. 1 are walked in guard chunks i_from .. i_to + 1 of
    `chunk` positions, and position p of a chunk refreshes iff (i_from - p) % n == 0."""
    out, i_from = [], int(start)
    while i_from >= 1:
        i_to = max(i_from - int(chunk), 0)
        out += [p for p in range(i_from, i_to, -1) if (i_from - p) % int(n) == 0]
        i_from = i_to
    return out


def cached_trajectory(eps_of, x, start, n, chunk, update):
    """Positions start .. 1 from x under cache_interval n in guard chunks of `chunk`: update(x, eps, p) is
    the rule's update at position p, eps_of(x, p, refresh) the prediction.  n = 1: the uncached loop."""
    marks = set(refresh_positions(start, n, chunk))
    for p in range(int(start), 0, -1):
        x = update(x, eps_of(x, p, p in marks), p)
    return x


def step_inputs(B, hw, seed):
    """(x_a, x_b, y, vals, mask): two independent latents and one condition."""
    g = torch.Generator().manual_seed(seed)
    x_a = torch.randn((B, 4, hw, hw), generator=g)
    x_b = torch.randn((B, 4, hw, hw), generator=g)
    y = torch.tensor([1 + (i % 3) for i in range(B)])
    vals = torch.rand((B, 12), generator=g)
    mask = (torch.rand((B, 12), generator=g) > 0.3).float()
    return x_a, x_b, y, vals, mask


# ---- 1: the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [16, 28])
def test_oracle_full_and_shallow_are_the_trunk_bit_for_bit(unet_sd, hw):
    x_a, x_b, y, vals, mask = step_inputs(2, hw, 3)
    with torch.no_grad():
        emb = ref.cond_embedding(unet_sd, torch.tensor([731, 12]), y, vals, mask)
        eps_ref, _ = ref.unet_trunk(unet_sd, x_a, emb)
        eps, D = full(unet_sd, x_a, emb)
        assert torch.equal(eps, eps_ref)
        assert tuple(D.shape) == (2, 64, hw // 2, hw // 2)
        assert torch.equal(shallow(unet_sd, x_a, emb, D), eps)
        # another step's D is another prediction
        emb_b = ref.cond_embedding(unet_sd, torch.tensor([431, 431]), y, vals, mask)
        eps_b, _ = full(unet_sd, x_b, emb_b)
        assert rel(shallow(unet_sd, x_b, emb_b, D), eps_b) > 1e-2


def test_oracle_reuse_step_differs_from_the_full_step(unet_sd):
    x_a, x_b, y, vals, mask = step_inputs(2, 16, 4)
    e = CachedEps(unet_sd, y, vals, mask, 3.0)
    e(x_a, torch.full((2,), 731), True)
    assert tuple(e.features().shape) == (4, 8, 8, 64)
    cached = e(x_b, torch.full((2,), 431), False)
    plain = CachedEps(unet_sd, y, vals, mask, 3.0)(x_b, torch.full((2,), 431), True)
    d = rel(cached, plain)
    print(f"[cache oracle] reuse vs full eps at b: rel-L2 = {d:.3e}")
    assert d > 1e-2


# ---- 2: argument rules ---------------------------------------------------------------------------------
def test_cache_interval_refusals_name_both_parties():
    d = diff.Diffuser(40)
    ok = dict(model=None, class_counts=(1, 2), z_shape=(4, 6, 5), progress=False, cache_interval=3)
    spec = dict(classes=2, cond=None, cond_mask=None, weight=1.0)
    cases = [
        (dict(base="dropped"), "composed"), (dict(also=[spec]), "composed"),
        (dict(guidance_scale=[3.0, 2.0]), "composed"),
        (dict(guidance_interval=(1, 20)), "guidance_interval"),
        # the ddpm sampler's unguided loop goes through the module's forward: refused before the x_T draw
        (dict(guidance_scale=0.0), "guidance_scale"), (dict(guidance_scale=None), "guidance_scale"),
        (dict(guidance_scale=0), "ddpm"),
    ]
    torch.manual_seed(3)
    before = torch.get_rng_state()
    for kw, word in cases:
        with pytest.raises(ValueError) as ei:
            d.sample_latent_cond(**ok, **kw)
        assert "cache_interval" in str(ei.value) and word in str(ei.value), (kw, str(ei.value))
    for bad in (0, -1, 2.0, "3", True, (3,)):
        with pytest.raises(ValueError) as ei:
            d.sample_latent_cond(**{**ok, "cache_interval": bad})
        assert "cache_interval" in str(ei.value)
    assert torch.equal(torch.get_rng_state(), before)
    # the parts that need a model to be accepted at all: checked on the rule itself
    for kw, word in ((dict(pag=True), "pag_scale"), (dict(geom=True), "geom_scale"), (dict(composed=True), "composed"),
                     (dict(guidance_interval=(1, 2)), "guidance_interval")):
        with pytest.raises(ValueError) as ei:
            d._cache_args(3, **kw)
        assert "cache_interval" in str(ei.value) and word in str(ei.value)

    class Foreign(torch.nn.Module):
        def forward(self, x, t, y, cond_vals=None, cond_mask=None):
            raise AssertionError("the model was touched")

    with pytest.raises(ValueError) as ei:
        d.sample_latent_cond(**{**ok, "model": Foreign()})
    assert "cache_interval" in str(ei.value) and "foreign" in str(ei.value)
    assert torch.equal(torch.get_rng_state(), before)
    with pytest.raises(ValueError) as ei:
        d._cache_args(3, unguided_ddpm=True)
    assert "cache_interval" in str(ei.value) and "ddpm" in str(ei.value)
    assert d._cache_args(None) == 1 and d._cache_args(1) == 1 and d._cache_args(4) == 4
    assert d._cache_args(1, unguided_ddpm=True) == 1
    assert d._cache_args(1, composed=True, pag=True, geom=True, guidance_interval=(1, 2)) == 1  # no request: no rule


def test_plan_carries_the_interval_and_passes_it_only_when_on():
    d = diff.Diffuser(1000)
    x = torch.randn(2, 4, 6, 5)
    for mode in (None, ("ddim", 20, 0.0), ("dpm", 20, "logsnr")):
        plain = d._plan(x, mode, 3.0)
        assert plain.cache == 1
        one = d._plan(x, mode, 3.0, cache=1)
        assert one.cache == 1 and "cache" not in one.kwargs(True, seed=0, use_graph=True)
        assert one.kwargs(True, seed=0, use_graph=True, phase=5) == plain.kwargs(True, seed=0, use_graph=True)
        plan = d._plan(x, mode, 3.0, cache=3)
        assert plan.cache == 3
        assert plan.kwargs(True, seed=0, use_graph=True)["cache"] == (3, 0)
        assert plan.kwargs(True, phase=4)["cache"] == (3, 4)
        rest = {k: v for k, v in plan.kwargs(True, seed=0, use_graph=True).items() if k != "cache"}
        assert rest == plain.kwargs(True, seed=0, use_graph=True)
    for bad in (dict(cache=0), dict(cache=2.0), dict(cache=True), dict(cache=3, interval=(1, 500)),
                dict(cache=3, geom=torch.ones(2))):
        with pytest.raises(ValueError):
            d._plan(x, None, 3.0, **bad)
    with pytest.raises(ValueError) as ei:
        d._plan(x, ("invert", 20, None, 0), 3.0, cache=3)
    assert "cache" in str(ei.value) and "inversion" in str(ei.value)
    comp = d._compose_args([1, 2], torch.zeros(2, 12), torch.zeros(2, 12), 3.0, base="dropped")
    with pytest.raises(ValueError) as ei:
        d._plan(x, None, 3.0, compose=comp, cache=3)
    assert "cache" in str(ei.value) and "composition" in str(ei.value)


def test_the_samplers_carry_the_keyword_and_the_loop_receives_it():
    import entityCsvSampler
    from dmx import distributed, engine
    for fn in (diff.Diffuser.sample_latent_cond, entityCsvSampler.EntityCsvSampler.sample,
               distributed.ShardedCondSampler.sample):
        p = inspect.signature(fn).parameters["cache_interval"]
        assert p.default is None
    for fn in (engine.NativeModel.step, engine.NativeModel.sample_loop):
        assert inspect.signature(fn).parameters["cache"].default is None
    assert callable(engine.NativeModel.cached_features)
    d = diff.Diffuser(40)
    seen = {}

    def loop(model, x, *a, **k):
        seen["kw"] = k
        return x

    d._run_cond_loop = loop
    d.sample_latent_cond(None, (1, 2), z_shape=(4, 6, 5), progress=False, cache_interval=4)
    assert seen["kw"]["cache"] == 4
    for off in (None, 1):
        d.sample_latent_cond(None, (1, 2), z_shape=(4, 6, 5), progress=False, cache_interval=off)
        assert "cache" not in seen["kw"]
    d.sample_latent_cond(None, (1, 2), z_shape=(4, 6, 5), progress=False)
    assert "cache" not in seen["kw"]


def test_csv_and_sharded_samplers_pass_the_keyword_on_and_refuse_alike():
    from dmx import distributed
    from entityCsvSampler import EntityCsvSampler
    seen = {}

    class Rec:
        def sample_latent_cond(self, **kw):
            seen.update(kw)
            return "out"

    s = EntityCsvSampler.__new__(EntityCsvSampler)
    s.diffuser, s.model, s.vae, s.class_id = Rec(), None, None, 1
    s._rows = lambda *a: (torch.zeros(2, 12), torch.zeros(2, 12))
    assert s.sample("rows.csv", cache_interval=3) == "out" and seen["cache_interval"] == 3
    seen.clear()
    s.sample("rows.csv")
    assert "cache_interval" not in seen  # without the keyword the call is what it was
    d = diff.Diffuser(40)
    torch.manual_seed(3)
    before = torch.get_rng_state()
    for kw, word in ((dict(base="dropped"), "composed"), (dict(guidance_interval=(1, 20)), "guidance_interval"),
                     (dict(cache_interval=0), "cache_interval"), (dict(guidance_scale=0.0), "ddpm")):
        with pytest.raises(ValueError) as ei:
            distributed.ShardedCondSampler(d, object(), None).sample({1: 2, 2: 1}, z_shape=(4, 8, 8), decode=False,
                                                                     **{"cache_interval": 3, **kw})
        assert "cache_interval" in str(ei.value) and word in str(ei.value)
    assert torch.equal(torch.get_rng_state(), before)


def test_native_cache_argument_rules():
    from dmx.engine import NativeModel
    assert NativeModel._cache(None, None, None, None, None) is None
    assert NativeModel._cache((1, 0), None, None, None, None) is None
    assert NativeModel._cache((1, 7), object(), object(), object(), object()) is None  # no request: no rule
    c = NativeModel._cache((3, 2), None, None, None, None)
    assert (c.interval, c.phase) == (3, 2)
    for bad in (3, (3,), (0, 0), (3, -1), (2.0, 0), (True, 0), (3, 1.0)):
        with pytest.raises(ValueError):
            NativeModel._cache(bad, None, None, None, None)
    for i, nm in enumerate(("compose", "geom", "perturb", "invert")):
        parts = [None] * 4
        parts[i] = object()
        with pytest.raises(ValueError) as ei:
            NativeModel._cache((3, 0), *parts)
        assert "cached" in str(ei.value) and nm in str(ei.value)


# ---- 3: refresh positions ----------------------------------------------------------------------------
@pytest.mark.parametrize("start,n,chunk", [(10, 3, 4), (7, 3, 50), (6, 2, 50), (12, 4, 50), (1000, 3, 50), (9, 5, 3),
                                           (5, 2, 2), (50, 7, 50), (51, 7, 50)])
@pytest.mark.parametrize("loop", ["host", "device"])
def test_refresh_positions_against_brute_force(start, n, chunk, loop):
    """What the samplers' loops ask of the engine — the phase per step (host loop), (steps, phase 0) per
    chunk call (device loop) — against the rule spelled out position by position."""
    d = diff.Diffuser(1000)
    d.GUARD_CHUNK = chunk
    x = torch.zeros(2, 4, 8, 8)
    plan = d._plan(x, ("ddim", start, 0.0), 3.0, cache=n)
    got, firsts = [], []
    if loop == "host":
        def fake_step(model, x, pos, plan, guided, *a, phase=None, **k):
            if plan.kwargs(guided, phase=phase)["cache"][1] % n == 0:  # (as the engine decides it: (phase + 0) % N)
                got.append(int(pos[0]))
            if phase == 0:
                firsts.append(int(pos[0]))
            return x

        d._step = fake_step
        d._run_cond_loop(None, x, torch.tensor([1, 2]), torch.zeros(2, 12), torch.zeros(2, 12), 3.0, 0, False,
                         ("ddim", start, 0.0), cache=n)
    else:
        class Loop:
            def sample_loop(self, x, t_dev, y, null_label, vals, msk, guidance, tables, steps, **kw):
                i_from, (N, phase) = int(t_dev.item()), kw["cache"]
                got.extend(i_from - k for k in range(steps) if (phase + k) % N == 0)
                firsts.append(i_from)
                t_dev -= steps

        d._guarded_loop(d._device_chunks(Loop(), plan, x, None, 0, None, None, None, 0), x, plan.start, None, inplace=True)
    want = refresh_positions(start, n, chunk)
    assert got == want
    chunks = list(range(start, 0, -chunk))
    assert firsts == chunks and all(p in want for p in chunks)  # every chunk begins with a refresh


def test_host_loop_passes_the_offset_in_the_chunk_and_the_device_loop_zero():
    d = diff.Diffuser(1000)
    d.GUARD_CHUNK = 4
    x = torch.zeros(2, 4, 8, 8)
    phases = []

    def fake_step(model, x, pos, plan, guided, *a, phase=None, **k):
        phases.append((int(pos[0]), phase))
        return x

    d._step = fake_step
    d._run_cond_loop(None, x, torch.tensor([1, 2]), torch.zeros(2, 12), torch.zeros(2, 12), 3.0, 0, False,
                     ("ddim", 10, 0.0), cache=3)
    assert phases == [(10, 0), (9, 1), (8, 2), (7, 3), (6, 0), (5, 1), (4, 2), (3, 3), (2, 0), (1, 1)]
    assert [p for p, ph in phases if ph % 3 == 0] == refresh_positions(10, 3, 4) == [10, 7, 6, 3, 2]
    phases.clear()
    d._run_cond_loop(None, x, torch.tensor([1, 2]), torch.zeros(2, 12), torch.zeros(2, 12), 3.0, 0, False,
                     ("ddim", 10, 0.0))
    assert all(ph is None for _, ph in phases)  # without the keyword _step is called as it always was

    class Loop:
        calls = []

        def sample_loop(self, x, t_dev, y, null_label, vals, msk, guidance, tables, steps, **kw):
            self.calls.append((steps, kw.get("cache")))

    plan = d._plan(x, ("ddim", 10, 0.0), 3.0, cache=3)
    nm = Loop()
    run = d._device_chunks(nm, plan, x, None, 0, None, None, None, 0)
    d._guarded_loop(run, x, plan.start, None, inplace=True)
    assert nm.calls == [(4, (3, 0)), (4, (3, 0)), (2, (3, 0))]


# ---- 4: header and bindings --------------------------------------------------------------------------
def test_header_and_bindings_name_the_new_symbols():
    from dmx import _lib
    src = open(os.path.join(REPO, "include", "dmx.h")).read()
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for sym in ("dmx_step_cached", "dmx_sample_loop_cached", "dmx_model_cached_features"):
        assert sym in src and sym in bound
    assert "typedef struct dmx_cache" in src and "int interval;" in src and "int phase;" in src
    assert [f[0] for f in _lib.Cache._fields_] == ["interval", "phase"]
    assert _lib.load().dmx_abi_version() == 1  # additive: the version stays


# ---- 5: the graph-key program, as the stand-alone sanitizer build it is ----------------------------------
def test_step_mode_check_with_the_cache_rules_under_sanitizers(tmp_path):
    rocm_clang = os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..", "llvm", "bin",
                              "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which(rocm_clang)
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    src_path = os.path.join(REPO, "tools", "step_mode_check.cpp")
    src = open(src_path).read()
    assert "cache_kind" in src and "cache_conflict" in src  # the cache cases are part of it
    exe = str(tmp_path / "step_mode_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(REPO, "include"), "-I", os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    src_path, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "step_mode_check: ok" in out
