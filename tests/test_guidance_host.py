"""Host (no GPU): the guidance controls' argument rules, signatures, segment arithmetic and ABI entries.

A step at position p of a loop has the network timestep tau[p-1] (tau = Diffuser._mode_timesteps(mode));
it uses CFG iff t_lo <= tau[p-1] <= t_hi.  tau ascends, so the guided positions form one run and a
loop (or a guard chunk of one) has at most three segments."""
import inspect
import os
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def diffuser(T=1000):
    import diff
    return diff.Diffuser(T)


# ---- argument rules ---------------------------------------------------------------------------------
def test_guidance_args_accepts_and_normalises():
    d = diffuser()
    assert d._guidance_args(3.0, None, 0.0, 1000) == (None, 0.0)
    assert d._guidance_args(0.0, None, 0.0, 1000) == (None, 0.0)   # the defaults ask nothing of the scale
    assert d._guidance_args(None, None, 0, 1000) == (None, 0.0)
    assert d._guidance_args(3.0, (1, 1000), 1.0, 1000) == ((1, 1000), 1.0)
    assert d._guidance_args(3.0, [200, 200], 0.25, 1000) == ((200, 200), 0.25)
    iv, phi = d._guidance_args(1.5, (torch.tensor(3).item(), 7), 0.5, 12)
    assert iv == (3, 7) and phi == 0.5 and all(type(v) is int for v in iv)


@pytest.mark.parametrize("phi", [-0.1, 1.0001, float("nan"), float("inf"), "a", None])
def test_rescale_outside_unit_interval_raises(phi):
    with pytest.raises(ValueError):
        diffuser()._guidance_args(3.0, None, phi, 1000)


@pytest.mark.parametrize("iv", [(0, 10), (5, 4), (1, 1001), (1,), (1, 2, 3), (1.0, 5), (1, 5.5), "ab", 7,
                                (True, 5), (None, 5)])
def test_malformed_interval_raises(iv):
    with pytest.raises(ValueError):
        diffuser()._guidance_args(3.0, iv, 0.0, 1000)


@pytest.mark.parametrize("g", [None, 0, 0.0, -1.0])
def test_controls_need_positive_guidance_scale(g):
    d = diffuser()
    with pytest.raises(ValueError):
        d._guidance_args(g, (1, 1000), 0.0, 1000)
    with pytest.raises(ValueError):
        d._guidance_args(g, None, 0.5, 1000)


def test_sampler_raises_before_touching_the_model():
    d = diffuser(12)
    kw = dict(z_shape=(4, 8, 8), vae=None, progress=False)
    state = torch.get_rng_state()
    for bad in (dict(guidance_rescale=1.5), dict(guidance_interval=(0, 3)), dict(guidance_interval=(3, 13)),
                dict(guidance_scale=0.0, guidance_rescale=0.5), dict(guidance_scale=0.0, guidance_interval=(1, 12)),
                dict(guidance_scale=None, guidance_interval=(1, 12))):
        with pytest.raises(ValueError):
            d.sample_latent_cond(object(), {1: 1}, **kw, **bad)
    assert torch.equal(torch.get_rng_state(), state)  # nothing was drawn


def test_engine_rejects_rescale_without_cfg():
    from dmx import engine
    assert engine._guidance_struct(0.0, 0.0, None) is None
    assert engine._guidance_struct(0, 3.0, object()) is None
    gd = engine._guidance_struct(0.5, 3.0, object())
    assert abs(gd.rescale - 0.5) == 0
    for phi, g, y in ((0.5, 0.0, object()), (0.5, 3.0, None), (1.5, 3.0, object()), (-0.5, 3.0, object())):
        with pytest.raises(ValueError):
            engine._guidance_struct(phi, g, y)


# ---- signatures ---------------------------------------------------------------------------------------
def test_three_samplers_carry_the_keywords():
    import diff
    from dmx import distributed
    from entityCsvSampler import EntityCsvSampler
    for fn in (diff.Diffuser.sample_latent_cond, distributed.ShardedCondSampler.sample, EntityCsvSampler.sample):
        ps = inspect.signature(fn).parameters
        assert ps["guidance_interval"].default is None
        assert ps["guidance_rescale"].default == 0.0 and isinstance(ps["guidance_rescale"].default, float)
    # out of scope: the public one-step calls keep their signatures
    for fn in (diff.Diffuser.denoise_cond, diff.Diffuser.ddim_step, diff.Diffuser.dpm_step):
        ps = inspect.signature(fn).parameters
        assert "guidance_rescale" not in ps and "rescale" not in ps and "unguided" not in ps


def test_native_model_step_and_loop_take_rescale():
    from dmx import engine
    for fn in (engine.NativeModel.step, engine.NativeModel.sample_loop):
        assert inspect.signature(fn).parameters["rescale"].default == 0.0
    assert list(inspect.signature(engine.cfg_rescale).parameters) == ["eu", "ec", "guidance", "phi"]


# ---- the guided run and the segments ------------------------------------------------------------------
def brute(tau, interval, i_from, i_to):
    """Positions i_from .. i_to + 1 with their kind, grouped where it changes."""
    out = []
    for p in range(i_from, i_to, -1):
        g = interval is None or interval[0] <= tau[p - 1] <= interval[1]
        if out and out[-1][2] == g:
            out[-1][1] = p - 1
        else:
            out.append([p, p - 1, g])
    return [tuple(s) for s in out]


def schedules():
    d = diffuser(1000)
    d12 = diffuser(12)
    yield "ddpm T=12", d12, d12._mode_timesteps(None)
    yield "ddim S=5", d, d.ddim_timesteps(5)
    yield "ddim S=7", d, d.ddim_timesteps(7)
    yield "dpm S=6", d, d.dpm_timesteps(6)
    yield "dpm S=20", d, d.dpm_timesteps(20, "logsnr")
    yield "dpm S=9 uniform", d, d.dpm_timesteps(9, "uniform")


def test_mode_timesteps_are_the_schedules():
    d = diffuser(12)
    assert d._mode_timesteps(None) == list(range(1, 13))
    d = diffuser(1000)
    assert d._mode_timesteps(("ddim", 5, 0.0)) == d.ddim_timesteps(5) == [200, 400, 600, 800, 1000]
    assert d._mode_timesteps(("dpm", 6, "logsnr")) == d.dpm_timesteps(6, "logsnr")


def test_segments_match_brute_force_everywhere():
    for name, d, tau in schedules():
        S, T = len(tau), d.num_timesteps
        bounds = sorted({1, T, tau[0], tau[-1]} | {t for t in tau} | {min(T, t + 1) for t in tau}
                        | {max(1, t - 1) for t in tau})
        intervals = [None] + [(lo, hi) for lo in bounds for hi in bounds if lo <= hi]
        for iv in intervals:
            run = d._guided_run(tau, iv)
            guided = [p for p in range(1, S + 1) if iv is None or iv[0] <= tau[p - 1] <= iv[1]]
            assert run == ((guided[0], guided[-1]) if guided else None), (name, iv)
            for p0 in sorted({S, max(1, S - 2), 1}):          # entry positions (img2img: p0 < S)
                for chunk in (3, S, 50):                       # guard chunks: boundaries fall inside them
                    i = p0
                    while i >= 1:
                        j = max(i - chunk, 0)
                        segs = d._guidance_segments(i, j, run)
                        assert segs == brute(tau, iv, i, j), (name, iv, p0, chunk, i, j)
                        assert 1 <= len(segs) <= 3
                        assert segs[0][0] == i and segs[-1][1] == j
                        assert all(a > b for a, b, _ in segs)
                        assert all(x[1] == y[0] for x, y in zip(segs, segs[1:]))
                        i = j


def test_segments_named_cases():
    d = diffuser(1000)
    seg = d._guidance_segments
    tau = d.ddim_timesteps(5)  # 200 400 600 800 1000
    assert d._guided_run(tau, None) == (1, 5)
    assert d._guided_run(tau, (1, 1000)) == (1, 5)            # covers everything
    assert seg(5, 0, (1, 5)) == [(5, 0, True)]
    assert d._guided_run(tau, (401, 599)) is None             # legal, covers no timestep of the schedule
    assert seg(5, 0, None) == [(5, 0, False)]
    assert d._guided_run(tau, (800, 1000)) == (4, 5)          # touches the top end
    assert seg(5, 0, (4, 5)) == [(5, 3, True), (3, 0, False)]
    assert d._guided_run(tau, (1, 200)) == (1, 1)             # touches the bottom end
    assert seg(5, 0, (1, 1)) == [(5, 1, False), (1, 0, True)]
    assert d._guided_run(tau, (400, 600)) == (2, 3)           # the middle: three segments
    assert seg(5, 0, (2, 3)) == [(5, 3, False), (3, 1, True), (1, 0, False)]
    assert seg(3, 0, (2, 3)) == [(3, 1, True), (1, 0, False)]  # entry position p0 = 3 < S
    assert seg(5, 2, (2, 3)) == [(5, 3, False), (3, 2, True)]  # a chunk that ends inside the run... at position 3
    assert seg(0, 0, (2, 3)) == [] and seg(2, 2, (1, 5)) == []
    # DDPM: tau = 1..T, positions are timesteps
    d12 = diffuser(12)
    tau = d12._mode_timesteps(None)
    assert d12._guided_run(tau, (4, 9)) == (4, 9)
    assert seg(12, 0, (4, 9)) == [(12, 9, False), (9, 3, True), (3, 0, False)]


# ---- the ABI entries ----------------------------------------------------------------------------------
def test_header_and_bindings_name_the_new_symbols():
    from dmx import _lib
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    bound = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for sym in ("dmx_step_guided", "dmx_sample_loop_guided", "dmx_cfg_rescale", "dmx_model_graph_captures"):
        assert sym + "(" in hdr and sym in bound, sym
    assert "typedef struct dmx_guidance" in hdr
    assert [f[0] for f in _lib.Guidance._fields_] == ["rescale"]
    assert len(bound["dmx_step_guided"][1]) == 7 and len(bound["dmx_sample_loop_guided"][1]) == 9
    assert len(bound["dmx_cfg_rescale"][1]) == 11
    lib = _lib.load()
    assert lib.dmx_abi_version() == 1
    assert lib.dmx_model_graph_captures(None) == -1
    # argument checks that need no device
    assert lib.dmx_cfg_rescale(None, None, 3.0, 0.5, None, None, 1, 4, 8, 8, None) == _lib.DMX_E_ARG
    assert lib.dmx_step_guided(None, None, None, None, None, None, None) == _lib.DMX_E_ARG


# ---- the graph slots' bookkeeping, stand-alone under the host sanitizers ---------------------------------
def _standalone_check(tmp_path, name):
    from dmx import build
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or build.HIPCC  # (host code only)
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    os.path.join(REPO, "tools", name + ".cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert name + ": ok" in out.stdout


def test_graph_slots_lru_standalone(tmp_path):
    _standalone_check(tmp_path, "graph_slots_check")


# ---- the graph key's rules (what enters it in which mode), stand-alone likewise ---------------------------
def test_step_mode_key_standalone(tmp_path):
    _standalone_check(tmp_path, "step_mode_check")
