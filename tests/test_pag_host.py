"""Host (no GPU): perturbed-attention guidance — the argument rules of Diffuser._pag_args, the branch
tables it builds, the samplers' keywords, the ABI entries and the graph key's rules with the perturb
member (stand-alone, under the host sanitizers).

The perturbed branch holds the main condition's rows again; its weight row is -s and the main branch's
becomes fp32(g + s), so the composed mix e_0 + sum_k w_k (e_k - e_0) is e_u + g (e_c - e_u) + s (e_c - e_p)."""
import inspect
import os
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = [1, 1, 2]


def setup(T=12):
    import diff
    d = diff.Diffuser(T)
    vals, msk = d._build_cond(Y, None, None, None, None, "cpu")
    vals = vals + torch.arange(36, dtype=torch.float32).view(3, 12) / 36
    return d, vals, msk


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


class Native:
    """Stands for a dmx network of the given libdmx kind (what _native_kind reads)."""
    def __init__(self, kind):
        type(self)._dmx_kind = kind

    def native(self):
        raise AssertionError("argument rules must not touch the engine")


def native(kind):
    return type("Native%d" % kind, (Native,), {})(kind)


# ---- pag_scale 0 is the call without the keywords -----------------------------------------------------
@pytest.mark.parametrize("scale", [0, 0.0, [0.0, 0.0, 0.0], torch.zeros(3)])
def test_zero_scale_is_the_plain_plan(scale):
    import diff
    d, vals, msk = setup()
    assert d._pag_args(scale, ("sa3",), Y, vals, msk, 3.0) is None
    assert d._pag_args(scale, ("nonsense",), Y, vals, msk, 3.0, guidance_interval=(1, 5)) is None
    x = torch.zeros((3, 4, 8, 8))
    plain = d._plan(x, ("dpm", 6, "logsnr"), 3.0)
    assert plain.perturb is None and plain.compose is None
    assert "perturb" not in plain.kwargs(True) and "compose" not in plain.kwargs(True)
    assert diff._SamplerPlan("ddpm").perturb is None


# ---- the tables -------------------------------------------------------------------------------------
def test_plain_cfg_call_gains_one_branch():
    d, vals, msk = setup()
    (y_rows, v_rows, m_rows, w), (blocks, branches) = d._pag_args(2.0, ("sa3",), Y, vals, msk, 3.0, null_label=7)
    assert y_rows.dtype == torch.long and y_rows.tolist() == [[7, 7, 7], Y, Y]
    assert v_rows.shape == m_rows.shape == (3, 3, 12) and v_rows.dtype == m_rows.dtype == torch.float32
    for k in range(3):   # base "null": the call's rows in every branch
        assert torch.equal(v_rows[k], vals) and torch.equal(m_rows[k], msk)
    assert w.dtype == torch.float32 and torch.equal(w, torch.stack([f32([3.0] * 3) + f32([2.0] * 3), -f32([2.0] * 3)]))
    assert (blocks, branches) == (0b000100, 0b100)
    for t in (y_rows, v_rows, m_rows, w):
        assert t.is_contiguous()


def test_per_sample_scale_and_fp32_sum():
    d, vals, msk = setup()
    s = [0.1, 0.0, 2.5]
    (y_rows, _, _, w), pt = d._pag_args(s, ["sa1", "sa6"], Y, vals, msk, 0.7)
    assert torch.equal(w[0], f32([0.7] * 3) + f32(s))       # fp32(g + s), one rounding
    assert torch.equal(w[1], -f32(s)) and w[1, 1] == 0       # a zero entry: that sample is not pushed
    assert pt == (0b100001, 0b100)
    (_, _, _, w2), _ = d._pag_args(torch.tensor(s, dtype=torch.float64), {"sa2"}, Y, vals, msk, 0.7)
    assert torch.equal(w2, w)


def test_no_cfg_is_k1_over_the_main_condition():
    d, vals, msk = setup()
    for g in (0.0, 0, None):
        (y_rows, v_rows, m_rows, w), pt = d._pag_args([1.5, 0.0, 3.0], ("sa3", "sa4"), Y, vals, msk, g)
        assert y_rows.tolist() == [Y, Y]
        assert torch.equal(v_rows[0], vals) and torch.equal(v_rows[1], vals)
        assert torch.equal(m_rows[0], msk) and torch.equal(m_rows[1], msk)
        assert torch.equal(w, -f32([[1.5, 0.0, 3.0]]))
        assert pt == (0b001100, 0b10)


def test_base_and_also_keep_their_branches():
    d, vals, msk = setup()
    also = [dict(classes=3, weight=0.5), dict(classes=[2, 2, 1], cond=vals * 2, cond_mask=msk, weight=[1, 2, 3])]
    comp = d._compose_args(Y, vals, msk, [1.0, -2.0, 0.0], "dropped", also)
    (y_rows, v_rows, m_rows, w), pt = d._pag_args(2.0, ("sa3",), Y, vals, msk, [1.0, -2.0, 0.0], comp)
    assert y_rows.shape[0] == 5 and pt == (4, 1 << 4)
    for new, old in zip((y_rows, v_rows, m_rows), comp):
        assert torch.equal(new[:4], old) and torch.equal(new[4], old[1])   # the main branch's rows again
    assert torch.equal(w[0], comp[3][0] + f32([2.0] * 3)) and torch.equal(w[1:3], comp[3][1:])
    assert torch.equal(w[3], -f32([2.0] * 3))
    with pytest.raises(ValueError, match="also"):
        d._pag_args(2.0, ("sa3",), Y, vals, msk, 3.0,
                    d._compose_args(Y, vals, msk, 3.0, "null", also + [dict(classes=1, weight=1.0)]))


# ---- every ValueError, before anything is drawn -----------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(pag_scale=-1.0), dict(pag_scale=[1.0, -0.5, 0.0]), dict(pag_scale=float("nan")),
    dict(pag_scale=float("inf")), dict(pag_scale=[1.0, 2.0]), dict(pag_scale=[1.0] * 4), dict(pag_scale="big"),
    dict(pag_blocks=()), dict(pag_blocks=("sa7",)), dict(pag_blocks=("sa0",)), dict(pag_blocks=("sa3", "sa3")),
    dict(pag_blocks=("sa3", 4)), dict(pag_blocks=3), dict(pag_blocks="sa33"),
    dict(guidance_interval=(2, 9)), dict(guidance_rescale=0.5), dict(geom_scale=1.0),
    dict(geom_scale=[0.0, 1.0, 0.0]),
])
def test_sampler_rejects_before_any_draw(kw):
    import diff
    d = diff.Diffuser(12)
    kw = dict(dict(pag_scale=2.0), **kw)
    cond = torch.arange(36, dtype=torch.float32).view(3, 12) / 36
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        d.sample_latent_cond(native(1), {1: 2, 2: 1}, z_shape=(4, 8, 8), vae=None, progress=False, cond=cond, **kw)
    assert torch.equal(state, torch.get_rng_state())


def test_models_that_cannot_be_perturbed():
    d, vals, msk = setup()
    with pytest.raises(ValueError, match="foreign"):
        d._pag_args(2.0, ("sa3",), Y, vals, msk, 3.0, model=torch.nn.Identity())
    with pytest.raises(ValueError, match="conditional"):
        d._pag_args(2.0, ("sa3",), Y, vals, msk, 3.0, model=native(3))
    with pytest.raises(ValueError, match="conditional"):
        d._pag_args(2.0, ("sa3",), Y, vals, msk, 3.0, model=native(4))
    for kind in (1, 2):
        assert d._pag_args(2.0, ("sa3",), Y, vals, msk, 3.0, model=native(kind)) is not None
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="foreign"):
        d.sample_latent_cond(torch.nn.Identity(), {1: 2, 2: 1}, z_shape=(4, 8, 8), vae=None, progress=False,
                             pag_scale=1.0)
    assert torch.equal(state, torch.get_rng_state())


def test_a_single_name_and_other_collections():
    d, vals, msk = setup()
    for blocks in ("sa3", ["sa3"], ("sa3",), {"sa3"}):
        assert d._pag_args(1.0, blocks, Y, vals, msk, 3.0)[1] == (4, 4)
    assert d._pag_args(1.0, d.PAG_BLOCKS, Y, vals, msk, 3.0)[1] == (63, 4)


# ---- the plan carries the pair; a shard takes its columns --------------------------------------------------
def test_plan_and_shard():
    d, vals, msk = setup()
    comp, pt = d._pag_args([1.0, 0.0, 2.0], ("sa3", "sa5"), Y, vals, msk, 3.0)
    x = torch.zeros((3, 4, 8, 8))
    plan = d._plan(x, ("ddim", 5, 0.0), 3.0, compose=comp, perturb=pt)
    assert plan.perturb == pt and plan.scale == 0.0
    for guided in (True, False):
        kw = plan.kwargs(guided, seed=3, use_graph=True)
        assert kw["perturb"] == pt and kw["compose"] is plan.compose
    shard = d._plan(x[1:3], ("ddim", 5, 0.0), 3.0, compose=comp, perturb=pt, rows=(1, 3))
    assert shard.perturb == pt     # the struct is shard-invariant
    for a, b in zip(shard.compose, comp):
        assert torch.equal(a, b[:, 1:3])
    with pytest.raises(ValueError):
        d._plan(x, None, 3.0, perturb=pt)


# ---- signatures --------------------------------------------------------------------------------------------
def test_keywords_and_defaults():
    import diff
    from dmx import distributed as dd
    from dmx import engine
    from entityCsvSampler import EntityCsvSampler
    for fn in (diff.Diffuser.sample_latent_cond, dd.ShardedCondSampler.sample, EntityCsvSampler.sample):
        p = inspect.signature(fn).parameters
        assert p["pag_scale"].default == 0.0 and tuple(p["pag_blocks"].default) == ("sa3",)
    for fn in (engine.NativeModel.step, engine.NativeModel.sample_loop, engine.NativeModel.forward):
        assert inspect.signature(fn).parameters["perturb"].default is None
    assert list(inspect.signature(engine.attn_identity).parameters) == ["qkv", "C"]
    assert diff.Diffuser.PAG_BLOCKS == ("sa1", "sa2", "sa3", "sa4", "sa5", "sa6")
    with pytest.raises(ValueError):
        engine.NativeModel._perturb((4, 4), None, None)                      # needs a composition
    with pytest.raises(ValueError):
        engine.NativeModel._perturb((4, 4), (1, 2, 3, 4), (1, 2))            # no geometry guidance
    for bad in ((0, 4), (64, 4), (4, 0), (4, 32), (4,), 4):
        with pytest.raises(ValueError):
            engine.NativeModel._perturb(bad, (1, 2, 3, 4), None)
    pt = engine.NativeModel._perturb((5, 6), (1, 2, 3, 4), None)
    assert (pt.blocks, pt.branches) == (5, 6)


# ---- the ABI ---------------------------------------------------------------------------------------------
NEW = ("dmx_step_perturbed", "dmx_sample_loop_perturbed", "dmx_unet_forward_perturbed", "dmx_attn_identity")


def test_abi_lists_the_new_symbols():
    import ctypes
    from dmx import _lib
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for name in NEW:
        assert name in sigs, name
    assert len(sigs["dmx_step_perturbed"][1]) == len(sigs["dmx_step_composed"][1]) + 1
    assert len(sigs["dmx_sample_loop_perturbed"][1]) == len(sigs["dmx_sample_loop_composed"][1]) + 1
    assert len(sigs["dmx_unet_forward_perturbed"][1]) == len(sigs["dmx_unet_forward"][1]) + 3
    assert ctypes.sizeof(_lib.Perturb) == 8 and [f[0] for f in _lib.Perturb._fields_] == ["blocks", "branches"]
    header = open(os.path.join(REPO, "include", "dmx.h")).read()
    for name in NEW + ("typedef struct dmx_perturb",):
        assert name in header, name
    lib = _lib.load()
    assert lib.dmx_abi_version() == 1
    # argument checks that need no device
    assert lib.dmx_step_perturbed(None, None, None, None, None, None, None, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_sample_loop_perturbed(None, None, None, None, None, None, None, None, 1, 0, None) == _lib.DMX_E_ARG
    assert lib.dmx_attn_identity(None, None, 1, 9, 64, None) == _lib.DMX_E_ARG
    assert lib.dmx_unet_forward_perturbed(None, None, None, None, None, None, None, None, 2, 8, 8, 0, 0, 1,
                                          None) == _lib.DMX_E_ARG
    assert b"blocks" in lib.dmx_last_error()
    assert lib.dmx_unet_forward_perturbed(None, None, None, None, None, None, None, None, 2, 8, 8, 4, 1, 1,
                                          None) == _lib.DMX_E_ARG
    assert b"row0" in lib.dmx_last_error()


# ---- the graph key's rules with the perturb member, stand-alone under the host sanitizers -----------------
def test_step_mode_key_standalone_with_perturb(tmp_path):
    from dmx import build
    src = os.path.join(REPO, "tools", "step_mode_check.cpp")
    text = open(src).read()
    for rule in ("in.perturb.blocks =", "in.perturb.branches =", "k.perturb", "use_perturb ? &perturb : nullptr",
                 "!(perturbed == composed)", "StepMode{}.perturb == nullptr"):
        assert rule in text, rule
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or build.HIPCC  # (host code only)
    exe = str(tmp_path / "step_mode_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "step_mode_check: ok" in out.stdout
