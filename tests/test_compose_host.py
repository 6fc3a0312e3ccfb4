"""Host (no GPU): composed guidance — the argument rules of Diffuser._compose_args, the samplers'
keywords, the ABI entries and the graph key's rules (stand-alone, under the host sanitizers).

Branch 0 is the base ("null": null label with the call's cond rows; "dropped": null label with zero
rows; a spec: a negative condition), branch 1 the call's own condition with weight guidance_scale,
branches 2.. the specs of `also`:  eps = e_0 + sum_k w_k (e_k - e_0)."""
import inspect
import os
import shutil
import subprocess

import numpy as np
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


# ---- what it returns -----------------------------------------------------------------------------------
def test_plain_call_is_not_composed():
    d, vals, msk = setup()
    assert d._compose_args(Y, vals, msk, 3.0) is None
    assert d._compose_args(Y, vals, msk, 3.0, "null", None) is None
    assert d._compose_args(Y, vals, msk, 3.0, "null", []) is None
    assert d._compose_args(Y, vals, msk, 0.0) is None            # (a plain call's scale is not this function's)
    assert d._compose_args(Y, vals, msk, torch.tensor(3.0)) is None  # a 0-d tensor is a scalar


def test_branch_tables():
    d, vals, msk = setup()
    y_rows, v_rows, m_rows, w = d._compose_args(Y, vals, msk, [1.0, -2.0, 0.0], "dropped",
                                                [dict(classes=3, weight=0.5),
                                                 dict(classes=[2, 2, 1], cond=vals * 2, cond_mask=msk,
                                                      weight=[1, 2, 3])],
                                                null_label=0)
    assert y_rows.dtype == torch.long and y_rows.tolist() == [[0, 0, 0], Y, [3, 3, 3], [2, 2, 1]]
    assert v_rows.shape == m_rows.shape == (4, 3, 12) and v_rows.dtype == m_rows.dtype == torch.float32
    assert not v_rows[0].any() and not m_rows[0].any()                     # "dropped": zero rows
    assert torch.equal(v_rows[1], vals) and torch.equal(m_rows[1], msk)   # the call's own condition
    ev, em = d._build_cond([3, 3, 3], None, None, None, None, "cpu")      # a spec goes through _build_cond
    assert torch.equal(v_rows[2], ev) and torch.equal(m_rows[2], em)
    assert torch.equal(v_rows[3], vals * 2) and torch.equal(m_rows[3], msk)
    assert w.dtype == torch.float32 and w.tolist() == [[1.0, -2.0, 0.0], [0.5, 0.5, 0.5], [1.0, 2.0, 3.0]]
    for t in (y_rows, v_rows, m_rows, w):
        assert t.is_contiguous()
    # base "null" with a per-sample scale: the reference's unconditional branch, null_label honoured
    y_rows, v_rows, m_rows, w = d._compose_args(Y, vals, msk, np.array([1.0, 2.0, 3.0]), null_label=7)
    assert y_rows.tolist() == [[7, 7, 7], Y] and torch.equal(v_rows[0], vals) and torch.equal(m_rows[0], msk)
    assert w.tolist() == [[1.0, 2.0, 3.0]]
    # a negative condition as the base, dict-form cond
    y_rows, v_rows, m_rows, w = d._compose_args(Y, vals, msk, 2.5, dict(classes=2, cond={2: {"x1": 0.25}}))
    ev, em = d._build_cond([2, 2, 2], {2: {"x1": 0.25}}, None, None, None, "cpu")
    assert y_rows.tolist() == [[2, 2, 2], Y] and torch.equal(v_rows[0], ev) and torch.equal(m_rows[0], em)
    assert w.tolist() == [[2.5, 2.5, 2.5]]


# ---- every ValueError, with no GPU -------------------------------------------------------------------------
SPEC = dict(classes=1, weight=1.0)


@pytest.mark.parametrize("kw", [
    dict(also=[SPEC] * 4),                                                   # more than four branches
    dict(also=[dict(classes=[1, 2], weight=1.0)]),                           # row counts not equal to B
    dict(also=[dict(classes=1, weight=[1.0, 2.0])]),
    dict(also=[dict(classes=1, cond=torch.zeros(2, 12), weight=1.0)]),
    dict(base=dict(classes=[1, 2, 3, 1])),
    dict(guidance_scale=[1.0, 2.0]),
    dict(guidance_scale=torch.ones(4)),
    dict(also=[dict(classes=1, weight=float("nan"))]),                       # non-finite weights
    dict(also=[dict(classes=1, weight=[1.0, float("inf"), 0.0])]),
    dict(guidance_scale=[1.0, float("nan"), 2.0]),
    dict(guidance_scale=float("inf"), base="dropped"),
    dict(guidance_scale=0.0, base="dropped"),                                # scalar scale not positive
    dict(guidance_scale=-1.0, also=[SPEC]),
    dict(guidance_scale=None, base="dropped"),
    dict(base="dropped", guidance_interval=(1, 12)),                         # with interval / rescale
    dict(also=[SPEC], guidance_rescale=0.5),
    dict(guidance_scale=[1.0, 1.0, 1.0], guidance_rescale=0.5),
    dict(base="none"),                                                       # malformed specs
    dict(base=3),
    dict(base=dict(cond=None)),
    dict(base=dict(classes=1, weight=1.0)),
    dict(also=dict(classes=1, weight=1.0)),
    dict(also=["dropped"]),
    dict(also=[dict(classes=1)]),
    dict(also=[dict(classes=1, weight=1.0, scale=2.0)]),
    dict(also=[dict(classes="ab", weight=1.0)]),
    dict(also=[dict(classes=1, weight="w")]),
])
def test_compose_args_value_errors(kw):
    d, vals, msk = setup()
    args = dict(guidance_scale=3.0, base="null", also=None, guidance_interval=None, guidance_rescale=0.0)
    args.update(kw)
    with pytest.raises(ValueError):
        d._compose_args(Y, vals, msk, args["guidance_scale"], args["base"], args["also"], args["guidance_interval"],
                        args["guidance_rescale"])


def test_samplers_raise_before_touching_the_model():
    from dmx import distributed
    d, _, _ = setup()
    state = torch.get_rng_state()
    bads = (dict(also=[SPEC] * 4), dict(base="dropped", guidance_rescale=0.5),
            dict(base="dropped", guidance_interval=(1, 12)),
            dict(guidance_scale=[1.0, 2.0]), dict(base="dropped", guidance_scale=0.0), dict(base="x"),
            dict(also=[dict(classes=1, weight=float("nan"))]))
    for bad in bads:
        with pytest.raises(ValueError):
            d.sample_latent_cond(object(), {1: 2, 2: 1}, z_shape=(4, 8, 8), vae=None, progress=False, **bad)
        with pytest.raises(ValueError):
            distributed.ShardedCondSampler(d, object(), None).sample({1: 2, 2: 1}, z_shape=(4, 8, 8), decode=False,
                                                                     **bad)
    assert torch.equal(torch.get_rng_state(), state)  # nothing was drawn


def test_entity_csv_sampler_takes_base_only():
    from entityCsvSampler import EntityCsvSampler
    ps = inspect.signature(EntityCsvSampler.sample).parameters
    assert ps["base"].default == "null" and "also" not in ps
    s = EntityCsvSampler.__new__(EntityCsvSampler)
    for bad in (dict(classes=1), "none"):
        with pytest.raises(ValueError):
            s.sample("missing.csv", base=bad)


# ---- signatures --------------------------------------------------------------------------------------------
def test_keywords_and_signatures():
    import diff
    from dmx import distributed, engine
    for fn in (diff.Diffuser.sample_latent_cond, distributed.ShardedCondSampler.sample):
        ps = inspect.signature(fn).parameters
        assert ps["base"].default == "null" and ps["also"].default is None
    for fn in (engine.NativeModel.step, engine.NativeModel.sample_loop):
        assert inspect.signature(fn).parameters["compose"].default is None
    assert list(inspect.signature(engine.compose_eps).parameters) == ["e_list", "weights"]
    # out of scope: the public one-step calls keep their signatures
    for fn in (diff.Diffuser.denoise_cond, diff.Diffuser.ddim_step, diff.Diffuser.dpm_step):
        ps = inspect.signature(fn).parameters
        assert "compose" not in ps and "base" not in ps and "also" not in ps


# ---- ABI -----------------------------------------------------------------------------------------------------
def test_header_and_bindings_name_the_new_symbols():
    from dmx import _lib
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    bound = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for sym in ("dmx_step_composed", "dmx_sample_loop_composed", "dmx_compose_eps"):
        assert sym + "(" in hdr and sym in bound, sym
    assert "typedef struct dmx_compose" in hdr and "#define DMX_COMPOSE_MAX 4" in hdr
    assert _lib.DMX_COMPOSE_MAX == 4
    assert [f[0] for f in _lib.Compose._fields_] == ["K", "y", "vals", "mask", "weight"]
    assert len(bound["dmx_step_composed"][1]) == 8 and len(bound["dmx_sample_loop_composed"][1]) == 10
    assert len(bound["dmx_compose_eps"][1]) == 9
    lib = _lib.load()
    assert lib.dmx_abi_version() == 1
    # argument checks that need no device
    assert lib.dmx_compose_eps(None, None, 1, 1, 4, 8, 8, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_step_composed(None, None, None, None, None, None, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_sample_loop_composed(None, None, None, None, None, None, None, 1, 0, None) == _lib.DMX_E_ARG
    assert lib.dmx_last_error()


# ---- the graph key's rules with the compose member, stand-alone under the host sanitizers ---------------------
def test_step_mode_key_standalone_with_compose(tmp_path):
    from dmx import build
    src = os.path.join(REPO, "tools", "step_mode_check.cpp")
    text = open(src).read()
    for rule in ("in.comp.K = 3", "in.comp.y =", "in.comp.vals =", "in.comp.mask =", "in.comp.weight =",
                 "in.a.y =", "in.a.vals =", "in.a.mask =", "in.a.guidance =", "in.a.null_label =", "k.comp"):
        assert rule in text, rule
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or build.HIPCC  # (host code only)
    exe = str(tmp_path / "step_mode_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "step_mode_check: ok" in out.stdout
