"""The narrower step / loop entries of include/dmx.h, called raw through dmx._lib.

NativeModel.step and NativeModel.sample_loop make one library call each (dmx_step_guided,
dmx_sample_loop_guided); dmx_step, dmx_step_ddim, dmx_step_dpm, dmx_step_known and their four
loops stay in the ABI for C callers.  Each is the general entry with the arguments it lacks NULL
and rescale 0: the same bits, the same final t and — for the loops — the same captured graphs.

Shape: the conditional U-Net at B = 2 on a 4x8x8 latent (the smallest the engine admits; CFG batch 4),
schedules of S = 3 positions."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

B, HW, S, G = 2, 8, 3, 3.0
KINDS = ["ddpm", "ddim", "dpm", "known"]


@pytest.fixture(scope="module")
def setup(cuda, unet_sd):
    """One model and one set of device buffers: the loops' graph keys hold their addresses."""
    import diff
    from dmx import engine
    from models.unet_cond_geom import UnetCondWithGeomHead
    m = UnetCondWithGeomHead()
    m.load_state_dict(unet_sd)
    nm = m.to(cuda).eval().native()
    d = diff.Diffuser(1000, device=cuda)
    nm.ctx.ensure_time_table(1000)
    gen = torch.Generator().manual_seed(900)

    def randn(*shape):
        return torch.randn(shape, generator=gen).to(cuda)

    s = dict(nm=nm, lib=nm.lib, model=m, x0=randn(B, 4, HW, HW), noise=randn(B, 4, HW, HW),
             x=torch.empty((B, 4, HW, HW), device=cuda), out=torch.empty((B, 4, HW, HW), device=cuda),
             hist=torch.empty((B, 4, HW, HW), device=cuda), y=torch.tensor([1, 3], device=cuda),
             vals=torch.rand((B, 12), generator=gen).to(cuda), cmask=torch.ones((B, 12), device=cuda),
             t=torch.zeros((B,), dtype=torch.long, device=cuda), tables=d.coef_tables(cuda, True),
             ddim=d.ddim_tables(S, 0.5, cuda), dpm=d.dpm_tables(S, "uniform", cuda))
    kmask = (torch.rand((B, 1, HW, HW), generator=gen) > 0.5).float().to(cuda)
    s["known"] = (randn(B, 4, HW, HW), randn(B, 4, HW, HW), kmask) + tuple(d.known_tables(d.ddim_timesteps(S), cuda))
    s["structs"] = dict(ddim=engine._sched_struct(s["ddim"], cuda),
                        dpm=engine._dpm_struct(s["dpm"], cuda, s["hist"], s["x"]),
                        known=engine._known_struct(s["known"], cuda, s["x"], need_mask=True))
    return s


def ref_or_null(struct):
    return None if struct is None else ctypes.byref(struct)


def parts(s, kind):
    """(ddim, dpm, known) structs of a kind; the known-region kind runs on the DDIM schedule."""
    st = s["structs"]
    return (st["ddim"] if kind in ("ddim", "known") else None, st["dpm"] if kind == "dpm" else None,
            st["known"] if kind == "known" else None)


def narrow_tail(s, kind):
    """The arguments the kind's own entry takes between the step args and (steps, use_graph,) stream."""
    ddim, dpm, known = parts(s, kind)
    return {"ddpm": (), "ddim": (ctypes.byref(s["structs"]["ddim"]),), "dpm": (ctypes.byref(s["structs"]["dpm"]),),
            "known": (ref_or_null(ddim), ref_or_null(dpm), ref_or_null(known))}[kind]


def guided_tail(s, kind, gd):
    return tuple(ref_or_null(p) for p in parts(s, kind)) + (ref_or_null(gd),)


def step_args(s, kind, x_in, x_out, t, t_stride, noise):
    nm = s["nm"]
    return nm._args(x_in, x_out, t, t_stride, s["y"], 0, s["vals"], s["cmask"], G,
                    s["tables"] if kind == "ddpm" else None, None if kind == "dpm" else noise, 11, 0)


def reset(s, p):
    s["x"].copy_(s["x0"])
    s["hist"].fill_(float("nan"))
    s["t"].fill_(p)


@pytest.mark.parametrize("kind", KINDS)
def test_step_entry_is_the_general_entry(setup, cuda, kind):
    from dmx import _lib
    s = setup
    lib, h = s["lib"], s["nm"].handle
    entry = {"ddpm": lib.dmx_step, "ddim": lib.dmx_step_ddim, "dpm": lib.dmx_step_dpm, "known": lib.dmx_step_known}[kind]
    gd = _lib.Guidance(0.0)
    got = {}
    for name in ("general", "narrow"):
        reset(s, S)
        s["out"].fill_(float("nan"))
        a = step_args(s, kind, s["x"], s["out"], s["t"], 1, s["noise"])   # host-given noise: nothing is drawn
        with torch.cuda.device(cuda):
            st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
            if name == "general":
                _lib.check(lib.dmx_step_guided(h, ctypes.byref(a), *guided_tail(s, kind, gd), st))
            else:
                _lib.check(entry(h, ctypes.byref(a), *narrow_tail(s, kind), st))
        torch.cuda.synchronize()
        got[name] = (s["out"].clone(), s["hist"].clone())
    assert torch.isfinite(got["general"][0]).all() and not torch.equal(got["general"][0], s["x0"])
    assert torch.equal(got["narrow"][0], got["general"][0])
    if kind == "dpm":
        assert torch.isfinite(got["general"][1]).all() and torch.equal(got["narrow"][1], got["general"][1])


@pytest.mark.parametrize("kind", KINDS)
def test_loop_entry_replays_the_general_entry_s_graph(setup, cuda, kind):
    from dmx import _lib
    s = setup
    nm, lib, h = s["nm"], s["lib"], s["nm"].handle
    entry = {"ddpm": lib.dmx_sample_loop, "ddim": lib.dmx_sample_loop_ddim, "dpm": lib.dmx_sample_loop_dpm,
             "known": lib.dmx_sample_loop_known}[kind]
    gd = _lib.Guidance(0.0)
    t = s["t"][:1]
    side = nm.side_stream()   # (capture needs a non-default stream)
    got = {}
    for name in ("general", "narrow"):
        reset(s, S)
        torch.cuda.synchronize()
        c0 = nm.graph_captures()
        a = step_args(s, kind, s["x"], s["x"], t, 0, None)
        with torch.cuda.device(cuda):
            st = ctypes.c_void_p(side.cuda_stream)
            if name == "general":
                _lib.check(lib.dmx_sample_loop_guided(h, ctypes.byref(a), *guided_tail(s, kind, gd), S, 1, st))
            else:
                _lib.check(entry(h, ctypes.byref(a), *narrow_tail(s, kind), S, 1, st))
        torch.cuda.synchronize()
        got[name] = (s["x"].clone(), int(t.item()), nm.graph_captures() - c0)
    assert torch.isfinite(got["general"][0]).all() and got["general"][1] == 0
    assert got["general"][2] == 1          # no other test runs this loop on these buffers
    assert torch.equal(got["narrow"][0], got["general"][0])
    assert got["narrow"][1] == 0
    assert got["narrow"][2] == 0           # it replayed the general entry's graph


def test_an_entry_s_own_part_must_be_given(setup, cuda):
    from dmx import _lib
    s = setup
    lib, h = s["lib"], s["nm"].handle
    reset(s, S)
    s["out"].fill_(7.0)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    a = step_args(s, "ddim", s["x"], s["out"], s["t"], 1, s["noise"])
    a_dpm = step_args(s, "dpm", s["x"], s["out"], s["t"], 1, None)
    ddim = ctypes.byref(s["structs"]["ddim"])
    with torch.cuda.device(cuda):
        assert lib.dmx_step_ddim(h, ctypes.byref(a), None, st) == _lib.DMX_E_ARG
        assert lib.dmx_step_dpm(h, ctypes.byref(a_dpm), None, st) == _lib.DMX_E_ARG
        assert lib.dmx_step_known(h, ctypes.byref(a), ddim, None, None, st) == _lib.DMX_E_ARG
        assert lib.dmx_step_guided(h, ctypes.byref(a), ddim, None, None, None, st) == _lib.DMX_E_ARG
    torch.cuda.synchronize()
    assert bool((s["out"] == 7.0).all())   # nothing was launched
    assert torch.equal(s["x"], s["x0"])
