"""CPU-only: the host side of the native optimizer (dmx/optim.py, csrc/optim_table.h) — import without
a GPU, refused arguments, the chunk table's cover, torch Adam's state_dict layout, EMA swap and the
ABI's argument checks."""
import copy
import os
import shutil
import subprocess

import pytest
import torch

from conftest import REPO


def _params(shapes=((3, 2), (5,), ()), seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


def test_import_needs_no_gpu():
    import dmx.optim as O
    assert issubclass(O.Adam, torch.optim.Optimizer) and issubclass(O.AdamW, O.Adam)
    opt = O.Adam(_params(), lr=1e-3)
    assert opt.defaults["lr"] == 1e-3 and opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["eps"] == 1e-8
    assert opt.defaults["weight_decay"] == 0.0 and opt.defaults["decoupled_weight_decay"] is False
    assert opt.grad_norm is None and opt.max_grad_norm is None and opt.ema_decay is None
    w = O.AdamW(_params())
    assert w.defaults["weight_decay"] == 1e-2 and w.defaults["decoupled_weight_decay"] is True


@pytest.mark.parametrize("name", ["amsgrad", "maximize", "capturable"])
def test_refused_constructor_arguments_name_themselves(name):
    from dmx.optim import Adam, AdamW
    for cls in (Adam, AdamW):
        with pytest.raises(ValueError, match=name):
            cls(_params(), **{name: True})
        cls(_params(), **{name: False})  # torch's default is accepted
    with pytest.raises(TypeError):
        Adam(_params(), no_such_argument=1)


def test_refused_closure_and_group_flags():
    from dmx.optim import Adam
    opt = Adam(_params())
    with pytest.raises(ValueError, match="closure"):
        opt.step(closure=lambda: 0.0)
    opt.param_groups[0]["amsgrad"] = True  # e.g. from a loaded torch checkpoint
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)),
                                dict(weight_decay=-1.0), dict(max_grad_norm=0.0), dict(ema_decay=1.0)])
def test_bad_hyperparameters(kw):
    from dmx.optim import Adam
    with pytest.raises(ValueError):
        Adam(_params(), **kw)


def test_refused_gradients_and_no_host_fallback():
    from dmx import DmxUnavailable
    from dmx.optim import Adam
    ps = _params()
    opt = Adam(ps)
    for p in ps:
        p.grad = torch.zeros_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(DmxUnavailable):  # CPU parameters: there is no host implementation
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, ps)) and opt.state_dict()["state"] == {}


def test_chunk_table_covers_every_element_once():
    from dmx.optim import CHUNK, chunk_table
    C = CHUNK
    sizes = [0, 1, 3, 4, C - 1, C, C + 1, 2 * C + 5]
    table = chunk_table(sizes)
    seen = [torch.zeros(n, dtype=torch.int32) for n in sizes]
    for t, off, ln in table:
        assert 0 <= t < len(sizes) and 1 <= ln <= C and off >= 0 and off % C == 0
        assert off + ln <= sizes[t]  # nothing beyond the tensor
        seen[t][off:off + ln] += 1
    assert all(bool((s == 1).all()) for s in seen)
    assert len(table) == sum(-(-n // C) for n in sizes)
    assert [t for t, _, _ in table] == sorted(t for t, _, _ in table)
    assert chunk_table([]) == [] and chunk_table([0, 0]) == []


def _layout_of(sd):
    return {i: {k: ((tuple(v.shape), v.dtype) if torch.is_tensor(v) else type(v)) for k, v in st.items()}
            for i, st in sd["state"].items()}


def test_state_dict_layout_is_torch_adams():
    from dmx.optim import Adam, state_layout
    ps = _params()
    ref = torch.optim.Adam(ps, lr=1e-3)
    for p in ps:
        p.grad = torch.ones_like(p)
    ref.step()
    want = _layout_of(ref.state_dict())
    assert state_layout(ps) == want
    # the optimizer's own state, initialised the way its first step does (the step needs the device)
    opt = Adam(_params())
    for i, p in enumerate(opt._params):
        opt._init_state(i, p)
    opt._steps[:] = 1.0
    sd = opt.state_dict()
    assert _layout_of(sd) == want
    assert all(float(st["step"]) == 1.0 for st in sd["state"].values())
    assert set(sd["param_groups"][0]) >= {"lr", "betas", "eps", "weight_decay", "params"}
    with_ema = Adam(_params(), ema_decay=0.9)
    assert _layout_of(with_ema.state_dict()) == state_layout(with_ema._params, ema=True)


def test_checkpoints_load_both_ways_on_the_host():
    from dmx.optim import Adam
    ps = _params()
    ref = torch.optim.Adam(ps, lr=2e-3, betas=(0.8, 0.99))
    for _ in range(3):
        for p in ps:
            p.grad = torch.ones_like(p)
        ref.step()
    sd = copy.deepcopy(ref.state_dict())
    opt = Adam(_params(), ema_decay=0.5)
    opt.load_state_dict(sd)
    assert [float(s) for s in opt._steps] == [3.0, 3.0, 3.0]
    assert opt.param_groups[0]["lr"] == 2e-3 and tuple(opt.param_groups[0]["betas"]) == (0.8, 0.99)
    for i, p in enumerate(opt._params):
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and float(st["step"]) == 3.0
        assert torch.equal(st["ema"], p)  # a checkpoint without EMA: the average restarts from the parameters
    opt._steps += 1.0  # the views in the state follow the array
    assert float(opt.state_dict()["state"][0]["step"]) == 4.0
    back = torch.optim.Adam(_params(), lr=1.0)
    back.load_state_dict(opt.state_dict())
    assert back.param_groups[0]["lr"] == 2e-3 and back.param_groups[0]["amsgrad"] is False
    assert float(back.state_dict()["state"][2]["step"]) == 4.0
    for p in back.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    back.step()  # torch Adam runs on from the native optimizer's checkpoint
    assert float(back.state_dict()["state"][2]["step"]) == 5.0


def test_param_groups_schedulers_and_zero_grad():
    from dmx.optim import Adam
    a, b = _params(((4,), (2, 2)))
    opt = Adam([{"params": [a], "lr": 1e-2}, {"params": [b], "weight_decay": 0.1}], lr=1e-3)
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 1e-3]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [5e-3, 5e-4]
    c = _params(((7,),))[0]
    opt.add_param_group({"params": [c], "betas": (0.5, 0.6)})
    assert len(opt._params) == 3 and list(opt._group_of) == [0, 1, 2] and len(opt._steps) == 3
    a.grad = torch.ones_like(a)
    opt.zero_grad(set_to_none=True)
    assert a.grad is None


def test_ema_weights_swap_is_exact_and_bumps_versions():
    from dmx.optim import Adam
    ps = _params()
    opt = Adam(ps, ema_decay=0.9)
    emas = [opt.state[p]["ema"] for p in ps]
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(emas, ps))
    with torch.no_grad():
        for e in emas:
            e.add_(1.0)
    p0 = [p.detach().clone() for p in ps]
    e0 = [e.clone() for e in emas]
    v0 = [p._version for p in ps]
    with pytest.raises(KeyError):
        with opt.ema_weights():
            assert all(torch.equal(p, e) for p, e in zip(ps, e0))
            assert all(torch.equal(e, p) for e, p in zip(emas, p0))
            assert all(p._version > v for p, v in zip(ps, v0))
            v1 = [p._version for p in ps]
            with pytest.raises(RuntimeError):
                opt.step()
            raise KeyError("from the block")
    assert all(torch.equal(p, q) for p, q in zip(ps, p0)) and all(torch.equal(e, f) for e, f in zip(emas, e0))
    assert all(p._version > v for p, v in zip(ps, v1))
    m = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError):
        opt.copy_ema_to(m)
    dst = [torch.zeros_like(p) for p in ps]
    opt.copy_ema_to(dst)
    assert all(torch.equal(d, e) for d, e in zip(dst, e0))
    with pytest.raises(RuntimeError):
        Adam(_params()).copy_ema_to(dst)


def test_abi_argument_checks_without_a_device():
    import ctypes
    from dmx import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    for sym in ("dmx_optim_chunks", "dmx_optim_create", "dmx_optim_destroy", "dmx_optim_set_step", "dmx_optim_step",
                "typedef struct dmx_optim_tensor", "typedef struct dmx_optim_chunk"):
        assert sym in hdr, sym
    assert ctypes.sizeof(_lib.OptimTensor) == 80 and ctypes.sizeof(_lib.OptimChunk) == 16
    assert f"#define DMX_OPTIM_CHUNK {_lib.DMX_OPTIM_CHUNK}\n" in hdr
    assert lib.dmx_optim_create(0, 1, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_optim_set_step(None, None, 0, None) == _lib.DMX_E_ARG
    assert lib.dmx_optim_step(None, 0.0, 0.0, 1.0, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_optim_destroy(None) == 0
    assert lib.dmx_optim_chunks(1, (ctypes.c_int64 * 1)(-1), None, 0) == -1


def test_optim_table_standalone(tmp_path):
    """The chunk table and the row checks (csrc/optim_table.h) under the host sanitizers."""
    from dmx import build
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or build.HIPCC  # (host code only)
    exe = str(tmp_path / "optim_table_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "diffusion-model_amd", "dmx", "csrc"),
                    os.path.join(REPO, "tools", "optim_table_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "optim_table_check: ok" in out.stdout
