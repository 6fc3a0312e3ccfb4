"""Native optimizer step: fused multi-tensor Adam / AdamW with global-norm gradient clipping and
an exponential moving average (EMA) of the weights (include/dmx.h dmx_optim, csrc/optim.h).

    opt = dmx.optim.Adam(model.parameters(), lr=1e-4, max_grad_norm=1.0, ema_decay=0.9999)
    ...
    loss.backward(); opt.step(); opt.zero_grad(set_to_none=True)
    with opt.ema_weights():
        sample(model)

``Adam`` is a ``torch.optim.Optimizer``: parameter groups, ``zero_grad``, lr schedulers and the
``state_dict`` layout (per-parameter ``step``, ``exp_avg``, ``exp_avg_sq``, plus ``ema``) are torch
Adam's, so checkpoints move between the two.  The arithmetic follows torch's single-tensor Adam; all of
it runs in three launches of libdmx on the parameters' device (there is no host fallback).  The
library is loaded at the first step, so importing this module needs no GPU.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine import require_cuda

CHUNK = _lib.DMX_OPTIM_CHUNK

# dmx_optim_tensor (include/dmx.h) as a numpy record: a step's rows are filled column-wise
_ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("ema", "<u8"),
                 ("step_size", "<f4"), ("inv_sqrt_bc2", "<f4"), ("lr_wd", "<f4"), ("eps", "<f4"),
                 ("wd", "<f4"), ("omb1", "<f4"), ("beta2", "<f4"), ("omb2", "<f4"),
                 ("flags", "<u4"), ("reserved", "<u4")])
assert _ROW.itemsize == ctypes.sizeof(_lib.OptimTensor)

_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable")


def chunk_table(numels: Iterable[int]) -> List[Tuple[int, int, int]]:
    """The (tensor, offset, length) chunks libdmx cuts a tensor list into (host only, no GPU)."""
    lib = _lib.load()
    numels = [int(x) for x in numels]
    arr = (ctypes.c_int64 * max(len(numels), 1))(*numels)
    count = lib.dmx_optim_chunks(len(numels), arr, None, 0)
    if count < 0:
        raise _lib.DmxError(_lib.DMX_E_ARG, lib.dmx_last_error().decode())
    out = (_lib.OptimChunk * max(count, 1))()
    lib.dmx_optim_chunks(len(numels), arr, out, count)
    return [(out[i].tensor, out[i].offset, out[i].len) for i in range(count)]


def state_layout(params: Iterable[torch.Tensor], ema: bool = False) -> Dict[int, Dict[str, tuple]]:
    """The ``state_dict()['state']`` layout after one step: index -> name -> (shape, dtype).  It is
    ``torch.optim.Adam``'s (``step`` a 0-dim fp32 tensor), with one more entry ``ema`` when EMA is on."""
    out = {}
    for i, p in enumerate(params):
        shape = tuple(p.shape)
        out[i] = {"step": ((), torch.float32), "exp_avg": (shape, p.dtype), "exp_avg_sq": (shape, p.dtype)}
        if ema:
            out[i]["ema"] = (shape, p.dtype)
    return out


class Adam(torch.optim.Optimizer):
    """Adam with coupled weight decay (``decoupled=True``: AdamW), optional clipping of the global
    gradient norm to ``max_grad_norm`` and optional EMA weights with decay ``ema_decay``.

    Parameters must be contiguous fp32 tensors on one HIP device when ``step()`` runs; a parameter
    whose ``.grad`` is None is skipped and its own ``step`` does not advance.  ``amsgrad``,
    ``maximize``, ``capturable``, ``differentiable`` and a ``closure`` are refused."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled: bool = False, max_grad_norm: Optional[float] = None,
                 ema_decay: Optional[float] = None, **refused):
        for name, value in refused.items():
            if name not in _REFUSED:
                raise TypeError(f"unexpected argument {name!r}")
            if value:
                raise ValueError(f"dmx.optim does not implement {name}={value!r}")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"Invalid ema_decay: {ema_decay}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._handle = None
        self._norm = None
        self._stepped = False
        self._swapped = False
        self._bound = False
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled))
        super().__init__(params, defaults)
        self._bound = True
        self._rebind()

    # ---- bookkeeping ----------------------------------------------------------------------------------
    def _rebind(self) -> None:
        """Rebuild the flat parameter list and the per-parameter ``step`` array from ``param_groups`` and
        ``state``.  Every ``step`` entry is a 0-dim view of one fp32 array, so a step advances all of
        them with one vector add."""
        self._release()
        self._params = [p for g in self.param_groups for p in g["params"]]
        self._group_of = np.array([gi for gi, g in enumerate(self.param_groups) for _ in g["params"]], dtype=np.int64)
        n = len(self._params)
        self._steps = np.zeros(n, dtype=np.float32)
        self._views = torch.from_numpy(self._steps)
        self._inited = np.zeros(n, dtype=bool)
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if st and "step" in st:
                self._steps[i] = float(st["step"])
                self._adopt(i, p, st)
            elif self.ema_decay is not None:  # EMA starts as a copy of the parameters at construction
                self._init_state(i, p)
        self._tmpl = None
        self._param_ptrs = None

    def _adopt(self, i: int, p: torch.Tensor, st: dict) -> None:
        st["step"] = self._views[i]
        if self.ema_decay is not None and "ema" not in st:  # (a checkpoint written without EMA)
            st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
        self._inited[i] = True

    def _init_state(self, i: int, p: torch.Tensor) -> None:
        st = self.state[p]
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        self._steps[i] = 0.0
        self._adopt(i, p, st)
        self._tmpl = None

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if self._bound:
            self._rebind()

    def state_dict(self):
        """torch Adam's layout.  Each ``step`` is a copy: torch's ``load_state_dict`` adopts the ``step``
        tensors it is given, and another optimizer must not advance this one's counters."""
        sd = super().state_dict()
        sd["state"] = {k: {**st, "step": st["step"].clone()} if "step" in st else st for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._rebind()

    def __getstate__(self):
        state = dict(super().__getstate__())
        state["dmx"] = {"max_grad_norm": self.max_grad_norm, "ema_decay": self.ema_decay}
        return state

    def __setstate__(self, state) -> None:
        state = dict(state)
        own = state.pop("dmx", None)  # (absent when load_state_dict calls this)
        super().__setstate__(state)
        if own is not None:  # a pickled or copied optimizer: no native object, nothing swapped
            self.__dict__.update(own, _handle=None, _norm=None, _stepped=False, _swapped=False, _bound=True)
        if self.__dict__.get("_bound"):
            self._rebind()

    def _release(self) -> None:
        h, self._handle = self.__dict__.get("_handle"), None
        if h is not None:
            _lib.load().dmx_optim_destroy(h)

    def __del__(self):
        try:
            self._release()
        except Exception:  # interpreter shutdown
            pass

    # ---- the step -------------------------------------------------------------------------------------
    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """The global gradient norm of the last step before clipping: a 0-dim device tensor (a view of
        the buffer the next step overwrites; reading it is the caller's synchronisation), or None
        without ``max_grad_norm`` or before the first step."""
        return self._norm[0] if self.max_grad_norm is not None and self._stepped else None

    @property
    def clip_coef(self) -> Optional[torch.Tensor]:
        """The factor the last step scaled the gradients by, min(1, max_grad_norm / (grad_norm + 1e-6)); a
        0-dim device tensor like grad_norm."""
        return self._norm[1] if self.max_grad_norm is not None and self._stepped else None

    def _check_groups(self) -> None:
        for g in self.param_groups:
            for name in _REFUSED:
                if g.get(name):
                    raise ValueError(f"dmx.optim does not implement {name}={g[name]!r}")

    def _bind_params(self, ptrs: List[int]) -> None:
        """The full check of the parameters and the native object for their sizes; run at the first step
        and whenever a parameter's storage has moved since the last one."""
        params, f32 = self._params, torch.float32
        dev = params[0].device
        require_cuda(params[0], "dmx.optim parameter")
        for p in params:
            if p.device != dev or p.dtype is not f32 or not p.is_contiguous() or p.is_sparse:
                raise ValueError("dmx.optim needs contiguous fp32 parameters on one device")
        numel = tuple(p.numel() for p in params)
        if self._handle is None or self._numel != numel or self._device != dev:
            self._release()
            lib, n, h = _lib.load(), len(params), ctypes.c_void_p()
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            _lib.check(lib.dmx_optim_create(idx, n, (ctypes.c_int64 * n)(*numel), ctypes.byref(h)))
            self._handle, self._numel, self._device = h, numel, dev
            self._norm = torch.zeros(2, dtype=f32, device=dev)
        self._tmpl = None  # (the state tensors are checked against the parameters again)
        self._param_ptrs = ptrs

    @staticmethod
    def _refuse(p: torch.Tensor, g: torch.Tensor) -> None:
        if g.is_sparse:
            raise RuntimeError("dmx.optim does not support sparse gradients")
        if not p.is_contiguous():
            raise ValueError("dmx.optim needs contiguous fp32 parameters on one device")
        raise ValueError("dmx.optim needs a contiguous fp32 gradient on the parameter's device "
                         f"(got {g.dtype}, {g.device}, contiguous={g.is_contiguous()})")

    def _hyper_key(self) -> tuple:
        return tuple((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                      bool(g.get("decoupled_weight_decay", False))) for g in self.param_groups)

    def _template(self, key: tuple) -> None:
        """The rows' columns that hold from step to step: the optimizer's own tensors (fixed until the state
        is rebuilt) and what follows from the groups' hyperparameters alone (rebuilt when `key` changes)."""
        params, dev, f32 = self._params, self._device, torch.float32
        sts = [self.state.get(p) or {} for p in params]
        ema_on = self.ema_decay is not None
        for p, st in zip(params, sts):
            for k in ("exp_avg", "exp_avg_sq", "ema"):
                t = st.get(k)
                if t is not None and (t.device != dev or t.dtype is not f32 or not t.is_contiguous()
                                      or t.shape != p.shape):
                    raise ValueError(f"optimizer state {k} does not match its parameter (device, dtype or layout); "
                                     "build the optimizer after moving the model")
        rows = np.zeros(len(params), dtype=_ROW)
        for col, k in (("m", "exp_avg"), ("v", "exp_avg_sq"), ("ema", "ema")):
            rows[col] = [st[k].data_ptr() if k in st and (k != "ema" or ema_on) else 0 for st in sts]
        lr, b1, b2, eps, wd, dec = (np.array(c)[self._group_of] for c in zip(*key))
        rows["lr_wd"] = np.where(dec, lr * wd, 0.0)
        rows["eps"] = eps
        rows["wd"] = np.where(dec, 0.0, wd)
        rows["omb1"] = 1.0 - b1
        rows["beta2"] = b2
        rows["omb2"] = 1.0 - b2
        rows["flags"] = np.where(dec, _lib.DMX_OPTIM_DECOUPLED, 0)
        self._tmpl, self._tmpl_key, self._lr, self._b1, self._b2 = rows, key, lr, b1, b2

    @torch.no_grad()
    def step(self, closure=None) -> None:
        if closure is not None:
            raise ValueError("dmx.optim does not implement closure")
        self._check_groups()
        if self._swapped:
            raise RuntimeError("step() inside ema_weights(): the parameters hold the EMA weights")
        if sum(len(g["params"]) for g in self.param_groups) != len(self._params):
            self._rebind()
        params = self._params
        n = len(params)
        if n == 0:
            return
        ptrs = [p.data_ptr() for p in params]
        if ptrs != self._param_ptrs:
            self._bind_params(ptrs)
        # The pointers of this step's gradients, read afresh.  torch keeps a .grad on its parameter's device
        # with its shape (the .grad setter and autograd's accumulation refuse anything else); its dtype may
        # differ (grad_dtype), and it may be sparse or strided.
        f32 = torch.float32
        grads = [p.grad for p in params]
        gptrs = []
        for p, g in zip(params, grads):
            if g is None:
                gptrs.append(0)
            elif g.is_sparse or g.dtype is not f32 or not g.is_contiguous() or not p.is_contiguous():
                self._refuse(p, g)
            else:
                gptrs.append(g.data_ptr())
        has = np.array([g is not None for g in grads])
        new = has & ~self._inited
        if new.any():
            for i in np.flatnonzero(new):
                self._init_state(int(i), params[int(i)])
        key = self._hyper_key()
        if self._tmpl is None or self._tmpl_key != key:
            self._template(key)
        rows = self._tmpl.copy()
        rows["p"] = ptrs
        rows["g"] = gptrs
        self._steps[has] += 1.0
        s = np.where(has, self._steps, 1.0).astype(np.float64)  # (skipped rows: any finite value)
        rows["step_size"] = self._lr / (1.0 - self._b1 ** s)
        rows["inv_sqrt_bc2"] = 1.0 / np.sqrt(1.0 - self._b2 ** s)
        lib = _lib.load()
        stream = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(lib.dmx_optim_set_step(self._handle, rows.ctypes.data, n, stream))
        d = self.ema_decay if self.ema_decay is not None else 0.0
        _lib.check(lib.dmx_optim_step(self._handle, self.max_grad_norm or 0.0, d, 1.0 - d,
                                      self._norm.data_ptr(), stream))
        self._stepped = True
        # the kernels write through raw pointers: tell autograd (and NativeBacked.native()) that the values changed
        touched = [p for p, g in zip(params, grads) if g is not None]
        if touched:
            torch.autograd.graph.increment_version(touched)

    # ---- EMA weights ------------------------------------------------------------------------------------
    def _ema_pairs(self) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        if self.ema_decay is None:
            raise RuntimeError("this optimizer keeps no EMA weights (ema_decay=None)")
        return self._params, [self.state[p]["ema"] for p in self._params]

    def _swap(self) -> None:
        params, emas = self._ema_pairs()
        if not params:
            return
        ps, es = [p.data for p in params], [e.data for e in emas]
        tmp = [t.clone() for t in ps]
        torch._foreach_copy_(ps, es)
        torch._foreach_copy_(es, tmp)
        torch.autograd.graph.increment_version(params)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameters hold the EMA weights (and the EMA tensors the parameters):
        swapped in place, bit for bit, and swapped back on exit, also when the block raises."""
        if self._swapped:
            raise RuntimeError("ema_weights() is not re-entrant")
        self._swap()
        self._swapped = True
        try:
            yield self
        finally:
            self._swap()
            self._swapped = False

    @torch.no_grad()
    def copy_ema_to(self, module_or_params) -> None:
        """Copy the EMA weights into a module's parameters (``parameters()`` order) or a list of tensors."""
        _, emas = self._ema_pairs()
        dst = list(module_or_params.parameters()) if isinstance(module_or_params, torch.nn.Module) \
            else list(module_or_params)
        if len(dst) != len(emas) or any(a.shape != b.shape for a, b in zip(dst, emas)):
            raise ValueError("copy_ema_to: the destination does not match the optimizer's parameters")
        if self._swapped:
            raise RuntimeError("copy_ema_to() inside ema_weights(): the parameters already hold the EMA weights")
        if dst:
            torch._foreach_copy_([t.data for t in dst], [e.data for e in emas])
            torch.autograd.graph.increment_version(dst)


class AdamW(Adam):
    """``Adam`` with decoupled weight decay and torch AdamW's defaults (``weight_decay=1e-2``)."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, **kwargs):
        if "decoupled" in kwargs:
            raise TypeError("AdamW is always decoupled; use Adam(decoupled=False) for coupled decay")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=True, **kwargs)
