"""Python side of the native engine: contexts, weight loading, step / loop / decode.

All arithmetic happens in libdmx.so (HIP kernels for gfx950).  This module only
moves pointers: torch provides device memory and streams.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import DdimSched, DpmSched, Guidance, InvertSched, KnownSched, StepArgs, check

TIME_DIM = 256


def pos_table(tmax: int) -> torch.Tensor:
    """pos[t-1] for t = 1..tmax with the reference's exact fp32 formula
    (models/unet_cond.py:155-161: long t repeated, times the fp32 inv_freq, sin|cos)."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, TIME_DIM, 2).float() / TIME_DIM))
    t = torch.arange(1, tmax + 1, dtype=torch.long).unsqueeze(-1)
    tt = t.repeat(1, TIME_DIM // 2) * inv_freq
    return torch.cat([torch.sin(tt), torch.cos(tt)], dim=-1).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class Context:
    """One dmx_ctx per device per process."""

    _ctxs: Dict[int, "Context"] = {}
    _lock = threading.Lock()

    def __init__(self, index: int):
        self.lib = _lib.load()
        self.index = index
        h = ctypes.c_void_p()
        check(self.lib.dmx_create(index, ctypes.byref(h)))
        self.handle = h
        self.tmax = 0

    @classmethod
    def get(cls, device: torch.device) -> "Context":
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with cls._lock:
            if idx not in cls._ctxs:
                cls._ctxs[idx] = Context(idx)
            return cls._ctxs[idx]

    def ensure_time_table(self, tmax: int) -> None:
        if tmax <= self.tmax:
            return
        tmax = max(tmax, 1000)
        tab = pos_table(tmax)
        check(self.lib.dmx_set_time_table(self.handle, ctypes.c_void_p(tab.data_ptr()), tmax))
        self.tmax = tmax


def require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.DmxUnavailable(
            f"{what} is on {t.device}; the dmx path runs only on an MI355X (HIP) device — move the model and "
            f"inputs with .to('cuda') (there is no CPU fallback)")


class NativeModel:
    """A repacked copy of one reference network inside libdmx (U-Net or VAE)."""

    def __init__(self, kind: int, params: Dict[str, torch.Tensor], in_ch: int = 4, remove_deep_conv: bool = False,
                 **cfg):
        self.kind = kind
        self.in_ch = in_ch
        some = next(iter(params.values()))
        require_cuda(some, "model weights")
        self.device = some.device
        self.ctx = Context.get(self.device)
        self.lib = self.ctx.lib
        h = ctypes.c_void_p()
        conf = _lib.ModelConfig.make(kind, in_ch, remove_deep_conv, **cfg)
        self.geom_dim = int(conf.geom_dim)
        self.keys = _lib.model_keys(kind, in_ch, remove_deep_conv, **cfg)
        check(self.lib.dmx_model_create_cfg(self.ctx.handle, ctypes.byref(conf), ctypes.byref(h)))
        self.handle = h
        keep = []
        for name, t in params.items():
            tt = t.detach().to(dtype=torch.float32).contiguous()
            keep.append(tt)
            shape = (ctypes.c_int64 * max(tt.dim(), 1))(*tt.shape)
            check(self.lib.dmx_model_set_tensor(self.handle, name.encode(), ctypes.c_void_p(tt.data_ptr()), shape,
                                                tt.dim()))
        with torch.cuda.device(self.device):
            check(self.lib.dmx_model_finalize(self.handle, ctypes.c_void_p(_stream(self.device))))
        # the registered tensors (views of the module's fp32 parameters, or converted copies) are
        # re-read by refresh() and the training entry points (include/dmx.h dmx_model_set_tensor)
        self._registered = keep
        self.aliases_params = all(k.data_ptr() == p.data_ptr() for k, p in zip(keep, params.values()))
        self._side_stream = None
        env = os.environ.get("DMX_PRECISION")
        if env:
            self.set_precision(env)

    PRECISIONS = {"fp32": 0, "x3": 1, "f16": 2}

    def set_precision(self, prec) -> None:
        """GEMM arithmetic: "x3" (default; fp32 split into fp16 hi+lo, 3 MFMAs, fp32 accumulate),
        "fp32" (fp32 MFMA, exact fp32 products) or "f16" (BASELINE config 4: GEMM / attention
        operands rounded to fp16, one MFMA, fp32 accumulate; norms, softmax and the scheduler stay fp32)."""
        code = self.PRECISIONS[prec] if isinstance(prec, str) else int(prec)
        check(self.lib.dmx_model_set_precision(self.handle, code))

    PREDICTIONS = {"eps": 0, "v": 1}

    def set_prediction(self, kind, p_o=None, p_x=None, *, d_s=None, d_d=None) -> None:
        """What the network predicts (include/dmx.h dmx_model_set_prediction): "eps" (the default), or "v"
        with the (T,) fp32 tables p_o = sqrt(ab), p_x = sqrt(1 - ab) (Diffuser.noise_tables) — every step
        and loop then converts its mixed output to eps before the update.  The library copies the tables;
        a change of kind or tables drops the captured graphs and the cached deep feature.  The pair last
        given is remembered by identity, so repeating a call costs nothing.
        d_s, d_d (with "v"; both or neither): the (T,) fp32 tables of the x0-form (Diffuser.x0_tables;
        include/dmx.h dmx_model_set_prediction_x0) — the steps then convert to (x0, eps) and update without a
        division, as a zero-terminal-SNR schedule needs; `prediction` stays "v" and `x0_form` turns True."""
        if kind not in self.PREDICTIONS:
            raise ValueError(f'prediction must be "eps" or "v" (got {kind!r})')
        if (d_s is None) != (d_d is None) or (d_s is not None and kind != "v"):
            raise ValueError('d_s and d_d are given together, and with prediction "v" only')
        last = getattr(self, "_prediction", ("eps", None, None, None, None))
        if last[0] == kind and (kind == "eps" or all(a is b for a, b in zip(last[1:], (p_o, p_x, d_s, d_d)))):
            return
        po_c = px_c = None
        T = 0
        if kind == "v":
            if p_o is None or p_x is None:
                raise ValueError('prediction "v" needs the p_o and p_x tables (Diffuser.noise_tables)')
            po_c = p_o.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
            px_c = p_x.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
            T = int(po_c.numel())
            if T < 1 or px_c.numel() != T:
                raise ValueError(f"p_o and p_x must be equal non-empty tables (got {po_c.numel()}, {px_c.numel()})")
        ds_c = dd_c = None
        if d_s is not None:
            ds_c = d_s.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
            dd_c = d_d.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
            if ds_c.numel() != T or dd_c.numel() != T:
                raise ValueError(f"d_s and d_d must have p_o's {T} entries (got {ds_c.numel()}, {dd_c.numel()})")
        with torch.cuda.device(self.device):
            if ds_c is not None:
                check(self.lib.dmx_model_set_prediction_x0(self.handle, _ptr(po_c), _ptr(px_c), _ptr(ds_c), _ptr(dd_c),
                                                           T, ctypes.c_void_p(_stream(self.device))))
            else:
                check(self.lib.dmx_model_set_prediction(self.handle, self.PREDICTIONS[kind], _ptr(po_c), _ptr(px_c),
                                                        T, ctypes.c_void_p(_stream(self.device))))
        self._prediction = (kind, p_o, p_x, d_s, d_d)  # (the tensors are kept: their identity stays valid)

    PRED_V_X0 = 2  # (include/dmx.h DMX_PRED_V_X0: "v" in x0-form)

    @property
    def prediction(self) -> str:
        code = self.lib.dmx_model_get_prediction(self.handle)
        return "v" if code == self.PRED_V_X0 else {v: k for k, v in self.PREDICTIONS.items()}[code]

    @property
    def x0_form(self) -> bool:
        return self.lib.dmx_model_get_prediction(self.handle) == self.PRED_V_X0

    def range_tripped(self, reset: bool = True) -> bool:
        """True when an output kernel saw a non-finite value since the last reset (include/dmx.h
        dmx_model_range_check: the split-precision range guard).  Synchronises the current stream."""
        f = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            check(self.lib.dmx_model_range_check(self.handle, int(reset), ctypes.byref(f),
                                                 ctypes.c_void_p(_stream(self.device))))
        return bool(f.value)

    @contextlib.contextmanager
    def precision_override(self, prec):
        old = self.precision
        self.set_precision(prec)
        try:
            yield self
        finally:
            self.set_precision(old)

    @property
    def precision(self) -> str:
        code = self.lib.dmx_model_get_precision(self.handle)
        return {v: k for k, v in self.PRECISIONS.items()}[code]

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.dmx_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def refresh(self) -> None:
        """Parameters changed in place (optimizer.step / load_state_dict): repack on the device."""
        with torch.cuda.device(self.device):
            check(self.lib.dmx_model_refresh(self.handle, ctypes.c_void_p(_stream(self.device))))

    # ---- training (include/dmx.h dmx_train_forward / dmx_train_backward) --------------------
    def train_forward(self, x, t, y, vals=None, mask=None, tmax=None):
        """Forward with a tape for dmx_train_backward -> (eps, geom or None, tape id).  tmax: an upper
        bound of t the caller vouches for (timesteps drawn in [1, tmax]); t is then not read back, so
        the call does not wait for the device."""
        require_cuda(x, "x")
        n, c, h, w = x.shape
        dev = x.device
        if tmax is not None:
            self.ctx.ensure_time_table(max(1000, int(tmax)))
        else:
            self.ctx.ensure_time_table(max(1000, int(t.max().item()) if t.numel() else 1))
        x = x.detach().to(dtype=torch.float32).contiguous()
        t = t.to(device=dev, dtype=torch.long).contiguous()
        y = y.to(device=dev, dtype=torch.long).contiguous()
        if vals is not None:
            vals = vals.detach().to(device=dev, dtype=torch.float32).contiguous()
            mask = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
        eps = torch.empty_like(x)
        geom = (torch.empty((n, self.geom_dim), device=dev, dtype=torch.float32)
                if self.kind == _lib.DMX_UNET_COND_GEOM else None)
        tid = ctypes.c_int64()
        with torch.cuda.device(dev):
            check(self.lib.dmx_train_forward(self.handle, _ptr(x), _ptr(t), _ptr(y), _ptr(vals), _ptr(mask), n, h, w,
                                             _ptr(eps), _ptr(geom), ctypes.byref(tid),
                                             ctypes.c_void_p(_stream(dev))))
        self._live_train = (x, t, y, vals, mask)
        return eps, geom, int(tid.value)

    def train_backward(self, tape_id: int, d_eps=None, d_geom=None) -> Dict[str, torch.Tensor]:
        """dLoss/dparam for every state_dict key, given dLoss/deps and dLoss/dgeom (None = 0)."""
        dev = self.device
        grads = {name: torch.empty(shape, device=dev, dtype=torch.float32) for name, shape in self.keys}
        ptrs = (ctypes.c_void_p * len(self.keys))(*[grads[name].data_ptr() for name, _ in self.keys])
        if d_eps is not None:
            d_eps = d_eps.to(device=dev, dtype=torch.float32).contiguous()
        if d_geom is not None:
            d_geom = d_geom.to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            check(self.lib.dmx_train_backward(self.handle, int(tape_id), _ptr(d_eps), _ptr(d_geom), ptrs,
                                              len(self.keys), ctypes.c_void_p(_stream(dev))))
        self._live_bwd = (d_eps, d_geom)
        return grads

    def input_grad(self, tape_id: int, d_eps=None, d_geom=None) -> torch.Tensor:
        """dLoss/dx (n,c,h,w) of the taped forward's x, given dLoss/deps and dLoss/dgeom (None = 0): the
        data-only backward (include/dmx.h dmx_train_backward_input).  No parameter gradient is computed;
        a train_backward on the same tape afterwards is unaffected."""
        live = getattr(self, "_live_train", None)
        if live is None:
            raise _lib.DmxError(_lib.DMX_E_ARG, "no training forward recorded (train_forward)")
        dev = self.device
        if d_eps is not None:
            d_eps = d_eps.to(device=dev, dtype=torch.float32).contiguous()
        if d_geom is not None:
            d_geom = d_geom.to(device=dev, dtype=torch.float32).contiguous()
        d_x = torch.empty_like(live[0])
        with torch.cuda.device(dev):
            check(self.lib.dmx_train_backward_input(self.handle, int(tape_id), _ptr(d_eps), _ptr(d_geom), _ptr(d_x),
                                                    ctypes.c_void_p(_stream(dev))))
        self._live_bwd = (d_eps, d_geom)
        return d_x

    def geom_grad(self, x, t, y, vals, mask):
        """The geometry-guidance loss of x at timesteps t and its input gradient ->
        (loss (n,), grad (n,c,h,w), geom (n,geom_dim), eps): the taped forward of (x, t, y, vals, mask),
        L_n = sum_j m_nj (geom_nj - v_nj)^2 / max(sum_j m_nj, 1e-6) against the same vals / mask
        (include/dmx.h dmx_geom_seed) and dL_n/dx by the data-only backward.  Replaces the training tape."""
        if self.kind != _lib.DMX_UNET_COND_GEOM:
            raise ValueError("geom_grad needs a model with a GeomHead (UnetCondWithGeomHead)")
        if vals is None or mask is None:
            raise ValueError("geom_grad needs cond_vals and cond_mask (the loss's target)")
        eps, geom, tape = self.train_forward(x, t, y, vals, mask)
        _, _, _, vals_c, mask_c = self._live_train
        n = geom.shape[0]
        loss = torch.empty((n,), device=geom.device, dtype=torch.float32)
        seed = torch.empty_like(geom)
        with torch.cuda.device(geom.device):
            check(self.lib.dmx_geom_seed(_ptr(geom), _ptr(vals_c), _ptr(mask_c), n, self.geom_dim, _ptr(loss),
                                         _ptr(seed), ctypes.c_void_p(_stream(geom.device))))
        return loss, self.input_grad(tape, None, seed), geom, eps

    def workspace_bytes(self) -> int:
        return int(self.lib.dmx_model_workspace_bytes(self.handle))

    def graph_captures(self) -> int:
        """Graph pairs (1-step + 8-step) captured by sample_loop since the model was created."""
        return int(self.lib.dmx_model_graph_captures(self.handle))

    # ---- U-Net ---------------------------------------------------------------------------
    def forward(self, x, t, y=None, vals=None, mask=None, want_geom=False, perturb=None):
        """The network's forward -> (eps, geom or None).  perturb = (blocks, row0, row1): the samples
        [row0, row1) run with identity attention in the blocks of `blocks` (bit i: sa(i+1); include/dmx.h
        dmx_unet_forward_perturbed); the other samples keep the bits of the plain forward."""
        n, c, h, w = x.shape
        self.ctx.ensure_time_table(int(t.max().item()) if t.numel() else 1)
        x = x.contiguous().float()
        t = t.to(device=x.device, dtype=torch.long).contiguous()
        if y is not None:
            y = y.to(device=x.device, dtype=torch.long).contiguous()
        if vals is not None:
            vals = vals.to(device=x.device, dtype=torch.float32).contiguous()
            mask = mask.to(device=x.device, dtype=torch.float32).contiguous()
        eps = torch.empty_like(x)
        geom = torch.empty((n, self.geom_dim), device=x.device, dtype=torch.float32) if want_geom else None
        with torch.cuda.device(x.device):
            if perturb is not None:
                blocks, row0, row1 = (int(v) for v in perturb)
                if not 1 <= blocks < 64 or not 0 <= row0 < row1 <= n:
                    raise ValueError(f"perturb must be (blocks in [1, 63], row0, row1) with 0 <= row0 < row1 <= {n} "
                                     f"(got {tuple(perturb)!r})")
                check(self.lib.dmx_unet_forward_perturbed(self.handle, _ptr(x), _ptr(t), _ptr(y), _ptr(vals),
                                                          _ptr(mask), _ptr(eps), _ptr(geom), n, h, w, blocks, row0,
                                                          row1, ctypes.c_void_p(_stream(x.device))))
            else:
                check(self.lib.dmx_unet_forward(self.handle, _ptr(x), _ptr(t), _ptr(y), _ptr(vals), _ptr(mask),
                                                _ptr(eps), _ptr(geom), n, h, w, ctypes.c_void_p(_stream(x.device))))
        return eps, geom

    def forward_taps(self, x, t, y=None, vals=None, mask=None):
        """Forward with debug taps -> {name: flat float32 tensor (NHWC order)}."""
        check(self.lib.dmx_debug_enable(self.handle, 1))
        try:
            eps, geom = self.forward(x, t, y, vals, mask, want_geom=self.kind == _lib.DMX_UNET_COND_GEOM)
            out = {}
            buf = ctypes.create_string_buffer(128)
            cnt = ctypes.c_int64()
            for i in range(self.lib.dmx_debug_num_taps(self.handle)):
                check(self.lib.dmx_debug_tap(self.handle, i, buf, 128, ctypes.byref(cnt), None, None))
                dst = torch.empty(cnt.value, device=x.device, dtype=torch.float32)
                check(self.lib.dmx_debug_tap(self.handle, i, buf, 128, ctypes.byref(cnt), _ptr(dst),
                                             ctypes.c_void_p(_stream(x.device))))
                out[buf.value.decode()] = dst
            torch.cuda.synchronize(x.device)
            out["eps"] = eps
            return out
        finally:
            check(self.lib.dmx_debug_enable(self.handle, 0))

    def _norm_inputs(self, x_in, t, y, vals, mask, noise):
        """The kernels read raw bytes: t / y as contiguous int64, vals / mask / noise as contiguous fp32,
        all on x's device (a bool cond_mask, float64 values or a column slice are converted here, as the
        reference's torch.cat / arithmetic would promote them).  The converted tensors are kept alive on
        the model until the next call so the enqueued launches never read freed memory."""
        dev = x_in.device
        t = t.to(device=dev, dtype=torch.long).contiguous()
        if y is not None:
            y = y.to(device=dev, dtype=torch.long).contiguous()
        if vals is not None:
            vals = vals.to(device=dev, dtype=torch.float32).contiguous()
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.float32).contiguous()
        if noise is not None:
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
        self._live = (t, y, vals, mask, noise)
        return t, y, vals, mask, noise

    def _args(self, x_in, x_out, t, t_stride, y, null_label, vals, mask, guidance, tables, noise, seed,
              sample_offset) -> StepArgs:
        n, _, h, w = x_in.shape
        a = StepArgs()
        a.x_in, a.x_out = x_in.data_ptr(), x_out.data_ptr()
        a.t, a.t_stride = t.data_ptr(), t_stride
        a.y = y.data_ptr() if y is not None else None
        a.null_label = int(null_label)
        a.vals = vals.data_ptr() if vals is not None else None
        a.mask = mask.data_ptr() if mask is not None else None
        a.guidance = float(guidance)
        if tables is not None:  # (None: the strided calls, which read their schedule instead)
            c1, c2, sd = tables
            a.c1, a.c2, a.sd, a.T = c1.data_ptr(), c2.data_ptr(), sd.data_ptr(), int(c1.numel())
        a.noise = noise.data_ptr() if noise is not None else None
        a.seed, a.sample_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset)
        a.n, a.h, a.w = n, h, w
        return a

    def _sched(self, sched, device, hist=None, x=None):
        """dmx_ddim_sched of a (t_map, k_e, k_a, k_s, k_d, k_n) tuple (Diffuser.ddim_tables) on `device`,
        or dmx_dpm_sched of a DpmSchedule (Diffuser.dpm_tables) with its history buffer `hist` (x's shape);
        makes sure the time table reaches the schedule's last timestep.  That timestep is read back
        once per schedule: the tuple is kept (alive, so its identity stays valid) with the value."""
        if isinstance(sched, DpmSchedule):
            sc = _dpm_struct(sched, device, hist, x)
        else:
            if hist is not None:
                raise ValueError("hist belongs to a DPM schedule (Diffuser.dpm_tables)")
            sc = _sched_struct(sched, device)
        last = getattr(self, "_sched_last", None)
        if last is None or last[0] is not sched[0]:
            last = self._sched_last = (sched[0], int(sched[0][-1].item()))
        self.ctx.ensure_time_table(last[1])
        return sc

    def _mode(self, x, sched, hist, known, rescale, guidance, y, tables):
        """The optional parts of a step or loop on x, as documented there -> (the ddim, dpm, known and
        guidance arguments of dmx_step_guided / dmx_sample_loop_guided, the tables its step args carry:
        None with a schedule).  rescale 0 goes as a guidance struct too: the library then runs exactly
        the plain / known-region call.  Makes sure the time table reaches the last timestep."""
        gd = _guidance_struct(rescale, guidance, y)
        kn = _known_struct(known, x.device, x, need_mask=True) if known is not None else None
        sc = None
        if sched is not None:
            sc = self._sched(sched, x.device, hist, x)
            tables = None
        else:
            self.ctx.ensure_time_table(int(tables[0].numel()))
        dpm = isinstance(sc, DpmSched)
        parts = (None if dpm else sc, sc if dpm else None, kn, gd if gd is not None else Guidance(0.0))
        return tuple(None if s is None else ctypes.byref(s) for s in parts), tables

    def _compose(self, x, compose, rescale):
        """The C view of compose = (y_rows, vals_rows, mask_rows, weights) for a step on x (n samples):
        y_rows (K+1, n) int64, row 0 the base branch; vals_rows / mask_rows (K+1, n, 12) or both None;
        weights (K, n) fp32 -> (dmx_compose, the converted tensors, which the caller keeps alive).
        Shapes, K and finiteness of nothing are read back here: the library checks K and the pointers."""
        if float(rescale) > 0:
            raise ValueError("a composed step takes no guidance rescale")
        y_rows, vals_rows, mask_rows, weights = compose
        dev, n = x.device, x.shape[0]
        y_c = torch.as_tensor(y_rows).to(device=dev, dtype=torch.long).contiguous()
        w_c = torch.as_tensor(weights).to(device=dev, dtype=torch.float32).contiguous()
        if y_c.dim() != 2 or y_c.shape[1] != n or not 2 <= y_c.shape[0] <= _lib.DMX_COMPOSE_MAX + 1:
            raise ValueError(f"compose y_rows must be (K+1, {n}) with 1 <= K <= {_lib.DMX_COMPOSE_MAX} "
                             f"(got {tuple(y_c.shape)})")
        K = y_c.shape[0] - 1
        if tuple(w_c.shape) != (K, n):
            raise ValueError(f"compose weights must be ({K}, {n}) (got {tuple(w_c.shape)})")
        if (vals_rows is None) != (mask_rows is None):
            raise ValueError("compose vals_rows and mask_rows must be given together")
        v_c = m_c = None
        if vals_rows is not None:
            v_c = torch.as_tensor(vals_rows).to(device=dev, dtype=torch.float32).contiguous()
            m_c = torch.as_tensor(mask_rows).to(device=dev, dtype=torch.float32).contiguous()
            for r, nm in ((v_c, "vals_rows"), (m_c, "mask_rows")):
                if tuple(r.shape) != (K + 1, n, 12):
                    raise ValueError(f"compose {nm} must be ({K + 1}, {n}, 12) (got {tuple(r.shape)})")
        comp = _lib.Compose(K, y_c.data_ptr(), v_c.data_ptr() if v_c is not None else None,
                            m_c.data_ptr() if m_c is not None else None, w_c.data_ptr())
        return comp, (y_c, v_c, m_c, w_c)

    def _geom(self, x, geom, sched, tables, rescale, compose, guidance, y, vals, mask):
        """The C view of geom = (scale, sig) for a step on x (n samples): scale (n,) and sig (S,) contiguous
        fp32 on x's device, S the positions of the step's schedule (the DDPM step: T); nothing is
        converted, the kernels (and a loop's graphs) read the caller's tensors."""
        if self.kind != _lib.DMX_UNET_COND_GEOM:
            raise ValueError("geometry guidance needs a model with a GeomHead (UnetCondWithGeomHead)")
        if compose is not None or float(rescale) > 0:
            raise ValueError("a geometry-guided step takes no composition and no guidance rescale")
        if y is None or not float(guidance) > 0 or vals is None or mask is None:
            raise ValueError("a geometry-guided step is a CFG step with a condition: it needs y, guidance > 0, "
                             "vals and mask")
        if not isinstance(geom, (tuple, list)) or len(geom) != 2:
            raise ValueError("geom must be the pair (scale, sig)")
        scale, sig = geom
        S = int(sched[0].numel()) if sched is not None else int(tables[0].numel())
        for v, nm, cnt in ((scale, "scale", x.shape[0]), (sig, "sig", S)):
            if (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 1 or v.numel() != cnt
                    or not v.is_contiguous() or v.device != x.device):
                raise ValueError(f"geom {nm} must be a contiguous 1-D fp32 tensor of {cnt} entries on {x.device}")
        return _lib.GeomGuide(scale.data_ptr(), sig.data_ptr(), S)

    @staticmethod
    def _perturb(perturb, compose, geom):
        """The C view of perturb = (blocks, branches) (include/dmx.h dmx_perturb): bit i of blocks is sa(i+1),
        bit k of branches is branch k of `compose`.  The library checks that the branches are the
        composition's trailing ones."""
        if compose is None:
            raise ValueError("perturb needs compose (the perturbed branches are branches of a composition)")
        if geom is not None:
            raise ValueError("a perturbed step takes no geometry guidance")
        if not isinstance(perturb, (tuple, list)) or len(perturb) != 2:
            raise ValueError("perturb must be the pair (blocks, branches)")
        blocks, branches = int(perturb[0]), int(perturb[1])
        if not 1 <= blocks < 64 or not 1 <= branches < 2 ** (_lib.DMX_COMPOSE_MAX + 1):
            raise ValueError(f"perturb blocks must lie in [1, 63] and branches in [1, {2 ** (_lib.DMX_COMPOSE_MAX + 1) - 1}] "
                             f"(got {tuple(perturb)!r})")
        return _lib.Perturb(blocks, branches)

    @staticmethod
    def _cache(cache, compose, geom, perturb, invert):
        """The C view of cache = (interval, phase) (include/dmx.h dmx_cache), or None for no request: None
        itself and every interval 1.  A cached step takes none of the parts named here."""
        if cache is None:
            return None
        if not isinstance(cache, (tuple, list)) or len(cache) != 2:
            raise ValueError("cache must be the pair (interval, phase)")
        n, phase = cache
        for v, nm, lo in ((n, "interval", 1), (phase, "phase", 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"cache {nm} must be an int >= {lo} (got {v!r})")
        if n == 1:
            return None
        given = [nm for nm, v in (("compose", compose), ("geom", geom), ("perturb", perturb), ("invert", invert))
                 if v is not None]
        if given:
            raise ValueError(f"a cached step (cache interval > 1) takes no {' / '.join(given)}")
        return _lib.Cache(n, phase)

    def cached_features(self) -> Optional[torch.Tensor]:
        """A copy of the deep feature D the last refresh step of a cached call left in the model —
        (rows, h/2, w/2, 64) fp32, rows = 2B in a CFG step (null half first), the output of sa5 — or
        None while the model holds no valid one.  Read-only diagnostic: for tests, and for measuring
        how far D drifts between the steps of a real checkpoint."""
        shape = (ctypes.c_int64 * 4)()
        with torch.cuda.device(self.device):
            st = ctypes.c_void_p(_stream(self.device))
            check(self.lib.dmx_model_cached_features(self.handle, shape, None, st))
            if shape[0] == 0:
                return None
            out = torch.empty(tuple(int(v) for v in shape), device=self.device, dtype=torch.float32)
            check(self.lib.dmx_model_cached_features(self.handle, shape, _ptr(out), st))
        return out

    def _invert(self, x, invert, sched, hist, known, rescale, compose, geom, perturb, noise=None):
        """The C view of invert = (tables, src) for a step or loop on x, which takes no other optional part;
        makes sure the time table reaches the rows' largest timestep (read back once per table tuple,
        which is kept alive with the value)."""
        others = (("sched", sched), ("hist", hist), ("known", known), ("compose", compose), ("geom", geom),
                  ("perturb", perturb), ("noise", noise))
        given = [nm for nm, v in others if v is not None] + (["rescale"] if float(rescale) > 0 else [])
        if given:
            raise ValueError(f"an inversion step takes no {' / '.join(given)}")
        if not isinstance(invert, (tuple, list)) or len(invert) != 2:
            raise ValueError("invert must be the pair (tables, src)")
        tables, src = invert
        iv = _invert_struct(tables, x.device, src, x)
        last = getattr(self, "_invert_last", None)
        if last is None or last[0] is not tables[0]:
            last = self._invert_last = (tables[0], int(tables[0].max().item()))
        self.ctx.ensure_time_table(last[1])
        return iv

    def step(self, x_in, x_out, t, y, null_label, vals, mask, guidance, tables, noise=None, seed=0,
             sample_offset=0, t_stride=1, sched=None, hist=None, known=None, rescale=0.0, compose=None, geom=None,
             perturb=None, invert=None, cache=None):
        """One denoising step: CFG (2n batched forward) when guidance > 0 and y given.

        sched (the 6-tuple of Diffuser.ddim_tables): one strided DDIM step instead; `t` then holds
        positions in [1, S] and `tables` is not read (may be None).
        sched a DpmSchedule (Diffuser.dpm_tables) with hist (x's shape, updated in place): one
        DPM-Solver++(2M) step; `noise` must be None and `seed` is not read.
        known (z0, e0, mask, q_a, q_e) with the tables of Diffuser.known_tables for the step's schedule
        (the DDPM step: tau = 1..T): the known-region blend follows the step on x_out (known_blend).
        rescale = phi in (0, 1] (a CFG step only; include/dmx.h dmx_guidance): the guided prediction is
        scaled per sample to the conditional one's standard deviation before the update.  0 is the
        plain step, launched exactly as without the keyword.
        compose = (y_rows, vals_rows, mask_rows, weights) (include/dmx.h dmx_compose; _compose): composed
        guidance over K + 1 branches in one (K+1) n forward — eps = e_0 + sum_k w_k (e_k - e_0).  y,
        null_label, vals, mask and guidance are then not read; rescale must be 0.
        geom = (scale (n,), sig (S,)) (include/dmx.h dmx_geom_guide; _geom): geometry guidance — a CFG step
        whose prediction gains (scale[n] sig[p-1]) dL_n/dx, L_n the GeomHead's masked regression loss
        against the step's own vals / mask.  UnetCondWithGeomHead only; no rescale, no compose.  The
        step replaces the training tape.  None is the plain step, launched exactly as without the keyword.
        perturb = (blocks, branches) (include/dmx.h dmx_perturb; with compose only): perturbed-attention
        guidance — the branches of bit mask `branches` (the composition's trailing ones) run with identity
        attention in the blocks of bit mask `blocks` (bit i: sa(i+1)).  None is the composed step.
        invert = (tables, src) (include/dmx.h dmx_invert_sched; tables: Diffuser.invert_tables, src: fp32,
        x's shape, not x): one row of a DDIM inversion instead — `t` holds countdown positions in [1, N],
        x_out = i_x src + i_e eps and src takes it on the last row of a position.  `tables`, `noise` and
        `seed` are not read, and no other optional part may be given.
        cache = (N, phase) (include/dmx.h dmx_cache): feature caching — the step refreshes the model's deep
        feature (sa5's output) where phase % N == 0, which is the plain step bit for bit, and otherwise runs
        only inc, up3, sa6 and the head on the stored one.  With sched / hist / known / rescale only; None
        and N = 1 are the step without the keyword."""
        _check_state(x_in, "x")
        _check_state(x_out, "x_out")
        ch = self._cache(cache, compose, geom, perturb, invert)
        iv = None
        if invert is not None:
            iv = self._invert(x_in, invert, sched, hist, known, rescale, compose, geom, perturb, noise)
        pt = self._perturb(perturb, compose, geom) if perturb is not None else None
        gg = None
        if geom is not None:
            gg = self._geom(x_in, geom, sched, tables, rescale, compose, guidance, y, vals, mask)
            self._live_geom = tuple(geom)
        if compose is not None:
            comp, self._live_comp = self._compose(x_in, compose, rescale)
            y = vals = mask = None
            null_label, guidance, rescale = 0, 0.0, 0.0
        if iv is None:
            mode, tables = self._mode(x_in, sched, hist, known, rescale, guidance, y, tables)
        else:
            tables = None
        t, y, vals, mask, noise = self._norm_inputs(x_in, t, y, vals, mask, noise)
        a = self._args(x_in, x_out, t, t_stride, y, null_label, vals, mask, guidance, tables, noise, seed,
                       sample_offset)
        with torch.cuda.device(x_in.device):
            if iv is not None:
                check(self.lib.dmx_step_invert(self.handle, ctypes.byref(a), ctypes.byref(iv),
                                               ctypes.c_void_p(_stream(x_in.device))))
            elif gg is not None:
                check(self.lib.dmx_step_geom(self.handle, ctypes.byref(a), *mode[:3], ctypes.byref(gg),
                                             ctypes.c_void_p(_stream(x_in.device))))
            elif pt is not None:
                check(self.lib.dmx_step_perturbed(self.handle, ctypes.byref(a), *mode, ctypes.byref(comp),
                                                  ctypes.byref(pt), ctypes.c_void_p(_stream(x_in.device))))
            elif compose is not None:
                check(self.lib.dmx_step_composed(self.handle, ctypes.byref(a), *mode, ctypes.byref(comp),
                                                 ctypes.c_void_p(_stream(x_in.device))))
            elif ch is not None:
                check(self.lib.dmx_step_cached(self.handle, ctypes.byref(a), *mode, ctypes.byref(ch),
                                               ctypes.c_void_p(_stream(x_in.device))))
            else:
                check(self.lib.dmx_step_guided(self.handle, ctypes.byref(a), *mode,
                                               ctypes.c_void_p(_stream(x_in.device))))

    def step_profile(self, x_in, x_out, t, y, null_label, vals, mask, guidance, tables, noise=None, seed=0,
                     t_stride=1, cap=1024):
        """One eager step with event timing per launch -> list of dicts."""
        self.ctx.ensure_time_table(int(tables[0].numel()))
        t, y, vals, mask, noise = self._norm_inputs(x_in, t, y, vals, mask, noise)
        a = self._args(x_in, x_out, t, t_stride, y, null_label, vals, mask, guidance, tables, noise, seed, 0)
        recs = (_lib.KernelRecord * cap)()
        n = ctypes.c_int()
        with torch.cuda.device(x_in.device):
            check(self.lib.dmx_step_profile(self.handle, ctypes.byref(a), recs, cap, ctypes.byref(n),
                                            ctypes.c_void_p(_stream(x_in.device))))
        return [dict(kernel=r.kernel.decode(), layer=r.layer.decode(), flops=r.flops, bytes=r.bytes, ms=r.ms)
                for r in recs[:n.value]]

    def side_stream(self) -> torch.cuda.Stream:
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(self.device)
        return self._side_stream

    def sample_loop(self, x, t_dev, y, null_label, vals, mask, guidance, tables, steps, seed=0, sample_offset=0,
                    use_graph=True, sched=None, hist=None, known=None, rescale=0.0, compose=None, geom=None,
                    perturb=None, invert=None, cache=None):
        """`steps` in-place steps on x with Philox noise; t_dev (device int64 scalar) is
        decremented on the device after each step.  Runs on a side stream (graph capture
        needs a non-default stream) ordered against the current stream.

        sched (the 6-tuple of Diffuser.ddim_tables): strided DDIM steps; t_dev then holds the
        position in [1, S] and `tables` is not read (may be None).
        sched a DpmSchedule (Diffuser.dpm_tables) with hist (x's shape, updated in place):
        DPM-Solver++(2M) steps, which draw nothing (`seed` is not read).
        known (z0, e0, mask, q_a, q_e) as in step(): every step is followed by the known-region blend.
        A loop entering below position S starts from known_blend's start latent.
        rescale = phi in (0, 1] as in step(): every step of the loop is a rescaled CFG step.
        The model keeps the captured graphs of the last few distinct loops (graph_captures counts the
        captures), so alternating guided, unguided and rescaled loops replay instead of recapturing.
        compose as in step(): every step of the loop is a composed step.  The captured graphs hold the
        pointers of the converted tables: pass contiguous int64 / fp32 device tensors to replay them.
        geom as in step(): every step of the loop is a geometry-guided step; the graphs hold the pointers
        of its two tables.
        perturb as in step(): every step of the loop is a perturbed composed step, with graphs of its own.
        invert = (tables, src) as in step(): `steps` rows of a DDIM inversion, t_dev counting the rows
        down from N; nothing is drawn (`seed` is not read) and the graphs hold the pointers of the four
        tables and of src.
        cache = (N, phase) as in step(): step k of the loop refreshes where (phase + k) % N == 0 and reuses
        the stored feature otherwise; the loop keeps one captured graph per step kind (graph_captures
        counts two) and replays them in the pattern."""
        _check_state(x, "x")
        ch = self._cache(cache, compose, geom, perturb, invert)
        iv = None
        if invert is not None:
            iv = self._invert(x, invert, sched, hist, known, rescale, compose, geom, perturb)
        pt = self._perturb(perturb, compose, geom) if perturb is not None else None
        gg = None
        if geom is not None:
            gg = self._geom(x, geom, sched, tables, rescale, compose, guidance, y, vals, mask)
            self._live_geom = tuple(geom)
        comp_live = ()
        if compose is not None:
            comp, comp_live = self._compose(x, compose, rescale)
            self._live_comp = comp_live
            y = vals = mask = None
            null_label, guidance, rescale = 0, 0.0, 0.0
        if iv is None:
            mode, tables = self._mode(x, sched, hist, known, rescale, guidance, y, tables)
        else:
            tables = invert[0]  # (kept alive below; the step args carry no tables)
        if t_dev.dtype != torch.long or not t_dev.is_contiguous() or t_dev.device != x.device:
            raise ValueError("sample_loop: t_dev must be a contiguous int64 device scalar on x's device "
                             "(it is decremented in place)")
        _, y, vals, mask, _ = self._norm_inputs(x, t_dev, y, vals, mask, None)
        a = self._args(x, x, t_dev, 0, y, null_label, vals, mask, guidance, None if iv is not None else tables, None,
                       seed, sample_offset)
        cur = torch.cuda.current_stream(x.device)
        side = self.side_stream()
        side.wait_stream(cur)
        live = (x, t_dev, y, vals, mask, hist if iv is None else invert[1])
        live += tuple(sched if sched is not None else tables) + tuple(known or ())
        live += tuple(comp_live) + (tuple(geom) if geom is not None else ())
        for keep in live:
            if keep is not None:
                keep.record_stream(side)
        with torch.cuda.device(x.device):
            if iv is not None:
                check(self.lib.dmx_sample_loop_invert(self.handle, ctypes.byref(a), ctypes.byref(iv), int(steps),
                                                      int(use_graph), ctypes.c_void_p(side.cuda_stream)))
            elif gg is not None:
                check(self.lib.dmx_sample_loop_geom(self.handle, ctypes.byref(a), *mode[:3], ctypes.byref(gg),
                                                    int(steps), int(use_graph), ctypes.c_void_p(side.cuda_stream)))
            elif pt is not None:
                check(self.lib.dmx_sample_loop_perturbed(self.handle, ctypes.byref(a), *mode, ctypes.byref(comp),
                                                         ctypes.byref(pt), int(steps), int(use_graph),
                                                         ctypes.c_void_p(side.cuda_stream)))
            elif compose is not None:
                check(self.lib.dmx_sample_loop_composed(self.handle, ctypes.byref(a), *mode, ctypes.byref(comp),
                                                        int(steps), int(use_graph),
                                                        ctypes.c_void_p(side.cuda_stream)))
            elif ch is not None:
                check(self.lib.dmx_sample_loop_cached(self.handle, ctypes.byref(a), *mode, ctypes.byref(ch),
                                                      int(steps), int(use_graph), ctypes.c_void_p(side.cuda_stream)))
            else:
                check(self.lib.dmx_sample_loop_guided(self.handle, ctypes.byref(a), *mode, int(steps),
                                                      int(use_graph), ctypes.c_void_p(side.cuda_stream)))
        cur.wait_stream(side)

    # ---- VAE -----------------------------------------------------------------------------
    def decode(self, z, want_img=True, want_u8=False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        n, c, h, w = z.shape
        z = z.contiguous().float()
        img = torch.empty((n, 3, 8 * h, 8 * w), device=z.device, dtype=torch.float32) if want_img else None
        u8 = torch.empty((n, 8 * h, 8 * w, 3), device=z.device, dtype=torch.uint8) if want_u8 else None
        with torch.cuda.device(z.device):
            check(self.lib.dmx_vae_decode(self.handle, _ptr(z), _ptr(img), _ptr(u8), n, h, w,
                                          ctypes.c_void_p(_stream(z.device))))
        return img, u8

    def decode_u8_into(self, z, u8) -> None:
        """Decode z (n,4,h,w) straight into a caller-owned uint8 (n,8h,8w,3) HWC buffer."""
        n, c, h, w = z.shape
        zc = z.contiguous().float()
        if u8.dtype != torch.uint8 or not u8.is_contiguous() or tuple(u8.shape) != (n, 8 * h, 8 * w, 3):
            raise ValueError(f"u8 must be a contiguous uint8 tensor of shape {(n, 8 * h, 8 * w, 3)}")
        with torch.cuda.device(zc.device):
            check(self.lib.dmx_vae_decode(self.handle, _ptr(zc), None, _ptr(u8), n, h, w,
                                          ctypes.c_void_p(_stream(zc.device))))
        self._live_dec = zc

    def encode(self, x, eps) -> Tuple[torch.Tensor, torch.Tensor]:
        """x (n,3,h,w), eps (n,4,h/8,w/8) -> (z, per-sample KL (n,)) (models/vae.py:51-62)."""
        n, c, h, w = x.shape
        x = x.contiguous().float()
        eps = eps.contiguous().float()
        z = torch.empty((n, 4, h // 8, w // 8), device=x.device, dtype=torch.float32)
        kl = torch.empty((n,), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            check(self.lib.dmx_vae_encode(self.handle, _ptr(x), _ptr(eps), _ptr(z), _ptr(kl), n, h, w,
                                          ctypes.c_void_p(_stream(x.device))))
        return z, kl

    # ---- VAE training (include/dmx.h dmx_vae_train_forward / dmx_vae_train_backward) ---------
    def vae_train_forward(self, x, eps):
        """VAE.forward's network part with a tape: x (n,3,h,w), eps (n,4,h/8,w/8) = the caller's randn
        draw -> (x_recon, z, per-sample KL (n,), tape id)."""
        require_cuda(x, "x")
        n, c, h, w = x.shape
        dev = x.device
        x = x.detach().to(dtype=torch.float32).contiguous()
        eps = eps.detach().to(device=dev, dtype=torch.float32).contiguous()
        if c != 3 or h % 8 or w % 8 or tuple(eps.shape) != (n, 4, h // 8, w // 8):
            raise ValueError(f"vae_train_forward: x must be (n,3,8a,8b) and eps (n,4,a,b); got {tuple(x.shape)}, "
                             f"{tuple(eps.shape)}")
        x_recon = torch.empty_like(x)
        z = torch.empty_like(eps)
        kl = torch.empty((n,), device=dev, dtype=torch.float32)
        tid = ctypes.c_int64()
        with torch.cuda.device(dev):
            check(self.lib.dmx_vae_train_forward(self.handle, _ptr(x), _ptr(eps), n, h, w, _ptr(x_recon), _ptr(z),
                                                 _ptr(kl), ctypes.byref(tid), ctypes.c_void_p(_stream(dev))))
        self._live_train = (x, eps)
        return x_recon, z, kl, int(tid.value)

    def vae_train_backward(self, tape_id: int, d_recon=None, d_z=None, d_kl=None) -> Dict[str, torch.Tensor]:
        """dLoss/dparam for every state_dict key, given the cotangents of x_recon, z and the per-sample
        KL (None = 0)."""
        dev = self.device
        grads = {name: torch.empty(shape, device=dev, dtype=torch.float32) for name, shape in self.keys}
        ptrs = (ctypes.c_void_p * len(self.keys))(*[grads[name].data_ptr() for name, _ in self.keys])
        cot = [None if d is None else d.to(device=dev, dtype=torch.float32).contiguous() for d in (d_recon, d_z, d_kl)]
        with torch.cuda.device(dev):
            check(self.lib.dmx_vae_train_backward(self.handle, int(tape_id), _ptr(cot[0]), _ptr(cot[1]), _ptr(cot[2]),
                                                  ptrs, len(self.keys), ctypes.c_void_p(_stream(dev))))
        self._live_bwd = tuple(cot)
        return grads


def _check_state(x: torch.Tensor, what: str) -> None:
    """The step kernels read / write x as contiguous fp32 NCHW on the device."""
    require_cuda(x, what)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor (got {x.dtype}, contiguous={x.is_contiguous()})")


def _guidance_struct(rescale, guidance, y) -> Optional[Guidance]:
    """The C view of a step's guidance controls: None for rescale 0 (nothing is asked of y or the scale)."""
    phi = float(rescale)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"rescale must be in [0, 1] (got {rescale})")
    if phi == 0.0:
        return None
    if y is None or not float(guidance) > 0:
        raise ValueError("rescale applies to CFG steps: it needs y and guidance > 0")
    return Guidance(phi)


def cfg_rescale(eu, ec, guidance, phi):
    """Standalone CFG mix + rescale (include/dmx.h dmx_cfg_rescale) for duck-typed models ->
    (eps, r): eg = eu + g (ec - eu); r[n] = 1 + phi (std(ec[n]) / std(eg[n]) - 1) over the sample's
    elements, moments in double, 1 where std(eg[n]) is not a positive finite number; eps = eg r[n].
    eu, ec: (n,c,h,w) on the GPU, any c, h, w >= 1; phi in [0, 1] (0: eps = eg, r = 1).
    Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    require_cuda(eu, "eps_uncond")
    phi = float(phi)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"phi must be in [0, 1] (got {phi})")
    dev = eu.device
    eu_c = eu.to(dtype=torch.float32).contiguous()
    ec_c = ec.to(device=dev, dtype=torch.float32).contiguous()
    if eu_c.dim() != 4 or tuple(ec_c.shape) != tuple(eu_c.shape) or min(eu_c.shape) < 1:
        raise ValueError(f"eps_uncond / eps_cond must be equal (n,c,h,w) tensors (got {tuple(eu.shape)}, "
                         f"{tuple(ec.shape)})")
    n, c, h, w = eu_c.shape
    eps = torch.empty_like(eu_c)
    r = torch.empty((n,), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.dmx_cfg_rescale(_ptr(eu_c), _ptr(ec_c), float(guidance), phi, _ptr(eps), _ptr(r), n, c, h, w,
                                  ctypes.c_void_p(_stream(dev))))
    return eps, r


def compose_eps(e_list, weights):
    """Standalone composed-guidance mix (include/dmx.h dmx_compose_eps) for duck-typed models -> eps:
    e_list = [e_0, e_1, .., e_K] (or one stacked (K+1,n,c,h,w) tensor), e_0 the base branch's prediction,
    each (n,c,h,w) on the GPU with any c, h, w >= 1; weights (K, n) or (K,) finite floats.
        d_k = e_k - e_0;  s = w_1 d_1;  s = s + w_k d_k (k = 2..K);  eps = e_0 + s
    one fp32 rounding per operation.  Operands stay bound to locals for the duration of the launch."""
    lib = _lib.load()
    e = e_list if isinstance(e_list, torch.Tensor) else torch.stack([t.to(dtype=torch.float32) for t in e_list])
    require_cuda(e, "e_list")
    dev = e.device
    e_c = e.to(dtype=torch.float32).contiguous()
    if e_c.dim() != 5 or not 2 <= e_c.shape[0] <= _lib.DMX_COMPOSE_MAX + 1 or min(e_c.shape) < 1:
        raise ValueError(f"e_list must hold 2 .. {_lib.DMX_COMPOSE_MAX + 1} equal (n,c,h,w) tensors "
                         f"(got {tuple(e_c.shape)})")
    K, n, c, h, w = e_c.shape[0] - 1, *e_c.shape[1:]
    w_c = torch.as_tensor(weights, dtype=torch.float32).to(device=dev)
    if w_c.dim() == 1:
        w_c = w_c[:, None].expand(-1, n)
    w_c = w_c.contiguous()
    if tuple(w_c.shape) != (K, n):
        raise ValueError(f"weights must be ({K}, {n}) or ({K},) (got {tuple(w_c.shape)})")
    eps = torch.empty((n, c, h, w), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(lib.dmx_compose_eps(_ptr(e_c), _ptr(w_c), K, n, c, h, w, _ptr(eps), ctypes.c_void_p(_stream(dev))))
    return eps


def attn_identity(qkv, C):
    """The identity attention core alone (include/dmx.h dmx_attn_identity): qkv (n, L, 3C) = q | k | v on
    the GPU -> (n, L, C) = v, an exact fp32 copy — what a perturbed block's core yields.  C in {64, 128, 256}."""
    lib = _lib.load()
    require_cuda(qkv, "qkv")
    C = int(C)
    q_c = qkv.to(dtype=torch.float32).contiguous()
    if C not in (64, 128, 256) or q_c.dim() != 3 or q_c.shape[2] != 3 * C or min(q_c.shape) < 1:
        raise ValueError(f"qkv must be (n, L, 3C) with C in (64, 128, 256) (got {tuple(qkv.shape)}, C={C})")
    n, L, _ = q_c.shape
    out = torch.empty((n, L, C), device=q_c.device, dtype=torch.float32)
    with torch.cuda.device(q_c.device):
        check(lib.dmx_attn_identity(_ptr(q_c), _ptr(out), n, L, C, ctypes.c_void_p(_stream(q_c.device))))
    return out


def geom_mix(eps, grad, scale, sig, pos):
    """Standalone geometry-guidance mix (include/dmx.h dmx_geom_mix) for duck-typed models -> eps':
        eps' = eps + (scale[n] sig[pos[n] - 1]) grad
    one fp32 rounding per operation; where scale[n] == 0 or grad == 0 the element keeps eps's bits.
    eps, grad: (n,c,h,w) on the GPU, any c, h, w >= 1; scale: a float or (n,) floats; sig: (S,) fp32
    (sqrt(1 - ab) per position); pos: (n,) positions in [1, S] or one value for every sample.
    Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    require_cuda(eps, "eps")
    dev = eps.device
    e_c = eps.to(dtype=torch.float32).contiguous()
    g_c = grad.to(device=dev, dtype=torch.float32).contiguous()
    if e_c.dim() != 4 or tuple(g_c.shape) != tuple(e_c.shape) or min(e_c.shape) < 1:
        raise ValueError(f"eps / grad must be equal (n,c,h,w) tensors (got {tuple(eps.shape)}, {tuple(grad.shape)})")
    n, c, h, w = e_c.shape
    s_c = torch.as_tensor(scale, dtype=torch.float32).to(device=dev).reshape(-1)
    if s_c.numel() == 1:
        s_c = s_c.expand(n)
    s_c = s_c.contiguous()
    if s_c.numel() != n:
        raise ValueError(f"scale has {s_c.numel()} entries for a batch of {n}")
    sig_c = sig.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    if sig_c.numel() < 1:
        raise ValueError("sig is empty")
    p_c = torch.as_tensor(pos).to(device=dev, dtype=torch.long).contiguous().reshape(-1)
    if p_c.numel() not in (1, n):
        raise ValueError(f"pos has {p_c.numel()} entries for a batch of {n}")
    out = torch.empty_like(e_c)
    with torch.cuda.device(dev):
        check(lib.dmx_geom_mix(_ptr(e_c), _ptr(g_c), _ptr(s_c), _ptr(sig_c), int(sig_c.numel()), _ptr(p_c),
                               0 if p_c.numel() == 1 and n > 1 else 1, _ptr(out), n, c, h, w,
                               ctypes.c_void_p(_stream(dev))))
    return out


def pred_to_eps(out, x, t, p_o, p_x, inplace=False):
    """A foreign v-model's (mixed) output as eps (include/dmx.h dmx_pred_to_eps) -> eps:
        eps = p_o[t - 1] out + p_x[t - 1] x        (torch's bits: two products and a sum, no FMA)
    out, x: (n,c,h,w) on the GPU, any c, h, w >= 1, x the latent the model was evaluated at; t: (n,) network
    timesteps (any stride) or one value for every sample, clamped to [1, T] for the table reads; p_o, p_x:
    (T,) fp32 tables sqrt(ab), sqrt(1 - ab) (Diffuser.noise_tables).  inplace: the result is written over
    `out` (a contiguous fp32 tensor, e.g. a network's fresh output) and `out` is returned, else a new tensor.
    Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    require_cuda(out, "out")
    dev = out.device
    o_c = out.detach().to(dtype=torch.float32).contiguous()
    x_c = x.detach().to(device=dev, dtype=torch.float32).contiguous()
    if o_c.dim() != 4 or tuple(x_c.shape) != tuple(o_c.shape) or min(o_c.shape) < 1:
        raise ValueError(f"out / x must be equal non-empty (n,c,h,w) tensors (got {tuple(out.shape)}, {tuple(x.shape)})")
    n, c, h, w = o_c.shape
    po_c = p_o.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    px_c = p_x.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    T = int(po_c.numel())
    if T < 1 or px_c.numel() != T:
        raise ValueError(f"p_o and p_x must be equal non-empty tables (got {po_c.numel()}, {px_c.numel()})")
    t_c = torch.as_tensor(t).to(device=dev, dtype=torch.long).reshape(-1)
    if t_c.numel() not in (1, n):
        raise ValueError(f"t has {t_c.numel()} entries for a batch of {n}")
    stride = 0 if t_c.numel() == 1 else int(t_c.stride(0))
    if stride < 1 and t_c.numel() > 1:
        t_c, stride = t_c.contiguous(), 1
    if inplace and (o_c.data_ptr() != out.data_ptr() or out.requires_grad or o_c.data_ptr() == x_c.data_ptr()):
        raise ValueError("inplace needs `out` to be a contiguous fp32 tensor without grad, and not x itself")
    eps = out if inplace else torch.empty_like(o_c)
    with torch.cuda.device(dev):
        check(lib.dmx_pred_to_eps(_ptr(o_c), _ptr(x_c), _ptr(t_c), stride, _ptr(po_c), _ptr(px_c), T, n, c, h, w,
                                  _ptr(eps), ctypes.c_void_p(_stream(dev))))
    return eps


def pred_split(out, x, t, p_o, p_x, inplace=False):
    """A v-model's (mixed) output as (x0, eps), the x0-form's conversion (include/dmx.h dmx_pred_split):
        x0 = p_o[t - 1] x - p_x[t - 1] out;  eps = p_o[t - 1] out + p_x[t - 1] x
    (torch's bits: two products and a sum or difference each, no FMA) in one pass.  Operands as in pred_to_eps;
    inplace: eps is written over `out`, which is returned in its place; x0 is always a new tensor."""
    lib = _lib.load()
    require_cuda(out, "out")
    dev = out.device
    o_c = out.detach().to(dtype=torch.float32).contiguous()
    x_c = x.detach().to(device=dev, dtype=torch.float32).contiguous()
    if o_c.dim() != 4 or tuple(x_c.shape) != tuple(o_c.shape) or min(o_c.shape) < 1:
        raise ValueError(f"out / x must be equal non-empty (n,c,h,w) tensors (got {tuple(out.shape)}, {tuple(x.shape)})")
    n, c, h, w = o_c.shape
    po_c = p_o.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    px_c = p_x.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    T = int(po_c.numel())
    if T < 1 or px_c.numel() != T:
        raise ValueError(f"p_o and p_x must be equal non-empty tables (got {po_c.numel()}, {px_c.numel()})")
    t_c = torch.as_tensor(t).to(device=dev, dtype=torch.long).reshape(-1)
    if t_c.numel() not in (1, n):
        raise ValueError(f"t has {t_c.numel()} entries for a batch of {n}")
    stride = 0 if t_c.numel() == 1 else int(t_c.stride(0))
    if stride < 1 and t_c.numel() > 1:
        t_c, stride = t_c.contiguous(), 1
    if inplace and (o_c.data_ptr() != out.data_ptr() or out.requires_grad or o_c.data_ptr() == x_c.data_ptr()):
        raise ValueError("inplace needs `out` to be a contiguous fp32 tensor without grad, and not x itself")
    eps = out if inplace else torch.empty_like(o_c)
    x0 = torch.empty_like(o_c)
    with torch.cuda.device(dev):
        check(lib.dmx_pred_split(_ptr(o_c), _ptr(x_c), _ptr(t_c), stride, _ptr(po_c), _ptr(px_c), T, n, c, h, w,
                                 _ptr(x0), _ptr(eps), ctypes.c_void_p(_stream(dev))))
    return x0, eps


def train_noise(z, sa, s1, t=None, noise=None, drop=None, y=None, null_label=0, vals=None, mask=None,
                cfg_drop_prob=0.0, seed=0, sample_offset=0, target=None):
    """The front half of a training iteration (include/dmx.h dmx_train_noise; train_latent_cond.py:136-145) ->
    (z_noisy, noise, t, drop, y_used, vals_used, mask_used):
        z_noisy = sa[t - 1] z + s1[t - 1] noise     (torch's bits: two products and a sum, no FMA)
        y_used = where(drop, null_label, y);  vals_used / mask_used = the rows of vals / mask, zero where drop
    z: (B,C,h,w) on the GPU, any C, h, w >= 1; sa, s1: (T,) fp32 tables sqrt(ab), sqrt(1 - ab).  t (B,) in
    [1, T], noise (z's shape) and drop (B,) bool are used as given; each one left None is drawn on the
    device by Philox under `seed` from the rows' global indices sample_offset + n (t uniform on [1, T],
    drop = u < cfg_drop_prob, noise standard normal), so a shard of a batch draws the batch's rows.
    y, vals / mask may be None (their outputs are then None).  No host synchronisation.
    target = True, or a contiguous fp32 tensor of z's shape on z's device to write into (include/dmx.h
    dmx_train_noise_target): the same launch also stores the v-prediction target
        target = sa[t - 1] noise - s1[t - 1] z      (torch's bits: two products and a difference, no FMA)
    and the result gains it as an eighth entry; the other seven keep the bits of the call without it.
    Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    require_cuda(z, "z")
    dev = z.device
    z_c = z.detach().to(dtype=torch.float32).contiguous()
    if z_c.dim() != 4 or min(z_c.shape) < 1:
        raise ValueError(f"z must be a non-empty (B,C,h,w) tensor (got {tuple(z.shape)})")
    B, C, h, w = z_c.shape
    sa_c = sa.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    s1_c = s1.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    T = int(sa_c.numel())
    if T < 1 or s1_c.numel() != T:
        raise ValueError(f"sa and s1 must be equal non-empty tables (got {sa_c.numel()}, {s1_c.numel()})")
    p = float(cfg_drop_prob)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"cfg_drop_prob must be in [0, 1] (got {cfg_drop_prob})")
    draw = 0
    if t is None:
        draw |= 1
        t_c = torch.empty((B,), device=dev, dtype=torch.long)
    else:
        t_c = t.to(device=dev, dtype=torch.long).contiguous().reshape(-1)
    if noise is None:
        draw |= 2
        nz_c = torch.empty_like(z_c)
    else:
        nz_c = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
    if drop is None:
        draw |= 4
        d_c = torch.empty((B,), device=dev, dtype=torch.bool)
    else:
        d_c = drop.to(device=dev, dtype=torch.bool).contiguous().reshape(-1)
    if t_c.numel() != B or d_c.numel() != B or tuple(nz_c.shape) != tuple(z_c.shape):
        raise ValueError(f"t / drop need {B} entries and noise z's shape (got {t_c.numel()}, {d_c.numel()}, "
                         f"{tuple(nz_c.shape)})")
    if (vals is None) != (mask is None):
        raise ValueError("vals and mask go together")
    y_c = y_u = v_c = m_c = v_u = m_u = None
    gd = 0
    if y is not None:
        y_c = y.to(device=dev, dtype=torch.long).contiguous().reshape(-1)
        if y_c.numel() != B:
            raise ValueError(f"y has {y_c.numel()} entries for a batch of {B}")
        y_u = torch.empty_like(y_c)
    if vals is not None:
        v_c = vals.detach().to(device=dev, dtype=torch.float32).contiguous()
        m_c = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
        if v_c.dim() != 2 or v_c.shape[0] != B or v_c.shape[1] < 1 or tuple(m_c.shape) != tuple(v_c.shape):
            raise ValueError(f"vals / mask must be equal ({B}, gd) tensors (got {tuple(vals.shape)}, "
                             f"{tuple(mask.shape)})")
        gd = int(v_c.shape[1])
        v_u, m_u = torch.empty_like(v_c), torch.empty_like(m_c)
    out = torch.empty_like(z_c)
    tg = None
    if target is True:
        tg = torch.empty_like(z_c)
    elif target is not None and target is not False:
        tg = target
        if (not isinstance(tg, torch.Tensor) or tg.dtype != torch.float32 or tg.device != dev
                or tuple(tg.shape) != tuple(z_c.shape) or not tg.is_contiguous()):
            raise ValueError(f"target must be True or a contiguous fp32 {tuple(z_c.shape)} tensor on {dev}")
    a = _lib.NoiseArgs(z=_ptr(z_c), sa=_ptr(sa_c), s1=_ptr(s1_c), T=T, draw=draw, t=_ptr(t_c), noise=_ptr(nz_c),
                       drop=_ptr(d_c), seed=int(seed) & (2 ** 64 - 1), sample_offset=int(sample_offset),
                       cfg_drop_prob=p, gd=gd, y=_ptr(y_c), null_label=int(null_label), vals=_ptr(v_c),
                       mask=_ptr(m_c), z_noisy=_ptr(out), y_used=_ptr(y_u), vals_used=_ptr(v_u),
                       mask_used=_ptr(m_u), B=B, C=C, h=h, w=w)
    with torch.cuda.device(dev):
        if tg is not None:
            check(lib.dmx_train_noise_target(ctypes.byref(a), _ptr(tg), ctypes.c_void_p(_stream(dev))))
            return out, nz_c, t_c, d_c, y_u, v_u, m_u, tg
        check(lib.dmx_train_noise(ctypes.byref(a), ctypes.c_void_p(_stream(dev))))
    return out, nz_c, t_c, d_c, y_u, v_u, m_u


class Objective:
    """What objective_loss computed and what objective_seed reads again: loss, noise_loss, geom_loss
    (0-dim views of one device buffer), per_sample (B,), and the operands, kept alive."""

    def __init__(self, args, keep, out, per_sample, has_geom):
        self._args, self._keep, self._out, self.has_geom = args, keep, out, has_geom
        self.loss, self.noise_loss, self.geom_loss = out[0], out[1], out[2]
        self.per_sample = per_sample


def objective_loss(eps, noise, t=None, weight=None, geom=None, vals=None, mask=None, geom_lambda=0.0, denom=None):
    """The training loss (include/dmx.h dmx_objective_loss; train_latent_cond.py:151-159) -> Objective:
        per_sample[n] = weight[t_n - 1] mean_chw (eps - noise)^2;  noise_loss = mean_n per_sample[n]
        geom_loss = sum mask (geom - vals)^2 / max(denom, 1e-6), denom = sum mask unless given
        loss = noise_loss + geom_lambda geom_loss
    fp32 differences and squares, double sums in a fixed order: the same bits from run to run.  eps, noise:
    (B,C,h,w) on the GPU; weight: (T,) fp32 with t (B,) in [1, T], or None for 1; geom, vals, mask: (B,gd)
    or None (no geometry term); denom: a 0-dim tensor or a float.  No host synchronisation."""
    lib = _lib.load()
    require_cuda(eps, "eps")
    dev = eps.device
    e_c = eps.detach().to(dtype=torch.float32).contiguous()
    n_c = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
    if e_c.dim() != 4 or min(e_c.shape) < 1 or tuple(n_c.shape) != tuple(e_c.shape):
        raise ValueError(f"eps / noise must be equal non-empty (B,C,h,w) tensors (got {tuple(eps.shape)}, "
                         f"{tuple(noise.shape)})")
    B, C, h, w = e_c.shape
    lam = float(geom_lambda)
    if not (lam >= 0.0 and lam < float("inf")):
        raise ValueError(f"geom_lambda must be finite and >= 0 (got {geom_lambda})")
    t_c = w_c = g_c = v_c = m_c = d_c = None
    T = gd = 0
    if weight is not None:
        if t is None:
            raise ValueError("a weight table needs t")
        w_c = weight.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
        t_c = t.to(device=dev, dtype=torch.long).contiguous().reshape(-1)
        T = int(w_c.numel())
        if T < 1 or t_c.numel() != B:
            raise ValueError(f"weight must be a non-empty table and t have {B} entries (got {T}, {t_c.numel()})")
    if geom is not None:
        if vals is None or mask is None:
            raise ValueError("the geometry term needs vals and mask")
        g_c = geom.detach().to(device=dev, dtype=torch.float32).contiguous()
        v_c = vals.detach().to(device=dev, dtype=torch.float32).contiguous()
        m_c = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
        if g_c.dim() != 2 or g_c.shape[0] != B or g_c.shape[1] < 1 or tuple(v_c.shape) != tuple(g_c.shape) or \
                tuple(m_c.shape) != tuple(g_c.shape):
            raise ValueError(f"geom / vals / mask must be equal ({B}, gd) tensors (got {tuple(geom.shape)}, "
                             f"{tuple(vals.shape)}, {tuple(mask.shape)})")
        gd = int(g_c.shape[1])
        if denom is not None:
            d_c = torch.as_tensor(denom, dtype=torch.float32).to(device=dev).reshape(-1).contiguous()
            if d_c.numel() != 1:
                raise ValueError("denom must be one number")
    part = torch.empty((3 * B,), device=dev, dtype=torch.float64)
    per_sample = torch.empty((B,), device=dev, dtype=torch.float32)
    out = torch.empty((4,), device=dev, dtype=torch.float32)
    a = _lib.ObjectiveArgs(eps=_ptr(e_c), noise=_ptr(n_c), t=_ptr(t_c), weight=_ptr(w_c), T=T, geom=_ptr(g_c),
                           vals=_ptr(v_c), mask=_ptr(m_c), gd=gd, denom=_ptr(d_c), geom_lambda=lam, part=_ptr(part),
                           per_sample=_ptr(per_sample), out=_ptr(out), B=B, C=C, h=h, w=w)
    with torch.cuda.device(dev):
        check(lib.dmx_objective_loss(ctypes.byref(a), ctypes.c_void_p(_stream(dev))))
    return Objective(a, (e_c, n_c, t_c, w_c, g_c, v_c, m_c, d_c, part), out, per_sample, g_c is not None)


def objective_seed(obj, up=None, want_geom=True):
    """The gradient of an Objective's loss (include/dmx.h dmx_objective_seed) -> (d_eps, d_geom or None):
        d_eps = up 2 w_n (eps - noise) / (B C h w);  d_geom = up geom_lambda 2 mask (geom - vals) / max(denom, 1e-6)
    what NativeModel.train_backward takes.  up: the upstream gradient as a one-element fp32 tensor on the
    GPU, read by the kernel (None: 1); no host synchronisation."""
    lib = _lib.load()
    e_c, g_c = obj._keep[0], obj._keep[4]
    dev = e_c.device
    if up is None:
        up_c = torch.ones((1,), device=dev, dtype=torch.float32)
    else:
        up_c = up.detach().to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
        if up_c.numel() != 1:
            raise ValueError(f"up must hold one number (got {up_c.numel()})")
    d_eps = torch.empty_like(e_c)
    d_geom = torch.empty_like(g_c) if (want_geom and g_c is not None) else None
    with torch.cuda.device(dev):
        check(lib.dmx_objective_seed(ctypes.byref(obj._args), _ptr(up_c), _ptr(d_eps), _ptr(d_geom),
                                     ctypes.c_void_p(_stream(dev))))
    obj._live_seed = (up_c, d_eps, d_geom)
    return d_eps, d_geom


def _update_operands(x, eu, ec, noise, pos, pos_name):
    """The operands the standalone updates share, as contiguous fp32 / int64 tensors on x's device and
    of x's shape (pos: one entry per sample) -> (x, eu, ec or None, noise or None, pos)."""
    require_cuda(x, "x")
    dev = x.device
    x_c = x.to(dtype=torch.float32).contiguous()
    eu_c = eu.to(device=dev, dtype=torch.float32).contiguous()
    ec_c = ec.to(device=dev, dtype=torch.float32).contiguous() if ec is not None else None
    nz_c = noise.to(device=dev, dtype=torch.float32).contiguous() if noise is not None else None
    p_c = pos.to(device=dev, dtype=torch.long).contiguous()
    for e, nm in ((eu_c, "eps"), (ec_c, "eps_cond"), (nz_c, "noise")):
        if e is not None and tuple(e.shape) != tuple(x_c.shape):
            raise ValueError(f"{nm} shape {tuple(e.shape)} != x shape {tuple(x_c.shape)}")
    if p_c.numel() != x_c.shape[0]:
        raise ValueError(f"{pos_name} has {p_c.numel()} entries for a batch of {x_c.shape[0]}")
    return x_c, eu_c, ec_c, nz_c, p_c


def ddpm_update(x, eu, ec, guidance, t, tables, noise=None, seed=0, sample_offset=0):
    """Standalone K1 (diff.py:151,158-162) for duck-typed models: returns x'.

    Every converted operand is bound to a local for the duration of the launch (a temporary
    freed right after taking its pointer could be handed to the next conversion by the
    caching allocator)."""
    lib = _lib.load()
    c1, c2, sd = tables
    x_c, eu_c, ec_c, nz_c, t_c = _update_operands(x, eu, ec, noise, t, "t")
    n, c, h, w = x_c.shape
    out = torch.empty_like(x_c)
    with torch.cuda.device(x.device):
        check(lib.dmx_ddpm_update(_ptr(x_c), _ptr(out), _ptr(eu_c), _ptr(ec_c), float(guidance), _ptr(t_c),
                                  1, _ptr(c1), _ptr(c2), _ptr(sd), int(c1.numel()), _ptr(nz_c), int(seed),
                                  int(sample_offset), n, c, h, w, ctypes.c_void_p(_stream(x.device))))
    return out


def _sched_struct(sched, device) -> DdimSched:
    """The C view of a (t_map, k_e, k_a, k_s, k_d, k_n) schedule: int64 / fp32 contiguous tensors of one
    length S on `device` (Diffuser.ddim_tables builds them so; nothing is converted here, the kernels
    read the caller's tensors)."""
    if len(sched) != 6:
        raise ValueError("sched must be the 6-tuple (t_map, k_e, k_a, k_s, k_d, k_n) of Diffuser.ddim_tables")
    S = int(sched[0].numel())
    for i, v in enumerate(sched):
        want = torch.long if i == 0 else torch.float32
        if v.dtype != want or v.dim() != 1 or v.numel() != S or not v.is_contiguous() or v.device != device:
            raise ValueError(f"sched[{i}] must be a contiguous 1-D {want} tensor of {S} entries on {device}")
    if S < 1:
        raise ValueError("sched is empty")
    return DdimSched(*[v.data_ptr() for v in sched], S)


def ddim_update(x, eu, ec, guidance, pos, sched, noise=None, seed=0, sample_offset=0):
    """Standalone strided DDIM update (include/dmx.h dmx_ddim_update) for duck-typed models: returns x'.
    pos: (n,) positions in [1, S]; sched: the 6-tuple of Diffuser.ddim_tables on x's device.
    Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    require_cuda(x, "x")
    sc = _sched_struct(sched, x.device)
    x_c, eu_c, ec_c, nz_c, p_c = _update_operands(x, eu, ec, noise, pos, "pos")
    n, c, h, w = x_c.shape
    out = torch.empty_like(x_c)
    with torch.cuda.device(x.device):
        check(lib.dmx_ddim_update(_ptr(x_c), _ptr(out), _ptr(eu_c), _ptr(ec_c), float(guidance), _ptr(p_c), 1,
                                  ctypes.byref(sc), _ptr(nz_c), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  int(sample_offset), n, c, h, w, ctypes.c_void_p(_stream(x.device))))
    return out


class DpmSchedule(tuple):
    """The (t_map, k_e, k_a, k_x, k_c, k_p) tables of a DPM-Solver++(2M) schedule (Diffuser.dpm_tables).
    The type is what tells it from a DDIM schedule, which stays a plain 6-tuple."""
    __slots__ = ()


def _dpm_struct(sched, device, hist, x) -> DpmSched:
    """The C view of a DpmSchedule and its history buffer: tables as in _sched_struct, hist a
    contiguous fp32 tensor of x's shape on `device` that does not share x's storage."""
    if not isinstance(sched, DpmSchedule) or len(sched) != 6:
        raise ValueError("sched must be the DpmSchedule (t_map, k_e, k_a, k_x, k_c, k_p) of Diffuser.dpm_tables")
    S = int(sched[0].numel())
    for i, v in enumerate(sched):
        want = torch.long if i == 0 else torch.float32
        if v.dtype != want or v.dim() != 1 or v.numel() != S or not v.is_contiguous() or v.device != device:
            raise ValueError(f"sched[{i}] must be a contiguous 1-D {want} tensor of {S} entries on {device}")
    if S < 1:
        raise ValueError("sched is empty")
    if hist is None:
        raise ValueError("a DPM schedule needs hist (the history buffer, x's shape)")
    if (hist.dtype != torch.float32 or not hist.is_contiguous() or hist.device != device
            or tuple(hist.shape) != tuple(x.shape)):
        raise ValueError(f"hist must be a contiguous fp32 tensor of shape {tuple(x.shape)} on {device}")
    if hist.data_ptr() == x.data_ptr():
        raise ValueError("hist must not alias x")
    return DpmSched(*[v.data_ptr() for v in sched], hist.data_ptr(), S)


def dpm_update(x, eu, ec, guidance, pos, sched, hist, out=None):
    """Standalone DPM-Solver++(2M) update (include/dmx.h dmx_dpm_update) for duck-typed models: returns
    x' and updates hist in place.  pos: (n,) positions in [1, S]; sched: the DpmSchedule of
    Diffuser.dpm_tables on x's device; hist: fp32, x's shape, read where k_p != 0 and always written.
    out: where x' goes (fp32, contiguous, x's shape; may be x itself), a new tensor by default.
    Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    x_c, eu_c, ec_c, _, p_c = _update_operands(x, eu, ec, None, pos, "pos")
    dev = x.device
    sc = _dpm_struct(sched, dev, hist, x_c)
    n, c, h, w = x_c.shape
    if out is None:
        out = torch.empty_like(x_c)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev
          or tuple(out.shape) != tuple(x_c.shape) or out.data_ptr() == hist.data_ptr()):
        raise ValueError(f"out must be a contiguous fp32 tensor of shape {tuple(x_c.shape)} on {dev}, not hist")
    with torch.cuda.device(dev):
        check(lib.dmx_dpm_update(_ptr(x_c), _ptr(out), _ptr(eu_c), _ptr(ec_c), float(guidance), _ptr(p_c), 1,
                                 ctypes.byref(sc), n, c, h, w, ctypes.c_void_p(_stream(dev))))
    return out


def _invert_struct(tables, device, src, x) -> InvertSched:
    """The C view of the (t_eval, i_x, i_e, adv) tables of Diffuser.invert_tables and the source buffer:
    int64 / fp32 / fp32 / int32 contiguous 1-D tensors of one length N on `device`, src a contiguous fp32
    tensor of x's shape on `device` that does not share x's storage.  Nothing is converted: the kernels
    read the caller's tensors."""
    if not isinstance(tables, (tuple, list)) or len(tables) != 4:
        raise ValueError("invert tables must be the 4-tuple (t_eval, i_x, i_e, adv) of Diffuser.invert_tables")
    N = int(tables[0].numel())
    for i, (v, want) in enumerate(zip(tables, (torch.long, torch.float32, torch.float32, torch.int32))):
        if v.dtype != want or v.dim() != 1 or v.numel() != N or not v.is_contiguous() or v.device != device:
            raise ValueError(f"invert tables[{i}] must be a contiguous 1-D {want} tensor of {N} entries on {device}")
    if N < 1:
        raise ValueError("invert tables are empty")
    if (not isinstance(src, torch.Tensor) or src.dtype != torch.float32 or not src.is_contiguous()
            or src.device != device or tuple(src.shape) != tuple(x.shape)):
        raise ValueError(f"src must be a contiguous fp32 tensor of shape {tuple(x.shape)} on {device}")
    if src.data_ptr() == x.data_ptr():
        raise ValueError("src must not alias x")
    return InvertSched(*[v.data_ptr() for v in tables], src.data_ptr(), N)


def invert_update(x, eu, ec, guidance, pos, tables, src, out=None):
    """Standalone DDIM-inversion update (include/dmx.h dmx_invert_update) for duck-typed models: returns
    y = i_x src + i_e eps and stores it in src where the row's adv is set.  x: the latent the prediction
    was made on (it gives the shape, any C >= 1; its values are not read); pos: (n,) countdown positions in
    [1, N]; tables: Diffuser.invert_tables on x's device; src: fp32, contiguous, x's shape.
    out: where y goes (fp32, contiguous, x's shape; may be x itself, never src), a new tensor by default.
    Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    x_c, eu_c, ec_c, _, p_c = _update_operands(x, eu, ec, None, pos, "pos")
    dev = x.device
    if out is None:
        out = torch.empty_like(x_c)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev
          or tuple(out.shape) != tuple(x_c.shape)):
        raise ValueError(f"out must be a contiguous fp32 tensor of shape {tuple(x_c.shape)} on {dev}")
    iv = _invert_struct(tables, dev, src, out)  # (src must not be where y goes)
    n, c, h, w = x_c.shape
    with torch.cuda.device(dev):
        check(lib.dmx_invert_update(_ptr(src), _ptr(out), _ptr(eu_c), _ptr(ec_c), float(guidance), _ptr(p_c), 1,
                                    ctypes.byref(iv), n, c, h, w, ctypes.c_void_p(_stream(dev))))
    return out


def _known_struct(known, device, x, need_mask=False) -> KnownSched:
    """The C view of a known region (z0, e0, mask, q_a, q_e): z0 / e0 contiguous fp32 of x's shape, mask
    contiguous fp32 (n,1,h,w) or (n,h,w) (None where the caller allows: every element kept), q_a / q_e the
    1-D fp32 tables of Diffuser.known_tables, all on `device`.  Nothing is converted: the kernels read the
    caller's tensors.  Aliasing of x and S against the schedule are checked by the library."""
    if not isinstance(known, (tuple, list)) or len(known) != 5:
        raise ValueError("known must be the 5-tuple (z0, e0, mask, q_a, q_e)")
    z0, e0, mask, q_a, q_e = known
    n, _, h, w = x.shape
    for v, nm in ((z0, "z0"), (e0, "e0")):
        if (v.dtype != torch.float32 or not v.is_contiguous() or v.device != device
                or tuple(v.shape) != tuple(x.shape)):
            raise ValueError(f"known {nm} must be a contiguous fp32 tensor of shape {tuple(x.shape)} on {device}")
    if mask is None:
        if need_mask:
            raise ValueError("known mask is required here (None only in known_blend: every element kept)")
    elif (mask.dtype != torch.float32 or not mask.is_contiguous() or mask.device != device
          or tuple(mask.shape) not in ((n, 1, h, w), (n, h, w))):
        raise ValueError(f"known mask must be a contiguous fp32 tensor of shape {(n, 1, h, w)} on {device}")
    S = int(q_a.numel())
    for v, nm in ((q_a, "q_a"), (q_e, "q_e")):
        if v.dtype != torch.float32 or v.dim() != 1 or v.numel() != S or not v.is_contiguous() or v.device != device:
            raise ValueError(f"known {nm} must be a contiguous 1-D fp32 tensor of {S} entries on {device}")
    if S < 1:
        raise ValueError("known tables are empty")
    return KnownSched(z0.data_ptr(), e0.data_ptr(), mask.data_ptr() if mask is not None else None,
                      q_a.data_ptr(), q_e.data_ptr(), S)


def known_blend(x, pos, known, out=None):
    """The known-region blend alone (include/dmx.h dmx_known_blend), for duck-typed models and start
    latents: returns x' = m == 0 ? kn : m == 1 ? x : m x + (1 - m) kn with kn = q_a[p-1] z0 + q_e[p-1] e0.
    x: (n,C,h,w) on the GPU; pos: (n,) positions or one value for every sample, clamped to [1, S];
    known: (z0, e0, mask, q_a, q_e) on x's device.  mask None: every element is kept, x' = kn, and x gives
    only the shape (its values are not read; it may be z0 itself).
    out: where x' goes (fp32, contiguous, x's shape; may be x itself, never z0 / e0 / mask), a new tensor
    by default.  Operands stay bound to locals for the duration of the launch, as in ddpm_update."""
    lib = _lib.load()
    require_cuda(x, "x")
    dev = x.device
    x_c = x.to(dtype=torch.float32).contiguous()
    kn = _known_struct(known, dev, x_c)
    n, c, h, w = x_c.shape
    p_c = pos.to(device=dev, dtype=torch.long).contiguous()
    if p_c.numel() not in (1, n):
        raise ValueError(f"pos has {p_c.numel()} entries for a batch of {n}")
    if out is None:
        out = torch.empty_like(x_c)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev
          or tuple(out.shape) != tuple(x_c.shape)):
        raise ValueError(f"out must be a contiguous fp32 tensor of shape {tuple(x_c.shape)} on {dev}")
    with torch.cuda.device(dev):
        check(lib.dmx_known_blend(_ptr(x_c) if known[2] is not None else None, _ptr(out), _ptr(p_c),
                                  0 if p_c.numel() == 1 and n > 1 else 1, ctypes.byref(kn), n, c, h, w,
                                  ctypes.c_void_p(_stream(dev))))
    return out
