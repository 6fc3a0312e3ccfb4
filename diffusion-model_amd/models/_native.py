"""Shared base of the drop-in networks: the reference's module tree (models/_modules.py)
backed by a repacked native copy inside libdmx.

The parameter layout (names, shapes, registration order, default initialisation) is
the reference's, so ``load_state_dict`` of a reference checkpoint works unchanged
(reference ``utils.py:68-73``).  ``forward`` never computes on the host: the first
call on a device packs the weights into libdmx (cached until a parameter is moved or
replaced; modified in place — optimizer.step, load_state_dict — it is repacked on the
device by ``NativeModel.refresh``) and every call after that is a native launch.

With autograd recording (grad mode on, trainable parameters) the U-Nets run the native
training forward and backward (``_NativeTrainFn``, include/dmx.h dmx_train_forward /
dmx_train_backward): ``loss.backward()`` of the reference training loop
(train_latent_cond.py:148-162) fills every parameter's ``.grad``.  The VAE does the same through
``_NativeVaeTrainFn`` (dmx_vae_train_forward / dmx_vae_train_backward) for train_vae.py's step.
"""
from __future__ import annotations

import os
import sys

import torch
from torch import nn

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from dmx import engine as _engine  # noqa: E402


class NativeBacked(nn.Module):
    """nn.Module whose compute lives in libdmx."""

    _dmx_kind = 0

    def __init__(self):
        super().__init__()
        object.__setattr__(self, "_dmx_cache", None)

    def _dmx_key(self):
        ps = [p for _, p in self.named_parameters()]
        return (ps[0].device, tuple(p.data_ptr() for p in ps), tuple(sorted(self._dmx_config().items())))

    def native(self) -> "_engine.NativeModel":
        key = self._dmx_key()
        versions = tuple(p._version for p in self.parameters())
        cache = self._dmx_cache
        if cache is not None and cache[0] == key:
            nm = cache[1]
            if cache[2] != versions:
                if not nm.aliases_params:  # converted copies were registered: rebuild
                    cache = None
                else:  # same storage, new values: repack in place on the device
                    nm.refresh()
                    object.__setattr__(self, "_dmx_cache", (key, nm, versions))
            if cache is not None:
                return nm
        self._dmx_check_supported()
        params = {k: v.detach() for k, v in self.named_parameters()}
        nm = _engine.NativeModel(self._dmx_kind, params, in_ch=getattr(self, "_dmx_in_ch", 4),
                                 remove_deep_conv=getattr(self, "remove_deep_conv", False), **self._dmx_config())
        object.__setattr__(self, "_dmx_cache", (key, nm, versions))
        return nm

    def _dmx_training(self) -> bool:
        """Autograd is recording and some parameter is trainable: run the native training step."""
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _dmx_train_forward(self, x, t, y, vals, mask):
        """(eps, geom) through _NativeTrainFn; geom is None for networks without a GeomHead."""
        for name, v in (("x", x), ("cond_vals", vals), ("cond_mask", mask)):
            if v is not None and v.requires_grad:
                raise NotImplementedError(f"dmx training computes parameter gradients only ({name} requires grad)")
        bad = [n for n, p in self.named_parameters() if p.dtype != torch.float32 or not p.is_contiguous()]
        if bad:
            raise NotImplementedError(f"dmx training needs contiguous fp32 parameters ({bad[0]})")
        names = [n for n, _ in self.named_parameters()]
        eps, geom = _NativeTrainFn.apply(self, names, x, t, y, vals, mask, *self.parameters())
        return eps, (geom if geom.numel() else None)

    def _dmx_config(self) -> dict:
        """Extra dmx_model_config fields (num_classes, geom_dim, geom_hidden, scale_factor)."""
        return {}

    def _dmx_check_supported(self) -> None:
        """Raise for constructor arguments whose network libdmx does not implement."""

    def _apply(self, fn, *args, **kwargs):  # .to()/.cuda() invalidate the native copy
        object.__setattr__(self, "_dmx_cache", None)
        return super()._apply(fn, *args, **kwargs)


class _NativeTrainFn(torch.autograd.Function):
    """Native forward with a tape / native backward of the conditional U-Nets.

    Inputs after (module, names): x, t, y, vals, mask, *parameters (named_parameters order);
    outputs (eps, geom) — geom is an empty tensor for UnetCond.  Gradients flow to the
    parameters only (x, t, y, vals, mask take none, as in train_latent_cond.py:148).  A
    branch that did not run (cond_mlp without cond_vals) gets None, as torch autograd gives."""

    @staticmethod
    def forward(ctx, module, names, x, t, y, vals, mask, *params):
        nm = module.native()
        eps, geom, tape = nm.train_forward(x, t, y, vals, mask)
        ctx.nm, ctx.tape, ctx.names, ctx.cond = nm, tape, names, vals is not None
        ctx.set_materialize_grads(False)
        if geom is None:
            geom = eps.new_empty(0)
            ctx.mark_non_differentiable(geom)
        return eps, geom

    @staticmethod
    def backward(ctx, d_eps, d_geom):
        if d_geom is not None and d_geom.numel() == 0:
            d_geom = None
        grads = ctx.nm.train_backward(ctx.tape, d_eps, d_geom)
        out = []
        for n in ctx.names:  # parameters outside the graph of the used outputs get None, as in torch
            unused = ((not ctx.cond and n.startswith("cond_mlp.")) or (d_geom is None and n.startswith("geom_head."))
                      or (d_eps is None and n.startswith("out.")))
            out.append(None if unused else grads[n])
        return (None, None, None, None, None, None, None, *out)


class _NativeObjectiveFn(torch.autograd.Function):
    """The whole training objective as one node over the parameters (Diffuser.training_loss): native
    taped forward on the noised latent, native loss (dmx_objective_loss); backward = the loss's seed
    scaled by the upstream gradient on the device (dmx_objective_seed) into the native backward.

    Inputs after (module, names, job): *parameters (named_parameters order).  job: z_noisy, t, y, vals_used,
    mask_used (the network's inputs), noise, vals (the targets), weight, geom_lambda, denom, tmax (None:
    t is the caller's and is read back).  Outputs (loss, [loss, noise_loss, geom_loss, denom], per_sample, eps, geom);
    only loss is differentiable.  The rules for unused branches are _NativeTrainFn's: cond_mlp.* get None
    without cond, geom_head.* where the loss has no geometry term (geom_lambda == 0)."""

    @staticmethod
    def forward(ctx, module, names, job, *params):
        nm = module.native()
        eps, geom, tape = nm.train_forward(job["z_noisy"], job["t"], job["y"], job["vals_used"], job["mask_used"],
                                           tmax=job["tmax"])
        use_geom = geom is not None and job["vals"] is not None
        obj = _engine.objective_loss(eps, job["noise"], job["t"], job["weight"], geom if use_geom else None,
                                     job["vals"] if use_geom else None, job["mask_used"] if use_geom else None,
                                     job["geom_lambda"], job["denom"])
        ctx.nm, ctx.tape, ctx.names, ctx.obj = nm, tape, names, obj
        ctx.cond, ctx.geom_term = job["vals_used"] is not None, use_geom and job["geom_lambda"] != 0.0
        ctx.set_materialize_grads(False)
        if geom is None:
            geom = eps.new_empty(0)
        loss = obj.loss.clone()  # (the other scalars stay views of the kernel's output buffer)
        outs = (obj._out, obj.per_sample, eps, geom)
        ctx.mark_non_differentiable(*outs)
        return (loss, *outs)

    @staticmethod
    def backward(ctx, up, *_):
        if up is None:
            return (None, None, None, *[None for _ in ctx.names])
        d_eps, d_geom = _engine.objective_seed(ctx.obj, up, want_geom=ctx.geom_term)
        grads = ctx.nm.train_backward(ctx.tape, d_eps, d_geom)
        out = []
        for n in ctx.names:
            unused = (not ctx.cond and n.startswith("cond_mlp.")) or (d_geom is None and n.startswith("geom_head."))
            out.append(None if unused else grads[n])
        return (None, None, None, *out)


class _NativeVaeTrainFn(torch.autograd.Function):
    """Native forward with a tape / native backward of VAE.forward's network part (models/vae.py:51-69).

    Inputs after (module, names): x, eps (the randn draw of encode), *parameters (named_parameters
    order); outputs (x_recon, z, kl_per_sample).  Gradients flow to the parameters only (x and eps take
    none); an output the loss does not use contributes a zero cotangent."""

    @staticmethod
    def forward(ctx, module, names, x, eps, *params):
        nm = module.native()
        x_recon, z, kl, tape = nm.vae_train_forward(x, eps)
        ctx.nm, ctx.tape, ctx.names = nm, tape, names
        ctx.set_materialize_grads(False)
        return x_recon, z, kl

    @staticmethod
    def backward(ctx, d_recon, d_z, d_kl):
        grads = ctx.nm.vae_train_backward(ctx.tape, d_recon, d_z, d_kl)
        return (None, None, None, None, *[grads[n] for n in ctx.names])
