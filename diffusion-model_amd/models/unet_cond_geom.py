"""Drop-in ``models.unet_cond_geom`` (reference models/unet_cond_geom.py:26-100)."""
from __future__ import annotations

import torch

from dmx import _lib
from dmx import engine as _engine
from models._modules import GeomHead
from models.unet_cond import UnetCond


class UnetCondWithGeomHead(UnetCond):
    """UnetCond + GeomHead; forward returns (eps_pred, geom_pred) like the reference."""

    _dmx_kind = _lib.DMX_UNET_COND_GEOM

    def __init__(self, in_ch=4, time_dim=256, num_classes=3, cfg_drop_prob=0.0, remove_deep_conv=False,
                 geom_dim=12, geom_hidden=256):
        super().__init__(in_ch=in_ch, time_dim=time_dim, num_classes=num_classes, cfg_drop_prob=cfg_drop_prob,
                         remove_deep_conv=remove_deep_conv)
        self.geom_head = GeomHead(in_ch=64, out_dim=geom_dim, hidden=geom_hidden)
        self._geom_dim, self._geom_hidden = geom_dim, geom_hidden

    def _dmx_config(self) -> dict:
        return {"num_classes": self.num_classes, "geom_dim": self._geom_dim, "geom_hidden": self._geom_hidden}

    def forward(self, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cond_vals: torch.Tensor = None,
                cond_mask: torch.Tensor = None, cond_drop_prob: float = 0.0):
        use = cond_vals is not None and cond_mask is not None  # unet_cond_geom.py:91 (no dropout here)
        return self._run(x, t, y, cond_vals if use else None, cond_mask if use else None, want_geom=True)

    def geom_grad(self, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cond_vals: torch.Tensor,
                  cond_mask: torch.Tensor):
        """The geometry-guidance loss and its gradient with respect to x ->
        (loss (n,), grad (n,c,h,w), geom (n,geom_dim), eps): per sample
        L_n = sum_j m_nj (geom_nj - v_nj)^2 / max(sum_j m_nj, 1e-6) with geom the GeomHead's output on
        (x, t, y, cond_vals, cond_mask) and v, m the same cond_vals / cond_mask, and dL_n/dx by the
        native data-only backward (NativeModel.geom_grad).  Works in eval mode and under no_grad: no
        autograd graph is built, nothing here is differentiable further, and no parameter gets a
        gradient.  forward() with an x that requires grad keeps raising NotImplementedError."""
        if cond_vals is None or cond_mask is None:
            raise ValueError("geom_grad needs cond_vals and cond_mask (the loss's target)")
        _engine.require_cuda(x, "x")
        with torch.no_grad():
            return self.native().geom_grad(x, t, y, cond_vals, cond_mask)
