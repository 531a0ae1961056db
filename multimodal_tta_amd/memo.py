"""``memo_tta``: MEMO (Zhang, Levine, Finn, NeurIPS 2022, "MEMO: Test Time Robustness via Adaptation and Augmentation") on
the native engine, next to ``entmin_tta`` (Tent) and ``sar_tta`` (SAR) - the method that was designed for one test point
adapted episodically: minimise the entropy of the prediction AVERAGED over several augmented views of the one input.

Per volume and step, with F_v = mirror along view v's axes (its own inverse) and the weights w shared by the views:

    z_v  = f(F_v x; w)                      v = 0..V-1   (V consecutive batch items on the volume's replica, train-mode norms)
    u_v  = F_v z_v                                       (back in the volume's own frame)
    pbar = 1/V sum_v sigmoid(u_v)           L = mean over (region, voxel) of H_bern(pbar)            (sigmoid head)
    pbar = 1/V sum_v softmax_r(u_v)         L = mean over voxel of -sum_r pbar_r log pbar_r            (softmax head)
    one step of training.optimizer with dL/dw summed over the V views

The views are every subset of ``method.memo.mirror_axes`` (nnU-Net's test-time mirroring): V = 2^k, view v mirrors
``mirror_axes[i]`` iff bit i of v is set, view 0 is the volume itself.  After the last step: the eval-mode forward of the
unmirrored volume (``ensemble: false``), or of all views, combined as logit(pbar) / log pbar (``ensemble: true``).

Where this differs from the paper: the views are the mirror group instead of AugMix samples (the one augmentation whose
inverse is exact on the voxel grid, so the views' predictions meet in one frame without resampling); the elements are
voxels (or voxel x region pairs), not images; the step count is ``method.steps``, shared with Tent.

With ``mirror_axes: []`` (V = 1) the method IS ``entmin_tta``: the same launches, bit for bit.  With V > 1 the fused
weight-gradient update is off (its reduction covers one batch item per set).  Everything else - episodic reset, groups,
lanes, the captured step - is ``entmin_tta``'s.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch

from . import ops
from .config import as_cfg, get_config
from .registry import register_plugin
from .tta import EntropyMinimizationTTA, drop_modality, modality_mask

AXIS_BITS = {"w": 1, "h": 2, "d": 4}          # the kernels' mirror masks: bit 0 = W, bit 1 = H, bit 2 = D (torch D, H, W)


def parse_mirror_axes(value: Any) -> List[str]:
    """``method.memo.mirror_axes``: a list of distinct axes out of d, h, w."""
    if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
        raise ValueError(f"method.memo.mirror_axes = {value!r}: expected a list of axes out of d, h, w")
    axes = [str(a).lower() for a in value]
    for a in axes:
        if a not in AXIS_BITS:
            raise ValueError(f"method.memo.mirror_axes = {list(value)!r}: unknown axis {a!r} (d, h or w)")
    if len(set(axes)) != len(axes):
        raise ValueError(f"method.memo.mirror_axes = {list(value)!r}: an axis is repeated")
    return axes


def view_masks(axes: Sequence[str]) -> List[int]:
    """The mirror mask of every view: view v mirrors axes[i] iff bit i of v is set (view 0 = the volume itself)."""
    return [sum(AXIS_BITS[a] for i, a in enumerate(axes) if (v >> i) & 1) for v in range(1 << len(axes))]


@register_plugin("memo_tta")
class MarginalEntropyTTA(EntropyMinimizationTTA):
    """``method.memo.mirror_axes`` (default [h, w]: 4 views) and ``method.memo.ensemble`` (default false); the optimizer is
    ``training.optimizer`` exactly as for ``entmin_tta``."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        m = get_config(as_cfg(config), "method", {}) or {}
        s = get_config(m, "memo", {}) or {}
        self.mirror_axes = parse_mirror_axes(get_config(s, "mirror_axes", ["h", "w"]))
        ens = get_config(s, "ensemble", False)
        if not isinstance(ens, bool):
            raise ValueError(f"method.memo.ensemble = {ens!r}: expected true or false")
        self.ensemble = ens
        self.view_axes = view_masks(self.mirror_axes)
        self.views = len(self.view_axes)
        if bool(get_config(get_config(m, "moddrop", {}) or {}, "enabled", False)):
            raise NotImplementedError("method.moddrop.enabled: true is not supported by memo_tta (one modality mask per step "
                                      "for all views is not defined yet)")
        # the fused weight update reduces one batch item per parameter set; V views per set take the separate passes
        self.fused_update = self.views == 1

    def setup(self, model, device) -> "MarginalEntropyTTA":
        super().setup(model, device)          # (tells the model its views: EntropyMinimizationTTA.setup)
        if self.tune_volumes is None and self.views > 1:
            # `auto`: launch geometry for the items actually in flight - lanes x group x views, with the group the runtime
            # settled on (models that fall back to group 1 are tuned for group 1)
            ops.tune_for_volumes_in_flight(self.lanes * self.group * self.views)
        return self

    # ------------------------------------------------------------------ one step
    def _step_launches(self, x_cl: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        if self.views == 1:
            super()._step_launches(x_cl, present)          # entmin_tta's own step: its loss kernel, its fused update
            return
        rt, ar = self.rt, self.rt.arena
        V = self.views
        ops.Workspace.lane = self.lane
        rt.training = True
        rt.use_sets = rt.group > 1          # batch items [g * V, (g + 1) * V) read / write parameter replica g
        try:
            rt.pack_all()
            logits = rt.forward_cl(x_cl) if present is None else rt.forward_cl(x_cl, present=present)
            n, d, h, w, r = logits.shape
            gdt = rt.thin_grad_dtype() if (not self.softmax and r <= 4) else torch.float32
            dlogits = rt.pool.cl("dlogits", n, d, h, w, r, ldc=(r + 3) // 4 * 4, dtype=gdt)
            partial = rt.pool.flat("memo_partial", ops.memo_partials(logits, V), dtype=torch.float64)
            loss = rt.pool.flat("ent_loss", rt.group if rt.group > 1 else 1)
            ops.memo_loss_items(logits, dlogits, self.view_axes, partial, loss, softmax=self.softmax)
            if ar.n_train > 0:
                rt.run_backward(dlogits)
                self.optimizer_step(n // V)
        finally:
            rt.use_sets = False

    # ------------------------------------------------------------------ per volume
    @torch.no_grad()
    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """As ``entmin_tta.adapt_volume``: x [B,C,D,H,W] (B <= ``method.group`` volumes), the final logits of the volumes
        ([B,D,H,W,R] channels-last, in the volumes' own frame) and the per-step losses."""
        if self.rt is None or self.views == 1:
            return super().adapt_volume(x, steps)
        rt, ar = self.rt, self.rt.arena
        V = self.views
        steps = self.steps if steps is None else int(steps)
        B = int(x.shape[0])
        if B > rt.group:
            raise ValueError(f"method.group = {rt.group}: at most {rt.group} volumes per call, got {B}")
        if self.episodic:
            ar.restore_source()
            rt.restore_buffers()
        C = x.shape[1]
        masked = bool(self.missing)
        base_present = modality_mask(C, self.missing, 0.0, None)
        x = x.float()
        wants_present = masked and getattr(rt, "supports_present", False)
        restage = masked and not getattr(rt, "input_mask_on_load", False)
        # mask, then mirror: the views are views of the volume the network is given
        x_cl = rt.stage_input(drop_modality(x, base_present) if restage else x)
        present = base_present if wants_present else None
        grouped = rt.group > 1
        loss_hist = rt.pool.flat("loss_hist", max(steps, 1) * (B if grouped else 1))
        loss_buf = rt.pool.flat("ent_loss", rt.group if grouped else 1)
        if grouped:
            loss_hist = loss_hist.view(max(steps, 1), B)
        rt.views = V          # every launch below carries V consecutive batch items per volume
        try:
            xv = rt.stage_views(x_cl, self.view_axes)
            for t in range(steps):
                self._step(xv, present)
                if grouped:
                    loss_hist[t].copy_(loss_buf[:B])
                else:
                    loss_hist[t:t + 1].copy_(loss_buf)
            rt.training = False
            ops.Workspace.lane = self.lane
            rt.use_sets = grouped
            rt.pack_all()
            if self.ensemble:
                zv = rt.forward_cl(xv, present=present) if wants_present else rt.forward_cl(xv)
                n, d, h, w, r = zv.shape
                logits_cl = rt.pool.cl("memo_ensemble", B, d, h, w, r, ldc=(r + 3) // 4 * 4)
                ops.memo_ensemble(zv, logits_cl, self.view_axes, softmax=self.softmax)
            else:
                rt.views = 1          # the volumes alone: one batch item per replica again
                logits_cl = rt.forward_cl(x_cl, present=present) if wants_present else rt.forward_cl(x_cl)
        finally:
            rt.use_sets = False
            rt.views = 1
        losses = loss_hist[:steps]
        return {"logits_cl": logits_cl, "losses": losses[:, 0] if (grouped and B == 1) else losses}
