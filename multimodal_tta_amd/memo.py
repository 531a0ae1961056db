"""``memo_tta``: MEMO (Zhang, Levine, Finn, NeurIPS 2022, "MEMO: Test Time Robustness via Adaptation and Augmentation") on
the native engine, next to ``entmin_tta`` (Tent) and ``sar_tta`` (SAR) - the method that was designed for one test point
adapted episodically: minimise the entropy of the prediction AVERAGED over several augmented views of the one input.

Per volume and step, with F_v = view v's map (mirrors, quarter turns: exact on the voxel grid, with an exact inverse) and the
weights w shared by the views:

    z_v  = f(F_v x; w)                      v = 0..V-1   (V consecutive batch items on the volume's replica, train-mode norms)
    u_v  = F_v^-1 z_v                                    (back in the volume's own frame)
    pbar = 1/V sum_v sigmoid(u_v)           L = mean over (region, voxel) of H_bern(pbar)            (sigmoid head)
    pbar = 1/V sum_v softmax_r(u_v)         L = mean over voxel of -sum_r pbar_r log pbar_r            (softmax head)
    one step of training.optimizer with dL/dw summed over the V views

The views are every subset of ``method.memo.mirror_axes`` (nnU-Net's test-time mirroring): V = 2^k, view v mirrors
``mirror_axes[i]`` iff bit i of v is set, view 0 is the volume itself.  ``method.memo.rot90.k`` (default []) adds quarter turns
in the (H, W) plane - the one geometric augmentation the upstream trainer applies (``RandRotate90d(max_k=3)``): the views are
then ({identity} + the turns of k) x the mirror group, mirror index fastest, V = 2^len(mirror_axes) * (1 + len(k)); an odd turn
needs H == W.  After the last step: the eval-mode forward of the
unmirrored volume (``ensemble: false``), or of all views, combined as logit(pbar) / log pbar (``ensemble: true``).

Where this differs from the paper: the views are the mirror group and the quarter turns instead of AugMix samples (the
augmentations whose inverse is exact on the voxel grid, so the views' predictions meet in one frame without resampling); the elements are
voxels (or voxel x region pairs), not images; the step count is ``method.steps``, shared with Tent.

With ``mirror_axes: []`` (V = 1) the method IS ``entmin_tta``: the same launches, bit for bit.  With V > 1 the fused
weight-gradient update is off (its reduction covers one batch item per set).  The class is its step (``_update``), the
staging of the views (``_stage``) and the ensemble (``_final_logits``); the per-volume loop is ``EntropyMinimizationTTA``'s.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .config import expect, get_config, is_integer, method_block
from .intensity import parse_intensity
from .registry import register_plugin
from .tta import EntropyMinimizationTTA, modality_mask

AXIS_BITS = {"w": 1, "h": 2, "d": 4}          # the kernels' mirror masks: bit 0 = W, bit 1 = H, bit 2 = D (torch D, H, W)


def parse_mirror_axes(value: Any, key: str = "method.memo.mirror_axes") -> List[str]:
    """A list of distinct axes out of d, h, w; ``key``: the config key it came from, for the messages."""
    if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
        raise ValueError(f"{key} = {value!r}: expected a list of axes out of d, h, w")
    axes = [str(a).lower() for a in value]
    for a in axes:
        if a not in AXIS_BITS:
            raise ValueError(f"{key} = {list(value)!r}: unknown axis {a!r} (d, h or w)")
    if len(set(axes)) != len(axes):
        raise ValueError(f"{key} = {list(value)!r}: an axis is repeated")
    return axes


# a quarter turn in the (H, W) plane as a view code: bit 4 = transpose H and W, THEN the mirrors of bits 0-2.  On a
# channels-last item [D, H, W, C], torch.rot90(x, k, dims=(H, W)) is code ROT90_CODES[k] (tests/test_rot90_host.py derives it)
ROT90_CODES = {1: 18, 2: 3, 3: 17}
TRANSPOSE = 16


def parse_rot90(value: Any, key: str = "method.memo.rot90") -> List[int]:
    """The ``rot90`` block ``{k: [...]}`` (or None for the default, no turns): a list of distinct quarter-turn counts out of
    1, 2, 3; ``key``: the config key it came from, for the messages."""
    value = {} if value is None else value
    if not hasattr(value, "keys"):
        raise ValueError(f"{key} = {value!r}: expected a mapping with the key k (a list of quarter turns out of 1, 2, 3)")
    for name in value.keys():
        if name != "k":
            raise ValueError(f"{key}.{name}: unknown key (expected k)")
    k = get_config(value, "k", [])
    if isinstance(k, (str, bytes)) or not hasattr(k, "__iter__") or hasattr(k, "keys"):
        raise ValueError(f"{key}.k = {k!r}: expected a list of quarter turns out of 1, 2, 3")
    turns = list(k)
    for t in turns:
        if not is_integer(t) or t not in ROT90_CODES:
            raise ValueError(f"{key}.k = {turns!r}: {t!r} is no quarter-turn count (1, 2 or 3)")
    if len(set(turns)) != len(turns):
        raise ValueError(f"{key}.k = {turns!r}: a turn is repeated")
    return [int(t) for t in turns]


def rotated_code(turn_code: int, mask: int) -> int:
    """The code of "mirror ``mask`` after the view ``turn_code``": the mirrors act on the view's own axes."""
    return (turn_code & TRANSPOSE) | ((turn_code & 7) ^ mask)


def check_square(view_axes: Sequence[int], h: int, w: int, key: str = "method.memo.rot90") -> None:
    """An odd quarter turn (a code with bit 4) needs H == W: raise before anything is staged or launched."""
    if h != w and any(int(a) & TRANSPOSE for a in view_axes):
        raise ValueError(f"{key}.k: an odd quarter turn needs square (H, W) planes, the volume has H = {h}, W = {w} "
                         "(k: [2] is the only turn of a non-square plane)")


def view_masks(axes: Sequence[str]) -> List[int]:
    """The mirror mask of every view: view v mirrors axes[i] iff bit i of v is set (view 0 = the volume itself)."""
    return [sum(AXIS_BITS[a] for i, a in enumerate(axes) if (v >> i) & 1) for v in range(1 << len(axes))]


@register_plugin("memo_tta")
class MarginalEntropyTTA(EntropyMinimizationTTA):
    """``method.memo.mirror_axes`` (default [h, w]: 4 views), ``method.memo.rot90`` (default {k: []}) and
    ``method.memo.ensemble`` (default false); the optimizer is
    ``training.optimizer`` exactly as for ``entmin_tta``."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "memo")
        self.mirror_axes = parse_mirror_axes(get_config(s, "mirror_axes", ["h", "w"]))
        self.ensemble = get_config(s, "ensemble", False)
        expect(isinstance(self.ensemble, bool), "method.memo.ensemble", self.ensemble, "true or false")
        self.rot90 = parse_rot90(get_config(s, "rot90", None), "method.memo.rot90")
        self.intensity = parse_intensity(get_config(s, "intensity", None), self.mirror_axes, "method.memo.intensity", self.rot90)
        # ({identity} + the quarter turns) x the mirror group, ``intensity.copies`` times over
        self.view_axes = self.intensity.view_axes
        self.views = len(self.view_axes)
        self._refuse_moddrop("true is not supported by memo_tta (one modality mask per step for all views is not defined yet)")
        # the fused weight update reduces one batch item per parameter set; V views per set take the separate passes
        self.fused_update = self.views == 1

    def setup(self, model, device) -> "MarginalEntropyTTA":
        super().setup(model, device)
        self._setup_ordinals()          # the intensity views' per-volume numbers
        return self

    # ------------------------------------------------------------------ one step
    def _update(self, xv: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        if self.views == 1:
            super()._update(xv, present)          # entmin_tta's own step: its loss kernel, its fused update
            return
        rt = self.rt          # (batch items [g * V, (g + 1) * V) read / write parameter replica g)
        rt.pack_all()
        logits = self._forward(xv, present)
        dlogits = self._dlogits(logits)
        partial = rt.pool.flat("memo_partial", ops.memo_partials(logits, self.views), dtype=torch.float64)
        loss = rt.pool.flat("ent_loss", rt.group)
        ops.memo_loss_items(logits, dlogits, self.view_axes, partial, loss, softmax=self.softmax)
        self._backward_and_step(dlogits, int(logits.shape[0]) // self.views)

    # ------------------------------------------------------------------ per volume
    def _stage(self, x_cl: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
        if self.views == 1:
            return super()._stage(x_cl)
        check_square(self.view_axes, int(x_cl.shape[2]), int(x_cl.shape[3]), "method.memo.rot90")
        self.rt.views = self.views          # every launch of the loop carries V consecutive batch items per volume
        if not self.intensity.active:
            return self.rt.stage_views(x_cl, self.view_axes), ()
        present = modality_mask(int(x_cl.shape[-1]), self.missing, 0.0, None)
        return self.rt.stage_views(x_cl, self.view_axes, self.intensity, self._ordinals_host, present), ()

    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None,
                     ordinals: Optional[Sequence[int]] = None) -> Dict[str, Any]:
        """As ``entmin_tta.adapt_volume``.  ``ordinals``: one number per volume for the draws of the intensity views
        (default: the volumes served so far), as for ``cotta_tta``; without intensity views they are counted and unused."""
        if self.rt is not None and ((self.views > 1 and self.intensity.active) or ordinals is not None):
            self._take_ordinals(int(x.shape[0]), ordinals)
        elif self.rt is not None:
            self._served += int(x.shape[0])
        return super().adapt_volume(x, steps)

    def _final_logits(self, x_cl: torch.Tensor, xv: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        if self.views == 1 or not self.ensemble:
            self.rt.views = 1          # the volumes alone: one batch item per replica again
            return super()._final_logits(x_cl, xv, present)
        zv = self._forward(xv, present)
        n, d, h, w, r = zv.shape
        logits_cl = self.rt.pool.cl("memo_ensemble", int(x_cl.shape[0]), d, h, w, r, ldc=(r + 3) // 4 * 4)
        ops.memo_ensemble(zv, logits_cl, self.view_axes, softmax=self.softmax)
        return logits_cl
