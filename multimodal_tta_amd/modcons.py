"""``modcons_tta``: modality-consistency adaptation, the cross-modal objective of the package - in the family of MM-TTA (Shin et
al., CVPR 2022, "MM-TTA: Multi-Modal Test-Time Adaptation for 3D Semantic Segmentation").  The other objectives score a voxel
from one forward of the whole input, or build their views from mirrors, turns and intensity draws; this one uses the fact
that a volume has several modalities: the prediction from all of them should agree with the prediction from each subset.
The agreement regularises entropy minimisation (a collapse has to happen consistently in every subset view) and adapts the
shared weights towards robustness to a missing modality - the shift ``method.missing_modalities`` models.

Per volume and step, with m_v the channel mask of view v and the weights w shared by the views:

    z_v = f(m_v x; w)                  v = 0..V-1   (V consecutive batch items on the volume's replica, train-mode norms)
    p_v = sigmoid(z_v) / softmax(z_v)
    H   = mean over elements of H(p_0)                              Tent's entropy of the full view
    K_v = mean over elements of KL(p_0 || p_v)        v >= 1        (Bernoulli per (voxel, region), categorical per voxel)
    L   = entropy_weight * H + weight * 1/(V-1) sum_v K_v
    one step of training.optimizer with dL/dw summed over the V views

View 0 keeps every present modality (the channels not in ``method.missing_modalities``); view v >= 1 keeps subset v of them:
``subsets: leave_one_out`` - one view per present modality with that modality zeroed -, ``single`` - one view per present
modality with only that one kept -, or an explicit list of lists of kept channel indices.  With ``detach: true`` the full
view is a teacher: no consistency gradient reaches z_0, which moves by the entropy term alone.  The views are staged once
per volume (``ops.modality_views``), outside the captured step; the step is one launch of ``ops.modcons_loss_items`` and its
finish between the forward and the backward.  The returned logits are the plain eval forward of view 0.

Where this differs from MM-TTA: one shared early-fusion network instead of a branch per modality; a KL to the full view
instead of pseudo-labels fused across the branches; views fixed per volume; no ensemble of the views in the returned logits;
it sits on top of Tent alone (not on SAR, MEMO, CoTTA and the rest); and not on the deep-fusion network, where a zeroed
channel is not an absent modality (the network averages over the encoders that are present).

``weight: 0`` takes the parent's step untouched - one view, nothing staged - and is ``entmin_tta`` bit for bit.  With
V > 1 the fused weight-gradient update is off (its reduction covers one batch item per set), as for ``memo_tta``.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import ops
from .config import as_cfg, expect, get_config, is_integer, is_number, method_block
from .models.unet import UNetRuntime
from .registry import register_plugin
from .tta import EntropyMinimizationTTA

MAX_VIEWS = 8
KEY = "method.modcons.subsets"
NAMED = ("leave_one_out", "single")


def parse_subsets(value: Any, key: str = KEY) -> Union[str, List[List[int]]]:
    """``leave_one_out``, ``single`` or a list of lists of channel indices (checked against the channels by ``keep_masks``)."""
    if isinstance(value, str):
        if value.lower() not in NAMED:
            raise ValueError(f"{key} = {value!r}: expected leave_one_out, single or a list of lists of kept channel indices")
        return value.lower()
    if isinstance(value, bytes) or not hasattr(value, "__iter__") or hasattr(value, "keys"):
        raise ValueError(f"{key} = {value!r}: expected leave_one_out, single or a list of lists of kept channel indices")
    subsets = []
    for s in value:
        if isinstance(s, (str, bytes)) or not hasattr(s, "__iter__") or hasattr(s, "keys"):
            raise ValueError(f"{key} = {list(value)!r}: {s!r} is no list of channel indices")
        idx = list(s)
        if not all(is_integer(i) for i in idx):
            raise ValueError(f"{key} = {list(value)!r}: {idx!r} is no list of channel indices")
        subsets.append([int(i) for i in idx])
    return subsets


def keep_masks(subsets: Union[str, Sequence[Sequence[int]]], channels: int, missing: Sequence[int] = (), key: str = KEY) -> List[int]:
    """The channel mask of every view (bit c = channel c kept): view 0 the present channels, view v >= 1 subset v of them."""
    channels = int(channels)
    present = [c for c in range(channels) if c not in set(int(i) for i in missing)]
    if len(present) < 2:
        raise ValueError(f"{key}: {len(present)} present modalities out of {channels} channels with method.missing_modalities = "
                         f"{list(missing)!r}; a subset view needs at least two")
    if subsets == "leave_one_out":
        chosen = [[c for c in present if c != drop] for drop in present]
    elif subsets == "single":
        chosen = [[c] for c in present]
    else:
        chosen = [list(s) for s in subsets]
        for s in chosen:
            for c in s:
                if not (0 <= c < channels):
                    raise ValueError(f"{key} = {chosen!r}: index {c} is outside the {channels} channels")
    full = sum(1 << c for c in present)
    masks = [full]
    for s in chosen:
        m = sum(1 << c for c in set(s)) & full          # intersected with the present set
        if m == 0:
            raise ValueError(f"{key} = {chosen!r}: the subset {s!r} keeps no present modality (an empty view)")
        if m == full:
            raise ValueError(f"{key} = {chosen!r}: the subset {s!r} keeps every present modality (it equals view 0)")
        if m in masks:
            raise ValueError(f"{key} = {chosen!r}: the subset {s!r} equals another subset")
        masks.append(m)
    if len(masks) < 2:
        raise ValueError(f"{key} = {chosen!r}: no subset (V = 1 + the number of subsets, 2 <= V <= {MAX_VIEWS})")
    if len(masks) > MAX_VIEWS:
        raise ValueError(f"{key} = {chosen!r}: V = {len(masks)} views (V = 1 + the number of subsets, 2 <= V <= {MAX_VIEWS})")
    return masks


def _weight(value: Any, key: str) -> float:
    expect(is_number(value) and value >= 0.0, key, value, "a finite number >= 0")
    return float(value)


@register_plugin("modcons_tta")
class ModalityConsistencyTTA(EntropyMinimizationTTA):
    """``method.modcons.subsets`` (default leave_one_out), ``weight`` (lambda, default 1.0; 0: ``entmin_tta``),
    ``entropy_weight`` (default 1.0) and ``detach`` (default true); the optimizer is ``training.optimizer`` exactly as for
    ``entmin_tta``.  The defaults are choices: nobody has measured a Dice with them."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "modcons")
        self.subsets = parse_subsets(get_config(s, "subsets", "leave_one_out"))
        self.weight = _weight(get_config(s, "weight", 1.0), "method.modcons.weight")
        self.entropy_weight = _weight(get_config(s, "entropy_weight", 1.0), "method.modcons.entropy_weight")
        self.detach = get_config(s, "detach", True)
        expect(isinstance(self.detach, bool), "method.modcons.detach", self.detach, "true or false")
        self._refuse_moddrop("true is not supported by modcons_tta (the subset views are staged once per volume, not once per "
                             "modality mask)")
        self.keep_masks: Optional[List[int]] = None
        self.views = 1
        if self.weight > 0.0:
            # the channel count is the model's: known here when the model block says it, else at setup
            mc = get_config(as_cfg(config), "model", {}) or {}
            channels = get_config(mc, "in_channels", None)
            if is_integer(channels) and channels > 0:
                self.resolve(channels)
            elif not isinstance(self.subsets, str):
                self.views = 1 + len(self.subsets)
        # the fused weight update reduces one batch item per parameter set; V views per set take the separate passes
        self.fused_update = self.views == 1

    def resolve(self, channels: int) -> List[int]:
        """The views of a model with ``channels`` input channels: ``keep_masks`` and ``views`` (ValueError naming
        ``method.modcons.subsets`` where the block does not fit the channels)."""
        if self.weight == 0.0:
            self.keep_masks, self.views = None, 1
        else:
            self.keep_masks = keep_masks(self.subsets, channels, self.missing)
            self.views = len(self.keep_masks)
        self.fused_update = self.views == 1
        return self.keep_masks

    def setup(self, model, device) -> "ModalityConsistencyTTA":
        if self.weight > 0.0:
            if getattr(model, "runtime_cls", None) is not UNetRuntime:
                raise NotImplementedError(f"modcons_tta drives the 'unet' model; {type(model).__name__} (the deep-fusion family) "
                                          "averages over the encoders that are present, so a zeroed channel is not an absent "
                                          "modality there")
            self.resolve(int(model.in_channels))
        super().setup(model, device)
        if self.views > 1:
            self._refuse_running_stats("modcons_tta", "the train-mode forward of the masked views")
        return self

    # ------------------------------------------------------------------ one step
    # ``losses`` holds L, ``entropy`` H and ``consistency`` C of every step
    records = EntropyMinimizationTTA.records + (("entropy", "modcons_entropy", torch.float32),
                                                ("consistency", "modcons_consistency", torch.float32))

    def _records(self):
        """``records``, and with V > 1 views the K_v and the hard disagreements with view 0: one [V-1] row per replica."""
        if self.views == 1:
            return self.records
        return self.records + (("view_kl", "modcons_view_kl", torch.float32, (self.views - 1,)),
                               ("disagree", "modcons_disagree", torch.int64, (self.views - 1,)))

    def _update(self, xv: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        if self.views == 1:
            super()._update(xv, present)          # entmin_tta's own step: its loss kernel, its fused update
            return
        rt = self.rt          # (batch items [g * V, (g + 1) * V) read / write parameter replica g)
        rt.pack_all()
        logits = self._forward(xv, present)
        dlogits = self._dlogits(logits)
        partial = rt.pool.flat("modcons_partial", ops.modcons_partials(logits, self.views), dtype=torch.float64)
        loss = rt.pool.flat("ent_loss", rt.group)
        entropy = rt.pool.flat("modcons_entropy", rt.group)
        consistency = rt.pool.flat("modcons_consistency", rt.group)
        k = self.views - 1
        view_kl = rt.pool.flat("modcons_view_kl", rt.group * k, zero=True)
        disagree = rt.pool.flat("modcons_disagree", rt.group * k, dtype=torch.int64, zero=True)
        ops.modcons_loss_items(logits, dlogits, self.views, partial, loss, entropy, consistency, view_kl, disagree,
                               weight=self.weight, entropy_weight=self.entropy_weight, detach=self.detach, softmax=self.softmax)
        self._backward_and_step(dlogits, int(logits.shape[0]) // self.views)

    # ------------------------------------------------------------------ per volume
    def _stage(self, x_cl: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
        if self.views == 1:
            return super()._stage(x_cl)
        rt = self.rt
        n, d, h, w, c = x_cl.shape
        rt.views = self.views          # every launch of the loop carries V consecutive batch items per volume
        xv = rt.pool.cl("modcons_views", n * self.views, d, h, w, c, ldc=(c + 3) // 4 * 4, zero=True, dtype=x_cl.dtype)
        ops.modality_views(x_cl, xv, self.keep_masks)
        return xv, ()

    def _final_logits(self, x_cl: torch.Tensor, xv: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        self.rt.views = 1          # view 0 alone: one batch item per replica again
        return super()._final_logits(x_cl, xv, present)

    @torch.no_grad()
    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """``EntropyMinimizationTTA.adapt_volume`` plus ``entropy`` and ``consistency`` per step (as ``losses``), ``view_kl``
        fp32 [steps, B, V-1] and ``disagree`` int64 [steps, B, V-1] (``weight: 0``: ``entropy`` = ``losses``, the rest empty or
        zero).  Every volume brings its V views onto its own replica: a call takes at most ``method.group`` volumes."""
        B = int(x.shape[0])
        if self.views > 1:
            self._check_volumes(B, "modcons_tta adapts ", " (the V views of a volume share its parameter replica)",
                                NotImplementedError)
        out = super().adapt_volume(x, steps)
        if self.views == 1:
            out["entropy"] = out["losses"].clone()
            out["consistency"] = torch.zeros_like(out["losses"])
            out["view_kl"] = torch.zeros((len(out["losses"]), B, 0), dtype=torch.float32, device=x.device)
            out["disagree"] = torch.zeros((len(out["losses"]), B, 0), dtype=torch.int64, device=x.device)
        return out
