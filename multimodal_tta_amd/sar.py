"""``sar_tta``: SAR (Niu et al., ICLR 2023, "Towards Stable Test-Time Adaptation in Dynamic Wild World") on the
native engine, next to ``entmin_tta`` (Tent).

Per volume and step (each volume of a group on its own weight replica):

    z1 = f(x; w);  keep1 = H(z1) < m;  L1 = mean of H over keep1;  g1 = dL1/dw
    w_saved = w;  w += rho * g1 / (||g1|| + 1e-12)          (the norm over every trainable parameter of the replica)
    z2 = f(x; w);  keep2 = keep1 & (H(z2) < m);  L2 = mean of H over keep2;  g2 = dL2/dw
    w = w_saved;  base-optimizer step with g2

with m = e_margin * ln K (K = 2 for the sigmoid head's Bernoulli elements (voxel, region), K = R for the softmax head's
voxels).  An empty filter gives L = NaN and a zero gradient, as torch's mean over an empty selection does.  Where this
differs from the classification paper: the elements are voxels (or voxel x region pairs), not images; the margin is a
fraction of ln K so that one default serves both heads; SAR's model-recovery reset is not built (it targets continual runs,
this package resets every volume).

The class is its step (``_update``) and one more per-step record; the per-volume loop, the captured step and the final
forward are ``EntropyMinimizationTTA``'s.
"""
from __future__ import annotations

import math
from typing import Any, Optional, Sequence

import torch

from . import ops
from .config import expect, get_config, is_number, method_block
from .registry import register_plugin
from .tta import EntropyMinimizationTTA, select_params


@register_plugin("sar_tta")
class SharpnessAwareReliableTTA(EntropyMinimizationTTA):
    """``method.sar.e_margin`` (fraction of ln K, default 0.4) and ``method.sar.rho`` (SAM radius, default 0.05), the SAR
    paper's defaults; the base optimizer is ``training.optimizer`` exactly as for ``entmin_tta``."""
    fused_update = False     # the ascent needs the whole gradient (its norm) before any weight moves

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "sar")
        # (converted before the check: a numeric string or a bool passes, unlike in the later methods)
        self.e_margin = float(get_config(s, "e_margin", 0.4))
        self.rho = float(get_config(s, "rho", 0.05))
        expect(is_number(self.e_margin) and self.e_margin > 0.0, "method.sar.e_margin", self.e_margin,
               "a finite positive fraction of ln K")
        expect(is_number(self.rho) and self.rho >= 0.0, "method.sar.rho", self.rho, "a finite radius >= 0")

    def setup(self, model, device) -> "SharpnessAwareReliableTTA":
        if not select_params(model, self.params_spec):
            # torch SAR has no gradient to take the ascent along either
            raise ValueError(f"sar_tta: method.params = {self.params_spec!r} selects no trainable parameter")
        return super().setup(model, device)

    def margin(self, regions: int) -> float:
        """The entropy margin in nats: e_margin * ln K."""
        return self.e_margin * math.log(float(regions) if self.softmax else 2.0)

    # ------------------------------------------------------------------ one step
    # ``losses`` holds L1 per step, ``kept`` the number of elements that passed the first filter
    records = EntropyMinimizationTTA.records + (("kept", "sar_kept", torch.int64),)

    def _update(self, x: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        rt, ar = self.rt, self.rt.arena
        rt.pack_all()
        logits = self._forward(x, present)
        dlogits = self._dlogits(logits)
        n, d, h, w, r = logits.shape
        slots = rt.group
        elems = n * d * h * w * (1 if self.softmax else r)
        margin = self.margin(r)
        partial = rt.pool.flat("sar_partial", ops.entropy_filtered_partials(logits), dtype=torch.float64)
        loss1 = rt.pool.flat("ent_loss", slots)          # the recorded loss is L1
        loss2 = rt.pool.flat("sar_loss2", slots)
        kept1 = rt.pool.flat("sar_kept", slots, dtype=torch.int64)
        kept2 = rt.pool.flat("sar_kept2", slots, dtype=torch.int64)
        keep1 = rt.pool.flat("sar_keep1", elems, dtype=torch.uint8)
        keep2 = rt.pool.flat("sar_keep2", elems, dtype=torch.uint8)
        ops.entropy_filtered_items(logits, dlogits, margin, None, keep1, partial, loss1, kept1, softmax=self.softmax)
        rt.run_backward(dlogits)
        # ascent: w_saved = w, w += rho g1 / ||g1|| per replica in use; the packed images follow the arena
        sets = min(n, ar.replicas)
        saved = rt.pool.flat("sar_saved", ar.replicas * ar.n_train).view(ar.replicas, ar.n_train)
        sam_partial = rt.pool.flat("sar_sam_partial", ops.sam_ascent_partials(ar.n_train, sets), dtype=torch.float64)
        ops.sam_ascent_sets(ar.params_all, ar.grads_all, saved, sam_partial, ar.n_train, sets, self.rho)
        rt.pack_all()
        logits = self._forward(x, present)
        ops.entropy_filtered_items(logits, dlogits, margin, keep1, keep2, partial, loss2, kept2, softmax=self.softmax)
        # exact restore (SAR's SAM copies old_p back), then the base optimizer with the gradient taken at w + eps
        self._backward_and_step(dlogits, n, between=lambda: ar.params_all[:sets, :ar.n_train].copy_(saved[:sets]))
