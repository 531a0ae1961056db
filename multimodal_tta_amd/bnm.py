"""``bnm_tta``: entropy minimisation minus a regional nuclear-norm term (Cui et al., CVPR 2020, "Towards Discriminability and
Diversity: Batch Nuclear-norm Maximization"; the regional nuclear-norm term of Hu et al., MICCAI 2021, "Fully Test-time
Adaptation for Image Segmentation", whose contour term is ``crf_tta``).  Every entropy objective is content when the minority
class - a small tumour - is pushed to confident background.  The nuclear norm of the prediction matrix is bounded below by
its Frobenius norm, so it rewards confidence, and it grows with the rank, so it rewards every class staying alive; it needs
no prior from the user.  Per volume and step, over a grid of boxes of ``block`` voxels (border boxes are smaller),

    L      = entropy_weight * H - weight * N                        H: entmin_tta's mean entropy
    N      = 1 / Q * sum_A nu(A)                                      Q: the matrices of the volume
    nu(A)  = sum_k sqrt(lambda_k(A^T A) + eps m) / sqrt(m min(m, K))   m: the box's voxels

with one m x K matrix of softmax rows per box on the softmax head (K = R) and one m x 2 matrix of rows (p, 1 - p) per box and
region on the sigmoid head (``ops.nuclear_entropy_items``: a Gram reduction, an eigenproblem per matrix and a gradient pass,
inside the captured step).  ``block: [0, 0, 0]`` is the whole volume - Cui et al.'s matrix with the voxels as the batch -,
``[16, 16, 16]`` the regional form of Hu et al.

Where this differs from both papers: the norm is smoothed (eps m under the root: differentiable at a confident, rank-1 box,
and a vanishing singular value is pushed with a bounded force); it is normalised by sqrt(m min(m, K)) to (0, 1], so one
weight serves every box size; the sigmoid head has no class axis to take a rank over, so each region gets the K = 2 Bernoulli
matrix; the regions are a grid of boxes, not pooled or overlapping ones, and in voxels, not mm; the term sits on top of Tent
alone (not on SAR / MEMO / CoTTA / EATA / DeYO, and not together with ``crf_tta``).

The class is ``_update`` with the loss call swapped - the reduction needs the logits in memory, so the step gives up the
head-loss epilogue of the last convolution - and the ``entropy`` / ``nuclear`` records; the per-volume loop - groups, lanes,
the captured step - is ``EntropyMinimizationTTA``'s.  ``weight: 0`` (with ``entropy_weight: 1``) takes the parent's step
untouched and is ``entmin_tta`` bit for bit.
"""
from __future__ import annotations

from typing import Any, Optional, Sequence

import torch

from . import ops
from .config import expect, get_config, is_integer, is_number, method_block
from .registry import register_plugin
from .tta import EntropyMinimizationTTA

MAX_WEIGHT = 16.0
MIN_EPS, MAX_EPS = 1e-6, 0.1


@register_plugin("bnm_tta")
class NuclearNormTTA(EntropyMinimizationTTA):
    """``method.bnm.weight`` ([0, 16], default 1.0; 0: ``entmin_tta``), ``entropy_weight`` ([0, 16], default 1.0; 0: BNM
    proper, the nuclear norm alone), ``block`` (three integers >= 0, default ``[0, 0, 0]``: the whole volume) and ``eps``
    ([1e-6, 0.1], default 1e-4); everything else is ``entmin_tta``'s, with one limit: every volume is its own objective with
    its own record slots, so a call takes at most ``method.group`` volumes."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "bnm")
        wt, ew = get_config(s, "weight", 1.0), get_config(s, "entropy_weight", 1.0)
        bk, ep = get_config(s, "block", [0, 0, 0]), get_config(s, "eps", 1e-4)
        expect(is_number(wt) and 0.0 <= wt <= MAX_WEIGHT, "method.bnm.weight", wt,
               f"a finite number in [0, {MAX_WEIGHT:g}] (0: entmin_tta)")
        expect(is_number(ew) and 0.0 <= ew <= MAX_WEIGHT, "method.bnm.entropy_weight", ew,
               f"a finite number in [0, {MAX_WEIGHT:g}] (0: the nuclear norm alone)")
        if wt == 0.0 and ew != 1.0:
            raise ValueError(f"method.bnm.entropy_weight = {ew!r}: with method.bnm.weight = 0 the step is entmin_tta's, "
                             "whose entropy weight is 1")
        bk = list(bk) if not isinstance(bk, (str, bytes)) and hasattr(bk, "__iter__") else bk
        expect(isinstance(bk, list) and len(bk) == 3 and all(is_integer(b) and b >= 0 for b in bk), "method.bnm.block", bk,
               "three integers >= 0 (0: the whole extent)")
        expect(is_number(ep) and MIN_EPS <= ep <= MAX_EPS, "method.bnm.eps", ep, f"a finite number in [{MIN_EPS:g}, {MAX_EPS:g}]")
        self.weight, self.entropy_weight, self.block, self.eps = float(wt), float(ew), [int(b) for b in bk], float(ep)
        # one slot per replica each.  weight 0 is the parent's step: its loss is the entropy, and nothing writes `nuclear`
        if self.weight > 0.0:
            self.records = (("losses", "bnm_loss", torch.float32), ("entropy", "bnm_entropy", torch.float32),
                            ("nuclear", "bnm_nuclear", torch.float32))
        else:
            self.records = (("losses", "ent_loss", torch.float32), ("entropy", "ent_loss", torch.float32),
                            ("nuclear", "bnm_nuclear", torch.float32))

    def _update(self, x: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        """The parent's sequence - pack, forward, objective, backward, optimizer - with the objective swapped: the forward
        stores its logits (no head-loss tail), and the passes over them leave L, H, N and dL/dlogits."""
        if self.weight == 0.0:
            super()._update(x, present)
            return
        rt = self.rt
        self._check_volumes(int(x.shape[0]), "bnm_tta adapts ")          # (every volume is its own objective, with own record slots)
        rt.pack_all(fused_current=True)
        loss = rt.pool.flat("bnm_loss", rt.group)
        entropy = rt.pool.flat("bnm_entropy", rt.group)
        nuclear = rt.pool.flat("bnm_nuclear", rt.group)
        logits = self._forward(x, present)
        dlogits = self._dlogits(logits)
        scratch = rt.pool.flat("bnm_scratch", ops.nuclear_scratch(logits, self.block, self.softmax), dtype=torch.float64)
        ops.nuclear_entropy_items(logits, dlogits, scratch, loss, entropy, nuclear, block=self.block, weight=self.weight,
                                  entropy_weight=self.entropy_weight, eps=self.eps, softmax=self.softmax)
        self._backward_and_step(dlogits, int(logits.shape[0]), fused=True)
