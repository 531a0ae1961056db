"""``lame_tta``: LAME (Boudiaf et al., CVPR 2022, "Parameter-free Online Test-time Adaptation") on the native engine - the one
method of the comparison that is of another kind than ``entmin_tta`` (Tent), ``sar_tta``, ``memo_tta``, ``cotta_tta``,
``eata_tta`` and ``deyo_tta``: it leaves the weights alone and corrects the OUTPUTS.  It looks for posteriors that stay close
to the model's own (a KL term) while neighbours with similar inputs agree (a Laplacian term); it cannot collapse a model.

For a volume the neighbours of a voxel are its 6 / 18 / 26 spatial neighbours, with an affinity from the input modalities.
Per volume, after the ``method.steps`` entropy steps of the parent (``steps: 0``: pure LAME on the source model, otherwise
Tent followed by the refinement), with l0 the logits ``entmin_tta`` would have returned:

    l(0)       = l0
    l_i(t+1)   = l0_i  + weight * sum_j w_ij tanh(l_j(t) / 2)           (sigmoid head, every region on its own)
    l_ik(t+1)  = l0_ik + weight * sum_j w_ij softmax(l_j(t))_k          (softmax head, no re-centring)
    w_ij       = exp(-sum_{c present} (x_ic - x_jc)^2 / (2 sigma^2)) / n,   n = connectivity;  sigma = 0: w_ij = 1 / n

for ``iterations`` synchronous iterations (``ops.lame_refine``, one launch each, outside the captured step, on the caller's
stream).  x is the staged volume (bf16 or fp32 as the model stages it), ``present`` the run's ``missing_modalities`` mask -
modality dropout draws do not enter: the base mask is used.  ``adapt_volume`` also returns ``flipped`` ([B] int64 on the
device): the elements whose hard prediction the refinement changed.

Where this differs from the paper: the iteration runs in logit space (the official code's 1e-10 inside its logarithm is
not restated); the neighbours are spatial, with a Gaussian affinity on the input intensities, not k nearest neighbours in
feature space; the iteration count is fixed (the paper's energy-based stop would need a device-to-host read inside the
lane); w is a_ij / n with the constant n, so it stays symmetric.

The class is ``_final_logits`` (the hook where a method decides what logits it returns) and the ``flipped`` record; the
per-volume loop - groups, lanes, the captured step - is ``EntropyMinimizationTTA``'s.  ``iterations: 0`` launches nothing
and is ``entmin_tta`` bit for bit.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence

import torch

from . import ops
from .config import expect, get_config, is_integer, is_number, method_block
from .registry import register_plugin
from .tta import EntropyMinimizationTTA, modality_mask

MAX_ITERATIONS = 64
MAX_WEIGHT = 16.0
CONNECTIVITIES = (6, 18, 26)


@register_plugin("lame_tta")
class LaplacianRefinedTTA(EntropyMinimizationTTA):
    """``method.lame.iterations`` (0 .. 64, default 10), ``weight`` ((0, 16], default 1.0), ``sigma`` (>= 0, default 1.0; 0:
    no affinity) and ``connectivity`` (6, 18 or 26, default 26); everything else is ``entmin_tta``'s."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "lame")
        it, wt = get_config(s, "iterations", 10), get_config(s, "weight", 1.0)
        sg, cn = get_config(s, "sigma", 1.0), get_config(s, "connectivity", 26)
        expect(is_integer(it) and 0 <= it <= MAX_ITERATIONS, "method.lame.iterations", it, f"an integer of 0 .. {MAX_ITERATIONS}")
        expect(is_number(wt) and 0.0 < wt <= MAX_WEIGHT, "method.lame.weight", wt, f"a finite number in (0, {MAX_WEIGHT:g}]")
        expect(is_number(sg) and sg >= 0.0, "method.lame.sigma", sg, "a finite number >= 0 (0: no affinity)")
        expect(is_integer(cn) and cn in CONNECTIVITIES, "method.lame.connectivity", cn, "6, 18 or 26")
        self.iterations, self.weight, self.sigma, self.connectivity = int(it), float(wt), float(sg), int(cn)
        self._flipped: Optional[torch.Tensor] = None

    def _final_logits(self, x_cl: torch.Tensor, x_step: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        """The parent's logits, refined.  They stay where the forward left them (nothing below writes them); the result and
        the second ping-pong buffer are pool buffers with stable names of the same row width."""
        logits = super()._final_logits(x_cl, x_step, present)
        n, d, h, w, r = logits.shape
        pool = self.rt.pool
        self._flipped = pool.flat("lame_flipped", n, dtype=torch.int64, zero=True)
        if self.iterations == 0:
            return logits
        ldc = int(logits.stride(3))
        out = pool.cl("lame_logits", n, d, h, w, r, ldc=ldc, zero=True)
        work = pool.cl("lame_work", n, d, h, w, r, ldc=ldc, zero=True)
        # the staged volume holds whatever the loader delivered in the absent channels (models/unet.py masks on load): the
        # run's base mask keeps them out of the affinity; the per-step dropout draws do not enter
        base = modality_mask(int(x_cl.shape[-1]), self.missing, 0.0, None)
        ops.lame_refine(logits, x_cl if self.sigma > 0.0 else None, out, work, self._flipped, connectivity=self.connectivity,
                        weight=self.weight, sigma=self.sigma, iterations=self.iterations, present=base, softmax=self.softmax)
        return out

    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """As ``entmin_tta.adapt_volume``, plus ``flipped`` ([B] int64, device): per volume the elements whose hard prediction
        the refinement changed (zeros for ``iterations: 0``)."""
        res = super().adapt_volume(x, steps)
        res["flipped"] = self._flipped[:int(x.shape[0])]
        return res
