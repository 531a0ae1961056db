"""``crf_tta``: entropy minimisation with a pairwise grid-CRF (Potts) regulariser in the loss (Tang et al., ECCV 2018, "On
Regularized Losses for Weakly-supervised CNN Segmentation"; the contour term of Hu et al., MICCAI 2021, "Fully Test-time
Adaptation for Image Segmentation" is the same idea).  The entropy objectives score every voxel on its own and leave a
scattering of small, confident false-positive islands; ``lame_tta`` answers that after the fact, on the outputs.  Here the
spatial prior sits inside the step, so the WEIGHTS learn it while they adapt.  Per volume and step

    L      = H + weight * P                                         H: entmin_tta's mean entropy
    P      = 1 / (2 n E) * sum_i sum_{j in N(i)} a_ij phi(p_i, p_j)   n = connectivity, E = the volume's element count
    phi    = potts:      sum_r [p_ir (1 - p_jr) + (1 - p_ir) p_jr]   (softmax head: 1 - sum_k p_ik p_jk)
             quadratic:  sum_k (p_ik - p_jk)^2
    a_ij   = exp(-sum_{c present} (x_ic - x_jc)^2 / (2 sigma^2));   sigma = 0: a_ij = 1

over the 6 / 18 / 26 spatial neighbours N(i) - LAME's stencil and LAME's affinity on the staged modalities, with a gradient
(``ops.crf_entropy_items``: loss and gradient in one pass over the logits, inside the captured step).  x is the staged volume
(bf16 or fp32 as the model stages it), ``present`` the run's ``missing_modalities`` mask - modality dropout draws do not
enter: the base mask is used, and on a runtime that re-stages the volume with every step's draw zeroed (the deep-fusion
network) the stencil reads a copy staged once per volume under the base mask.

Where this differs from the papers: the neighbours are those of the voxel grid, not a dense CRF; the affinity is taken on
the staged intensities, with no distance in mm; the regional nuclear-norm term of Hu et al. is a plugin of its own
(``bnm_tta``, bnm.py), not a second term here; the term sits on top of Tent alone (not on SAR / MEMO / CoTTA / EATA / DeYO).

The class is ``_update`` with the loss call swapped - the stencil needs the logits in memory, so the step gives up the
head-loss epilogue of the last convolution - and the ``entropy`` / ``pairwise`` records; the per-volume loop - groups, lanes,
the captured step - is ``EntropyMinimizationTTA``'s.  ``weight: 0`` takes the parent's step untouched and is ``entmin_tta``
bit for bit.
"""
from __future__ import annotations

from typing import Any, Optional, Sequence

import torch

from . import ops
from .config import expect, get_config, is_integer, is_number, method_block
from .registry import register_plugin
from .tta import EntropyMinimizationTTA, modality_mask

MAX_WEIGHT = 16.0
MIN_SIGMA = 1e-18          # below about 4.6e-20 the factor 1 / (2 sigma^2) overflows fp32 (mmtta_crf_entropy_items refuses it)
CONNECTIVITIES = (6, 18, 26)
FORMS = ops.CRF_FORMS


@register_plugin("crf_tta")
class CrfRegularizedTTA(EntropyMinimizationTTA):
    """``method.crf.weight`` ([0, 16], default 1.0; 0: ``entmin_tta``), ``sigma`` (>= 0, default 1.0; 0: no affinity),
    ``connectivity`` (6, 18 or 26, default 26) and ``form`` (``potts`` | ``quadratic``, default ``potts``); everything else
    is ``entmin_tta``'s, with one limit.  Every volume is its own objective with its own record slots, so a call takes at
    most ``method.group`` volumes (``entmin_tta`` with ``group: 1`` accepts a batch that shares the one weight set; here that
    is a ``ValueError``).  (bf16 thin gradients need the tiled route, that is <= 4 input channels: the runtimes store them
    only then - models/unet.py requires ``in_channels <= 4`` for bf16 storage - so the generic route always meets fp32.)"""

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "crf")
        wt, sg = get_config(s, "weight", 1.0), get_config(s, "sigma", 1.0)
        cn, fm = get_config(s, "connectivity", 26), get_config(s, "form", "potts")
        expect(is_number(wt) and 0.0 <= wt <= MAX_WEIGHT, "method.crf.weight", wt,
               f"a finite number in [0, {MAX_WEIGHT:g}] (0: entmin_tta)")
        expect(is_number(sg) and (sg == 0.0 or sg >= MIN_SIGMA), "method.crf.sigma", sg,
               f"0 (no affinity) or a finite number >= {MIN_SIGMA:g}")
        expect(is_integer(cn) and cn in CONNECTIVITIES, "method.crf.connectivity", cn, "6, 18 or 26")
        expect(isinstance(fm, str) and fm in FORMS, "method.crf.form", fm, f"one of {', '.join(FORMS)}")
        self.weight, self.sigma, self.connectivity, self.form = float(wt), float(sg), int(cn), str(fm)
        # one slot per replica each.  weight 0 is the parent's step: its loss is the entropy, and nothing writes `pairwise`
        if self.weight > 0.0:
            self.records = (("losses", "crf_loss", torch.float32), ("entropy", "crf_entropy", torch.float32),
                            ("pairwise", "crf_pairwise", torch.float32))
        else:
            self.records = (("losses", "ent_loss", torch.float32), ("entropy", "ent_loss", torch.float32),
                            ("pairwise", "crf_pairwise", torch.float32))

    def _stage(self, x_cl: torch.Tensor):
        """The step input and, where the loop re-stages the volume with every step's dropout draw zeroed (a runtime that does
        not mask on load), a copy of the volume as staged under the base mask for the stencil: the draws stay out of the
        affinity.  The copy is a pool buffer with a stable address (the captured step reads it)."""
        x_step, views = super()._stage(x_cl)
        rt = self.rt
        restaged = self.moddrop_p > 0.0 and not getattr(rt, "input_mask_on_load", False)
        if restaged and self.weight > 0.0 and self.sigma > 0.0:
            n, d, h, w, c = x_cl.shape
            x_aff = rt.pool.cl("crf_x", n, d, h, w, c, ldc=int(x_cl.stride(3)), zero=True, dtype=x_cl.dtype)
            x_aff.copy_(x_cl)
            views = tuple(views) + (x_aff,)
        return x_step, views

    def _update(self, x: torch.Tensor, present: Optional[Sequence[bool]], x_aff: Optional[torch.Tensor] = None) -> None:
        """The parent's sequence - pack, forward, objective, backward, optimizer - with the objective swapped: the forward
        stores its logits (no head-loss tail), and one pass over them leaves L, H, P and dL/dlogits.  ``x_aff``: the volume
        the affinity reads when that is not the step input (``_stage``)."""
        if self.weight == 0.0:
            super()._update(x, present)
            return
        if x_aff is None:
            x_aff = x
        rt = self.rt
        self._check_volumes(int(x.shape[0]), "crf_tta adapts ")          # (every volume is its own objective, with own record slots)
        rt.pack_all(fused_current=True)
        loss = rt.pool.flat("crf_loss", rt.group)
        entropy = rt.pool.flat("crf_entropy", rt.group)
        pairwise = rt.pool.flat("crf_pairwise", rt.group)
        logits = self._forward(x, present)
        dlogits = self._dlogits(logits)
        partial = rt.pool.flat("crf_partial", ops.crf_partials(logits), dtype=torch.float64)
        # the staged volume holds whatever the loader delivered in the absent channels (models/unet.py masks on load): the
        # run's base mask keeps them out of the affinity; the per-step dropout draws do not enter (x_aff)
        base = modality_mask(int(x_aff.shape[-1]), self.missing, 0.0, None)
        ops.crf_entropy_items(logits, x_aff if self.sigma > 0.0 else None, dlogits, partial, loss, entropy, pairwise,
                              connectivity=self.connectivity, weight=self.weight, sigma=self.sigma, form=self.form,
                              present=base, softmax=self.softmax)
        self._backward_and_step(dlogits, int(logits.shape[0]), fused=True)
