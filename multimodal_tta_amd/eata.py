"""``eata_tta``: EATA (Niu et al., ICML 2022, "Efficient Test-Time Model Adaptation without Forgetting") on the native
engine, next to ``entmin_tta`` (Tent), ``sar_tta`` (SAR), ``memo_tta`` (MEMO) and ``cotta_tta`` (CoTTA) - the method whose
pull back towards the source model is deterministic, and the second one made for ``episodic: false``: a reliable-entropy
step whose kept elements are weighted by how far below the margin they lie, plus a penalty on the distance from the source
weights, weighted by a diagonal Fisher estimate.

Per volume and step (each volume of a group on its own weight replica ``w``; ``w0`` the source weights, ``F`` the Fisher
estimate, ``m = e_margin * ln K`` with K = 2 for the sigmoid head's (voxel, region) elements and K = R for the softmax head's
voxels):

    z = f(x; w);  keep = H(z) < m;  c = exp(m - H(z))                  (c carries no gradient; 1 < c <= e^m)
    L = sum over keep of c H / |keep|                                  (NaN and a zero gradient when nothing is kept, as SAR)
    g = dL/dw
    g_i += 2 lam F_i (w_i - w0_i);  P = lam sum_i F_i (w_i - w0_i)^2   (the trainable span; skipped when lam = 0)
    one step of training.optimizer with g

The Fisher estimate comes from N volumes at the source weights (``estimate_fisher``), with the model's own hard prediction as
the label:

    z = f(x; w0) (train-mode norms, as the step);  y = 1[z >= 0]       (softmax head: one-hot of the first arg max)
    l = mean over elements of BCE(z, y)                                (softmax head: mean over voxels of lse(z) - max z)
    F += (dl/dw)^2                                                     (fp32, volumes in the order given);  F /= N at the end

``F`` is one fp32 span over the trainable parameters, shared by all replicas (and by the lanes of an evaluator), read-only
while volumes adapt, and it survives the episodic reset.

Where this differs from the paper: the elements are voxels (or voxel x region pairs), not images; the margin is a fraction
of ln K; the redundancy filter is not built (for a K = 2 element the cosine between (p, 1 - p) and a moving average of it is a
function of p alone, a second confidence threshold next to the margin, and with voxels of one forward pass there is no
backward pass it could save); the Fisher samples are test or validation volumes handed to ``estimate_fisher``, not 2000
ImageNet images; the step count is ``method.steps``.

Scope: the fused weight-gradient update is off (the gradient has to exist in the arena before the penalty is added to it).
The class is its step (``_update``), two more per-step records and the Fisher estimate; the per-volume loop - groups, lanes,
the captured step, the final forward - is ``EntropyMinimizationTTA``'s.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, Optional, Sequence

import torch

from . import ops
from .config import expect, get_config, is_integer, is_number, method_block
from .ops import MmttaError
from .registry import register_plugin
from .tta import EntropyMinimizationTTA, drop_modality, modality_mask


def fisher_to_state(span: torch.Tensor, refs: Sequence[Any], volumes: int) -> Dict[str, Any]:
    """The flat Fisher span as ``{"volumes": N, "fisher": {parameter name: tensor}}`` (trainable parameters of ``refs`` only,
    host tensors in the parameters' shapes)."""
    return {"volumes": int(volumes),
            "fisher": {r.name: span[r.offset:r.offset + r.numel].detach().reshape(r.shape).cpu().clone()
                       for r in refs if r.trainable}}


def fisher_from_state(state: Dict[str, Any], refs: Sequence[Any], n_train: int, device) -> torch.Tensor:
    """The inverse of ``fisher_to_state``: the flat fp32 span [n_train] (zero in the alignment gaps between parameters)."""
    if not isinstance(state, dict) or "fisher" not in state or "volumes" not in state:
        raise MmttaError("a Fisher state is {'volumes': N, 'fisher': {parameter name: tensor}}")
    if int(state["volumes"]) < 1:
        raise MmttaError(f"a Fisher state of {state['volumes']} volumes")
    entries = state["fisher"]
    span = torch.zeros(max(int(n_train), 1), dtype=torch.float32)
    for r in refs:
        if not r.trainable:
            continue
        if r.name not in entries:
            raise MmttaError(f"the Fisher state has no entry for the trainable parameter {r.name!r}")
        t = entries[r.name]
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(r.shape):
            raise MmttaError(f"the Fisher state's {r.name!r} has shape {tuple(getattr(t, 'shape', ()))}, the parameter "
                             f"{tuple(r.shape)}")
        span[r.offset:r.offset + r.numel] = t.detach().to(torch.float32).reshape(-1).cpu()
    return span[:int(n_train)].to(device) if n_train > 0 else span[:0].to(device)


@register_plugin("eata_tta")
class FisherRegularizedTTA(EntropyMinimizationTTA):
    """``method.eata.e_margin`` (fraction of ln K, default 0.4), ``fisher_alpha`` (lam, default 2000.0, the paper's),
    ``fisher.volumes`` (default 8) and ``fisher.path`` (default null); the optimizer is ``training.optimizer`` exactly as
    for ``entmin_tta``."""
    fused_update = False     # the gradient must exist in the arena before the penalty is added to it

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "eata")
        f = get_config(s, "fisher", {}) or {}
        margin, lam, vols = get_config(s, "e_margin", 0.4), get_config(s, "fisher_alpha", 2000.0), get_config(f, "volumes", 8)
        expect(is_number(margin) and margin > 0.0, "method.eata.e_margin", margin, "a finite positive fraction of ln K")
        expect(is_number(lam) and lam >= 0.0, "method.eata.fisher_alpha", lam, "a finite weight >= 0")
        expect(is_integer(vols) and vols >= 1, "method.eata.fisher.volumes", vols, "an integer >= 1")
        self.e_margin, self.fisher_alpha, self.fisher_volumes = float(margin), float(lam), int(vols)
        path = get_config(f, "path", None)
        self.fisher_path: Optional[str] = None if path in (None, "", "null") else str(path)
        self.fisher: Optional[torch.Tensor] = None          # fp32 [n_train], shared by the replicas (and the lanes)
        self.fisher_count = 0                               # the volumes behind it

    def margin(self, regions: int) -> float:
        """The entropy margin in nats: e_margin * ln K."""
        return self.e_margin * math.log(float(regions) if self.softmax else 2.0)

    @property
    def needs_fisher(self) -> bool:
        """True while the regulariser is on and no Fisher estimate is in place (an evaluator then provides one)."""
        return self.fisher_alpha > 0.0 and self.fisher is None

    # ------------------------------------------------------------------ one step
    # ``losses`` holds L without the penalty, ``kept`` the number of elements below the margin, ``penalty`` P
    records = EntropyMinimizationTTA.records + (("kept", "eata_kept", torch.int64), ("penalty", "eata_penalty", torch.float32))

    def _update(self, x: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        rt, ar = self.rt, self.rt.arena
        rt.pack_all()
        logits = self._forward(x, present)
        dlogits = self._dlogits(logits)
        n, d, h, w, r = logits.shape
        slots = rt.group
        elems = n * d * h * w * (1 if self.softmax else r)
        partial = rt.pool.flat("eata_partial", ops.entropy_weighted_partials(logits), dtype=torch.float64)
        loss = rt.pool.flat("ent_loss", slots)
        kept = rt.pool.flat("eata_kept", slots, dtype=torch.int64)
        keep = rt.pool.flat("eata_keep", elems, dtype=torch.uint8)
        penalty = rt.pool.flat("eata_penalty", slots, zero=True)
        ops.entropy_weighted_items(logits, dlogits, self.margin(r), keep, partial, loss, kept, softmax=self.softmax)
        self._backward_and_step(dlogits, n, between=lambda: self._fisher_penalty(min(n, ar.replicas), penalty))

    def _fisher_penalty(self, sets: int, penalty: torch.Tensor) -> None:
        """Between the backward and the optimizer: g += 2 lam F (w - w0) on the first ``sets`` replicas, P into ``penalty``."""
        rt, ar = self.rt, self.rt.arena
        if self.fisher_alpha > 0.0:
            pen_partial = rt.pool.flat("eata_pen_partial", ops.fisher_penalty_partials(ar.n_train, sets), dtype=torch.float64)
            ops.fisher_penalty_sets(ar.params_all, ar.grads_all, self.fisher, ar.source, ar.n_train, sets, self.fisher_alpha,
                                    pen_partial, penalty)

    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """As ``entmin_tta.adapt_volume``, plus ``kept`` and ``penalty`` per step ([steps], or [steps, B] for a group).  As
        for ``sar_tta``, a runtime without parameter sets (``group`` 1) takes one volume per call: the objective keeps one
        loss / count slot per weight replica, and more batch items than that end in an ``MmttaError`` from ``ops``."""
        if self.rt is not None and self.fisher_alpha > 0.0 and self.rt.arena.n_train > 0 and self.fisher is None:
            raise MmttaError(f"eata_tta: method.eata.fisher_alpha = {self.fisher_alpha:g} needs a Fisher estimate: call "
                             "estimate_fisher(volumes) or load_fisher(state), or set method.eata.fisher.path")
        return super().adapt_volume(x, steps)

    # ------------------------------------------------------------------ the Fisher estimate
    @torch.no_grad()
    def estimate_fisher(self, volumes: Iterable[torch.Tensor]) -> int:
        """The Fisher estimate from ``volumes`` ([B,C,D,H,W] tensors, B <= ``method.group``) at the source weights; the
        volumes of a tensor run as one grouped launch sequence, volume b on replica b.  Returns the number of volumes used.
        Weights, running statistics and the optimizer's step counter are the source's afterwards."""
        if self.rt is None:
            raise MmttaError("call setup(model, device) first")
        rt, ar = self.rt, self.rt.arena
        nt = ar.n_train
        span = torch.zeros(max(nt, 1), dtype=torch.float32, device=ar.device)[:nt]
        self._reset()          # every replica holds the source
        count = 0
        try:
            for x in volumes:
                B = int(x.shape[0])
                if B > rt.group:
                    raise ValueError(f"method.group = {rt.group}: at most {rt.group} volumes per tensor, got {B}")
                count += self._fisher_launches(x.float(), span)
        finally:
            rt.training = False
            rt.use_sets = False
            self._reset()
        if count < 1:
            raise ValueError("estimate_fisher: no volumes")
        if nt > 0:
            ops.fisher_scale(span, nt, count)
        self.set_fisher(span, count)
        return count

    def _fisher_launches(self, x: torch.Tensor, span: torch.Tensor) -> int:
        """Forward with the step's switches, pseudo-label loss, backward, F += g^2 for the volumes of ``x``."""
        rt, ar = self.rt, self.rt.arena
        B, C = int(x.shape[0]), int(x.shape[1])
        present = None
        if self.missing:
            base = modality_mask(C, self.missing, 0.0, None)
            if getattr(rt, "supports_present", False):
                present = base
            if not getattr(rt, "input_mask_on_load", False):
                x = drop_modality(x, base)
        x_cl = rt.stage_input(x)
        ops.Workspace.lane = self.lane
        rt.training = True
        rt.use_sets = rt.group > 1
        rt.pack_all()
        logits = self._forward(x_cl, present)
        dlogits = self._dlogits(logits)
        partial = rt.pool.flat("eata_pl_partial", ops.pseudo_label_partials(logits), dtype=torch.float64)
        loss = rt.pool.flat("eata_pl_loss", max(rt.group, B))
        ops.pseudo_label_loss_items(logits, dlogits, partial, loss, softmax=self.softmax)
        if ar.n_train > 0:
            rt.run_backward(dlogits)
            # (a runtime without parameter sets takes one volume per tensor - estimate_fisher refuses more - and has the one
            # gradient; several volumes on one weight set would give the square of their summed gradient, not F)
            ops.fisher_accumulate_sets(span, ar.grads_all, ar.n_train, min(B, ar.replicas) if rt.group > 1 else 1)
        rt.training = False
        rt.use_sets = False
        return B

    def set_fisher(self, span: Optional[torch.Tensor], volumes: int = 0) -> None:
        """Use ``span`` (fp32 [n_train] on the plugin's device; not copied, so lanes can share one) as the Fisher estimate."""
        if span is not None:
            ar = self.rt.arena
            if span.dtype != torch.float32 or span.dim() != 1 or span.numel() != ar.n_train or span.device != ar.params.device \
                    or not span.is_contiguous():
                raise MmttaError(f"set_fisher: expected a contiguous fp32 [{ar.n_train}] span on {ar.params.device}, got "
                                 f"{tuple(span.shape)} {span.dtype} on {span.device}")
        self.fisher, self.fisher_count = span, int(volumes) if span is not None else 0
        self._graphs.clear()          # a captured step holds the address of the span it was captured with

    def fisher_state(self) -> Dict[str, Any]:
        """``{"volumes": N, "fisher": {state_dict key: tensor}}`` of the trainable parameters; ``torch.save`` of it is the
        file ``method.eata.fisher.path`` names."""
        if self.fisher is None:
            raise MmttaError("eata_tta: no Fisher estimate (estimate_fisher / load_fisher)")
        return fisher_to_state(self.fisher, self.rt.arena.refs, self.fisher_count)

    def load_fisher(self, state: Any) -> None:
        """``state``: what ``fisher_state`` returns, or the path of a file that holds it."""
        if self.rt is None:
            raise MmttaError("call setup(model, device) first")
        if isinstance(state, str):
            state = torch.load(state, map_location="cpu", weights_only=True)
        ar = self.rt.arena
        self.set_fisher(fisher_from_state(state, ar.refs, ar.n_train, ar.params.device), int(state["volumes"]))
