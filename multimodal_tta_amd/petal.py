"""``petal_tta``: PETAL (Brahma & Rai, CVPR 2023, "A Probabilistic Framework for Lifelong Test-Time Adaptation") on the
native engine, next to ``cotta_tta`` (CoTTA) and ``eata_tta`` (EATA) - the third method made for ``episodic: false``.  It is
CoTTA's mean teacher and consistency loss (``cotta.py``: views, target, loss, teacher average, all unchanged) with the
restore decided by the data: after every step, in every parameter tensor, the elements the step's own gradient says least
about - the smallest Fisher information of the step, the squared gradient of its loss - return to the source values.

The rule, per weight replica s and trainable tensor t of n_t elements, with g the gradient the step's backward left in
``Arena.grads_all`` (of the loss alone, before any weight decay), ``key(g) = bits(g) & 0x7fffffff`` read as an unsigned
integer and delta = ``method.petal.quantile``:

    k_t     = floor(delta * n_t)                  on the host, in double, once per model; 0 <= k_t < n_t
    gamma   = the k_t-th smallest key of tensor t in replica s      (0-based; an element's own bits, never interpolated)
    w_i    <- source_i (the source BITS) where key(g_i) < gamma; otherwise unchanged

The keys are a total order over zeros (+0 == -0), denormals, infinities and NaNs.  Elements whose key ties with gamma stay:
a tensor whose gradient is all zero restores nothing (those elements did not move either), ``k_t = 0`` restores nothing, and
without ties at gamma exactly k_t elements of the tensor are restored.  Optimizer moments are left alone, as in CoTTA's
restore; the alignment padding between the tensors of the arena belongs to no tensor and is never restored.

Where this differs from the paper: the ranking is on |g|, not g^2 (the same order, and a square can underflow); the
threshold is an order statistic, not ``torch.quantile``'s interpolated value, so small tensors with delta * n_t < 1 restore
nothing; the SWAG posterior over the weights and the source-prior regulariser are not built (``eata_tta``'s Fisher pull
covers that ground); views and elements are CoTTA's as built here (mirror group and quarter turns, voxels).

Two launch sequences per step on top of CoTTA's: ``ops.magnitude_select_sets`` (a radix select per tensor and replica,
seven launches whatever the data, inside the captured step) and ``ops.petal_update_sets`` (one streaming pass: teacher
average + restore) in place of ``ops.cotta_update_sets``.  ``quantile: 0`` skips the select and equals ``cotta_tta`` with
``restore_p: 0`` bit for bit.  Scope and refusals (BatchNorm models, ``moddrop.enabled``) are CoTTA's.
"""
from __future__ import annotations

import math
from typing import Any, List, Optional, Sequence, Tuple

import torch

from . import ops
from .config import expect, get_config, is_number, method_block
from .cotta import MeanTeacherTTA
from .registry import register_plugin


def rank_rows(refs: Sequence[Any], quantile: float) -> List[Tuple[int, int, int]]:
    """The rows (offset, numel, k_t = floor(quantile * numel)) of the trainable ``Arena.refs``, both decay groups, ascending
    by offset; the alignment padding between two tensors is in no row."""
    rows = []
    for r in sorted((r for r in refs if r.trainable and r.numel > 0), key=lambda r: r.offset):
        k = int(math.floor(float(quantile) * r.numel))
        rows.append((int(r.offset), int(r.numel), min(max(k, 0), r.numel - 1)))
    return rows


@register_plugin("petal_tta")
class FisherRestoreTTA(MeanTeacherTTA):
    """``method.petal.mirror_axes``, ``rot90``, ``intensity`` and ``alpha`` as ``method.cotta``'s, and ``quantile`` (default
    0.03, the paper's): the share of every parameter tensor - its elements of least gradient magnitude - that returns to the
    source after a step."""
    block = "petal"

    def __init__(self, config: Any = None):
        super().__init__(config)
        q = get_config(method_block(config, "petal"), "quantile", 0.03)
        expect(is_number(q) and 0.0 <= q < 1.0, "method.petal.quantile", q, "a share with 0 <= quantile < 1")
        self.quantile = float(q)
        self.restore_p = 0.0          # (no stochastic restore: the keys of method.cotta that method.petal does not carry)
        self.table: Optional[ops.RankTable] = None
        self.gamma: Optional[torch.Tensor] = None          # [replicas, rows] int32: the thresholds' uint32 bits

    def setup(self, model, device) -> "FisherRestoreTTA":
        super().setup(model, device)
        ar = self.rt.arena
        rows = rank_rows(ar.refs, self.quantile)
        self.table = ops.rank_segments_table(rows, ar.device) if rows else None
        self.gamma = torch.zeros((ar.replicas, max(len(rows), 1)), dtype=torch.int32, device=ar.device)
        return self

    def _after_step(self, sets: int, restored: torch.Tensor) -> None:
        """Select, then update: the thresholds of every (replica, tensor) from the step's gradient, then teacher EMA +
        ranked restore in one pass.  ``quantile: 0``: no select, the thresholds stay 0 and nothing lies below them."""
        rt, ar = self.rt, self.rt.arena
        nt = ar.n_train
        if self.table is None:
            return
        if self.quantile > 0.0:
            scratch = rt.pool.flat("petal_select", ops.magnitude_select_scratch(self.table, ar.replicas), dtype=torch.int32)
            ops.magnitude_select_sets(ar.grads_all, self.table, sets, self.gamma, scratch)
        upd = rt.pool.flat("petal_upd_partial", ops.petal_update_partials(nt, sets), dtype=torch.int64)
        ops.petal_update_sets(ar.params_all, self.teacher, ar.source, ar.grads_all, self.gamma, self.table, nt, sets,
                              self.alpha, upd, restored)
