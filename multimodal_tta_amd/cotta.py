"""``cotta_tta``: CoTTA (Wang et al., CVPR 2022, "Continual Test-Time Domain Adaptation") on the native engine, next to
``entmin_tta`` (Tent), ``sar_tta`` (SAR) and ``memo_tta`` (MEMO) - the mean-teacher method, and the one made for
``episodic: false``: the student learns from the augmentation-averaged prediction of a teacher that is an exponential moving
average of the student, and after every step a random small share of the student's weights returns to the source values.

Per volume and step (each volume of a group on its own weight replica), with F_v = view v's map (mirrors, and the quarter
turns of ``method.cotta.rot90.k``, as ``memo_tta``), w the student, w' the teacher and w0 the source weights:

    t  = logit( 1/V sum_v sigmoid(F_v^-1 f(F_v x; w')) )         (softmax head: log of the mean softmax)   no gradient
    z  = f(x; w)
    L  = mean over (voxel, region) of -q log sigmoid(z) - (1 - q) log sigmoid(-z),  q = sigmoid(t)        (sigmoid head)
    L  = mean over voxels of -sum_r exp(t_r) log softmax(z)_r                                             (softmax head)
    one step of training.optimizer on w with dL/dw
    w' = alpha w' + (1 - alpha) w                              (w after its step)
    w_i = w0_i where u_i < restore_p                           (u: Philox4x32-10, see below)

The teacher runs through the student's own launches: the trainable span of the arena is saved, the teacher written in its
place, the images repacked, the V views forwarded (train-mode norms, as the student's step) and the span copied back.  The
teacher is one fp32 span per weight replica, set to the source weights with the arena (setup, the episodic reset); with
``episodic: false`` teacher and student persist across volumes.  After the last step the returned logits are the eval-mode
forward of the STUDENT on the unmirrored volume, as for Tent.

The restore draw: ``u_i = (word >> 8) * 2^-24`` with word number ``i & 3`` of Philox4x32-10 under the key
``(seed & 0xffffffff, seed >> 32)`` at the counter ``(i >> 2, t, ordinal, 0)``; ``i`` is the element's index in the replica's
trainable span (``Arena.refs`` maps it to parameters), ``t`` the arena's device step counter after the optimizer step (1 for
the first step of a volume, read on the device so that a replayed graph draws anew) and ``ordinal`` a per-volume number -
by default the count of volumes this plugin has served since ``setup`` (lane ``l`` of an evaluator starts at ``l * 2^24``),
or ``adapt_volume(..., ordinals=[...])``.  The ordinal, not the replica slot, enters the draw: a group of volumes equals the
same volumes served one at a time.

Where this differs from the paper: the views are the mirror group and quarter turns in the (H, W) plane
(``method.cotta.mirror_axes``, ``method.cotta.rot90``, ``memo_tta``'s views: the augmentations whose inverse is exact on the
voxel grid) and, with ``method.cotta.affine`` (``affine.py``: off as shipped), small rotations / zooms / shifts that are
resampled - the teacher's predictions take no gradient, so such a view is a gather forward (``ops.affine_views``) and a
gather back (``ops.affine_ensemble`` in place of ``ops.memo_ensemble``) - not AugMix or colour jitter; the teacher always averages
its views (the paper's confidence-gated switch between one and 32 views is not built); the elements are voxels (or voxel x
region pairs), not images; the restore draw is per element of the flat trainable span, not per tensor.

Scope: the fused weight-gradient update is off (the step's gradient is taken with the separate passes); the teacher has no
resident packed images (two repacks per step); BatchNorm models raise ``NotImplementedError`` (the teacher's train-mode
forward would move the running statistics the student owns) - parameter-free and affine Instance / Group norms work;
``moddrop.enabled: true`` raises as in ``memo_tta`` while ``missing_modalities`` works (mask, then mirror); the deep-fusion
network takes views at ``group`` 1 only.  The class is its step (``_update``), the teacher's reset with the episodic one
(``_reset``), the staging of the views (``_stage``), one more per-step record and the ordinals; the per-volume loop - groups,
lanes, the captured step, the final forward - is ``EntropyMinimizationTTA``'s.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .affine import check_extents, parse_affine
from .config import expect, get_config, is_number, method_block, seed_value
from .intensity import parse_intensity
from .memo import check_square, parse_mirror_axes, parse_rot90
from .registry import register_plugin
from .tta import EntropyMinimizationTTA, modality_mask


@register_plugin("cotta_tta")
class MeanTeacherTTA(EntropyMinimizationTTA):
    """``method.cotta.mirror_axes`` (default [h, w]: 4 teacher views), ``rot90`` (default {k: []}), ``alpha`` (teacher momentum, default 0.999),
    ``restore_p`` (default 0.01), ``seed`` (default 0) and ``affine`` (default {views: 0}: ``affine.py``); the optimizer is ``training.optimizer`` exactly as for
    ``entmin_tta``."""
    fused_update = False     # one gradient for the whole span, then the teacher / restore pass over it
    block = "cotta"          # the ``method.<block>`` mapping the keys are read from (a subclass reads its own)

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, self.block)
        key = f"method.{self.block}"
        self.mirror_axes = parse_mirror_axes(get_config(s, "mirror_axes", ["h", "w"]), f"{key}.mirror_axes")
        self.rot90 = parse_rot90(get_config(s, "rot90", None), f"{key}.rot90")
        self.intensity = parse_intensity(get_config(s, "intensity", None), self.mirror_axes, f"{key}.intensity", self.rot90)
        # ({identity} + the quarter turns) x the mirror group, ``intensity.copies`` times over
        self.view_axes = self.intensity.view_axes
        # ... followed by the affine views of ``affine.views`` (code 0; with the default 0 nothing of affine.py runs)
        self.affine = parse_affine(get_config(s, "affine", None), len(self.view_axes), f"{key}.affine")
        self.coded_views = len(self.view_axes)
        if self.affine.active:
            self.view_axes = list(self.view_axes) + [0] * self.affine.views
        self.views = len(self.view_axes)
        alpha, p = get_config(s, "alpha", 0.999), get_config(s, "restore_p", 0.01)
        expect(is_number(alpha) and 0.0 <= alpha <= 1.0, f"{key}.alpha", alpha, "a teacher momentum with 0 <= alpha <= 1")
        expect(is_number(p) and 0.0 <= p < 1.0, f"{key}.restore_p", p, "a probability with 0 <= p < 1")
        self.alpha, self.restore_p, self.seed = float(alpha), float(p), seed_value(get_config(s, "seed", 0), f"{key}.seed")
        self._refuse_moddrop(f"true is not supported by {self.block}_tta (one modality mask per step for the teacher's views "
                             "and the student is not defined yet)")
        self.teacher: Optional[torch.Tensor] = None          # [replicas, n_train] fp32

    def setup(self, model, device) -> "MeanTeacherTTA":
        super().setup(model, device)          # (tells the model its views: EntropyMinimizationTTA.setup)
        rt, ar = self.rt, self.rt.arena
        self._refuse_running_stats(f"{self.block}_tta", "the teacher's train-mode forward", owner="the student")
        if self.affine.active and hasattr(rt, "stage_family"):
            raise NotImplementedError(f"method.{self.block}.affine.views = {self.affine.views}: affine views are not built for the "
                                      "deep-fusion network (its family batch is staged from the views)")
        self.teacher = torch.empty((ar.replicas, ar.n_train), dtype=torch.float32, device=ar.device)
        self._setup_ordinals()          # the restore draw's (and the intensity views') per-volume numbers
        self.reset_teacher()
        return self

    def reset_teacher(self) -> None:
        """The teacher of every replica = the source weights (where ``Arena.restore_source`` puts the student)."""
        ar = self.rt.arena
        self.teacher.copy_(ar.source[:ar.n_train].unsqueeze(0).expand_as(self.teacher))

    # ------------------------------------------------------------------ one step
    # ``restored``: the number of elements the step returned to their source values
    records = EntropyMinimizationTTA.records + (("restored", "cotta_restored", torch.int64),)

    def _update(self, x_cl: torch.Tensor, present: Optional[Sequence[bool]], xv: torch.Tensor) -> None:
        rt, ar = self.rt, self.rt.arena
        nt = ar.n_train
        B = int(x_cl.shape[0])
        sets = min(B, ar.replicas)
        # 1. targets: the teacher in the student's place, its V views (batch items [g * V, (g + 1) * V) on replica g), their
        # ensemble in the volume's frame
        saved = rt.pool.flat("cotta_saved", ar.replicas * nt).view(ar.replicas, nt)
        if nt > 0:
            saved[:sets].copy_(ar.params_all[:sets, :nt])
            ar.params_all[:sets, :nt].copy_(self.teacher[:sets])
        rt.views = self.views
        rt.pack_all()
        zv = self._forward(xv, present)
        n, d, h, w, r = zv.shape
        target = rt.pool.cl("cotta_target", B, d, h, w, r, ldc=(r + 3) // 4 * 4)
        if self.affine.active:
            inv = rt.pool.flat("affine_inv", B * self.affine.views * 12)          # uploaded by stage_views, per volume
            ops.affine_ensemble(zv, target, self.view_axes, self.coded_views, rt.affine_inv_host, inv, softmax=self.softmax)
        else:
            ops.memo_ensemble(zv, target, self.view_axes, softmax=self.softmax)
        # 2. the student on the volume alone
        if nt > 0:
            ar.params_all[:sets, :nt].copy_(saved[:sets])
        rt.views = 1
        rt.pack_all()
        logits = self._forward(x_cl, present)
        # 3. consistency loss
        dlogits = self._dlogits(logits)
        partial = rt.pool.flat("cotta_partial", ops.consistency_partials(logits), dtype=torch.float64)
        loss = rt.pool.flat("ent_loss", rt.group)
        ops.consistency_loss_items(logits, target, dlogits, partial, loss, softmax=self.softmax)
        restored = rt.pool.flat("cotta_restored", ar.replicas, dtype=torch.int64, zero=True)
        # 4. - 6. backward, the optimizer (it advances the step counter), teacher EMA + restore
        self._backward_and_step(dlogits, B, after=lambda: self._after_step(sets, restored))

    def _after_step(self, sets: int, restored: torch.Tensor) -> None:
        """The pass after the optimizer step over the first ``sets`` replicas: teacher EMA + stochastic restore."""
        rt, ar = self.rt, self.rt.arena
        nt = ar.n_train
        upd = rt.pool.flat("cotta_upd_partial", ops.cotta_update_partials(nt, sets), dtype=torch.int64)
        ops.cotta_update_sets(ar.params_all, self.teacher, ar.source, nt, sets, self.alpha, self.restore_p, self.seed,
                              ar.step, self._ordinals, upd, restored)

    # ------------------------------------------------------------------ per volume
    def _reset(self) -> None:
        super()._reset()
        self.reset_teacher()

    def _stage(self, x_cl: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
        check_square(self.view_axes, int(x_cl.shape[2]), int(x_cl.shape[3]), f"method.{self.block}.rot90")
        if self.affine.active:
            check_extents(x_cl.shape[1:4], f"method.{self.block}.affine")
        self.rt.views = self.views
        coded = self.view_axes[:self.coded_views]
        affine = self.affine if self.affine.active else None
        if self.intensity.active and self.coded_views > 1:
            present = modality_mask(int(x_cl.shape[-1]), self.missing, 0.0, None)
            xv = self.rt.stage_views(x_cl, coded, self.intensity, self._ordinals_host, present, affine=affine)
        elif affine is not None:
            xv = self.rt.stage_views(x_cl, coded, ordinals=self._ordinals_host, affine=affine)
        else:
            xv = self.rt.stage_views(x_cl, coded)
        self.rt.views = 1          # the loop runs on the volumes; the step switches to the views for the teacher
        return x_cl, (xv,)

    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None,
                     ordinals: Optional[Sequence[int]] = None) -> Dict[str, Any]:
        """As ``entmin_tta.adapt_volume``: x [B,C,D,H,W] (B <= ``method.group`` volumes), the student's final logits and the
        per-step losses, plus ``restored``: the number of restored elements per step ([steps], or [steps, B] for a group of
        B > 1 volumes).  ``ordinals``: one number per volume for the restore draw and the intensity views (default: the
        volumes served so far)."""
        if self.rt is not None:
            self._take_ordinals(int(x.shape[0]), ordinals)
        return super().adapt_volume(x, steps)
