"""``deyo_tta``: DeYO (Lee et al., ICLR 2024, "Entropy is not Enough for Test-Time Adaptation") on the native engine, next
to ``entmin_tta`` (Tent), ``sar_tta`` (SAR), ``memo_tta`` (MEMO), ``cotta_tta`` (CoTTA) and ``eata_tta`` (EATA) - the method
of the SAR / EATA line that does not trust entropy alone: a confident element is adapted on only if it stops being confident
once the object's shape is destroyed, that is, once the patches of the input are shuffled.  An element whose confidence
survives the shuffle rests on local texture - for multi-centre MRI / PET-CT volumes the scanner's intensity, the shift itself.

Per volume and step (each volume of a group on its own weight replica ``w``; K = 2 for the sigmoid head's (voxel, region)
elements and K = R for the softmax head's voxels):

    x'   = shuffle(x; grid, perm)                      (staged once per volume, fixed for all its steps)
    z'   = f(x'; w)                                    (train-mode norms, no gradient; copied out of the logits buffer)
    z    = f(x ; w)                                    (the forward whose activations the backward uses)
    z''  = unshuffle(z')                               (z''(v) = z' at the place where the content of voxel v went)
    H    = the entropy element of z
    PLPD = p(z)[y^] - p(z'')[y^]                       (y^ the hard prediction of z: 1[z >= 0], or the first arg max)
    keep1 = H < e_margin ln K;  keep = keep1 and PLPD > plpd_threshold
    a    = exp(e_margin0 ln K - H) + exp(PLPD)         (a carries no gradient)
    L    = sum over keep of a H / |keep|               (NaN and a zero gradient when nothing is kept, as SAR / EATA)
    one step of training.optimizer with dL/dw

The shuffle: ``method.deyo.patches: [gd, gh, gw]`` patches per axis (each 1 .. 16, P = gd gh gw >= 2, every axis extent
divisible by its count); destination slot j (row-major over the grid) holds source patch perm[j].  The permutation is drawn
on the host per volume from the volume's ordinal (``draw_permutation``): Fisher-Yates from the identity with Philox4x32-10
under the key ``(seed & 0xffffffff, seed >> 32)`` - for j = P-1 .. 1, u = word 0 at the counter ``(j, 0, ordinal, 3)``,
k = (u (j + 1)) >> 32, swap perm[j] and perm[k].  Counter word 3 = 3 keeps the draw apart from CoTTA's restore (0), the
noise (1) and the parameters (2) of the intensity views.  The ordinal, not the replica slot, enters the draw: a group of
volumes equals the same volumes served one at a time.

Where this differs from the paper: the elements are voxels (or voxel x region pairs), not images; the margins are fractions
of ln K; the permutation is fixed per volume, not re-drawn per step; the patches form a 3-D grid of the volume as it is,
without the paper's resize (extents the grid does not divide are refused); the paper's pixel-shuffle and occlusion variants
and the switches of its reweighting ablation are not built; the step count is ``method.steps``.

Scope: two forwards and one backward per step, the weights packed once in front of both (they do not move in between, so the
fused weight-gradient update stays on); models with running statistics raise ``NotImplementedError`` (the extra train-mode
forward would move them); ``moddrop.enabled: true`` raises (the shuffled copy is staged once per volume) while
``missing_modalities`` works (the mask applies to both forwards).  The class is its step (``_update``), the staging of the
shuffled copy (``_stage``), two more per-step records and the ordinals; the per-volume loop - groups, lanes, the captured
step, the final forward - is ``EntropyMinimizationTTA``'s.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .config import expect, get_config, is_integer, is_number, method_block, seed_value
from .intensity import philox4x32_10
from .registry import register_plugin
from .tta import EntropyMinimizationTTA

DRAW_STREAM = 3          # counter word 3 of the permutation draw (0: cotta_tta's restore, 1 / 2: the intensity views)
MAX_PATCHES_PER_AXIS = 16


def parse_patches(value: Any, key: str = "method.deyo.patches") -> List[int]:
    """``[gd, gh, gw]``: three patch counts of 1 .. 16 with a product of at least 2."""
    if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__") or hasattr(value, "keys"):
        raise ValueError(f"{key} = {value!r}: expected three patch counts [gd, gh, gw]")
    grid = list(value)
    expect(len(grid) == 3 and all(is_integer(g) and 1 <= g <= MAX_PATCHES_PER_AXIS for g in grid), key, grid,
           f"three integers of 1 .. {MAX_PATCHES_PER_AXIS}")
    if grid[0] * grid[1] * grid[2] < 2:
        raise ValueError(f"{key} = {grid!r}: one patch cannot be shuffled (P = gd * gh * gw >= 2)")
    return [int(g) for g in grid]


def draw_permutation(seed: int, ordinal: int, patches: int) -> List[int]:
    """The patch permutation of the volume ``ordinal``: Fisher-Yates from the identity, j = P-1 .. 1 swapped with
    k = (u (j + 1)) >> 32 for u = word 0 of Philox4x32-10 at the counter (j, 0, ordinal, 3) under the seed's key."""
    perm = list(range(int(patches)))
    if patches < 2:
        return perm
    js = list(range(patches - 1, 0, -1))
    words = philox4x32_10((js, 0, int(ordinal), DRAW_STREAM), (seed & 0xFFFFFFFF, seed >> 32))[0]
    for j, u in zip(js, words.tolist()):
        k = (int(u) * (j + 1)) >> 32
        perm[j], perm[k] = perm[k], perm[j]
    return perm


def _positive(value: Any, key: str) -> float:
    expect(is_number(value) and value > 0.0, key, value, "a finite positive fraction of ln K")
    return float(value)


@register_plugin("deyo_tta")
class ShuffleFilteredTTA(EntropyMinimizationTTA):
    """``method.deyo.e_margin`` (fraction of ln K, default 0.5), ``e_margin0`` (0.4), ``plpd_threshold`` (0.2), ``patches``
    (default [4, 4, 4]) and ``seed`` (default 0); the optimizer is ``training.optimizer`` exactly as for ``entmin_tta``."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "deyo")
        self.e_margin = _positive(get_config(s, "e_margin", 0.5), "method.deyo.e_margin")
        self.e_margin0 = _positive(get_config(s, "e_margin0", 0.4), "method.deyo.e_margin0")
        thr = get_config(s, "plpd_threshold", 0.2)
        expect(is_number(thr) and -1.0 <= thr < 1.0, "method.deyo.plpd_threshold", thr,
               "a finite probability difference with -1 <= threshold < 1")
        self.plpd_threshold, self.seed = float(thr), seed_value(get_config(s, "seed", 0), "method.deyo.seed")
        self.patches = parse_patches(get_config(s, "patches", [4, 4, 4]))
        self._refuse_moddrop("true is not supported by deyo_tta (the shuffled copy of the volume is staged once per volume, "
                             "not once per modality mask)")
        self._table: Optional[torch.Tensor] = None          # device int32 [B, 2, P] of the volumes being adapted

    def margin(self, regions: int, fraction: Optional[float] = None) -> float:
        """A margin in nats: ``fraction`` (default e_margin) * ln K."""
        f = self.e_margin if fraction is None else fraction
        return f * math.log(float(regions) if self.softmax else 2.0)

    def setup(self, model, device) -> "ShuffleFilteredTTA":
        super().setup(model, device)
        self._refuse_running_stats("deyo_tta", "the shuffled volume's train-mode forward")
        self._setup_ordinals()          # the permutation draw's per-volume numbers
        return self

    # ------------------------------------------------------------------ one step
    # ``losses`` holds L, ``kept`` the elements in the loss, ``kept_entropy`` those below the entropy margin
    records = EntropyMinimizationTTA.records + (("kept", "deyo_kept", torch.int64),
                                                ("kept_entropy", "deyo_kept_entropy", torch.int64))

    def _update(self, x: torch.Tensor, present: Optional[Sequence[bool]], x_shuf: torch.Tensor) -> None:
        rt = self.rt
        rt.pack_all(fused_current=True)          # once, in front of both forwards: the weights do not move in between
        # 1. the shuffled volume; its logits leave the pool's logits buffer, which the second forward writes again
        key = getattr(rt, "family_key", None)
        if key is not None:
            rt.family_key = "deyo_xm_shuf"
        try:
            zs = self._forward(x_shuf, present)
        finally:
            if key is not None:
                rt.family_key = key
        n, d, h, w, r = zs.shape
        logits_shuf = rt.pool.cl("deyo_logits_shuf", n, d, h, w, r, ldc=(r + 3) // 4 * 4, zero=True)
        ops.lincomb([zs], [1.0], logits_shuf)
        # 2. the volume itself: the activations the backward reads
        logits = self._forward(x, present)
        dlogits = self._dlogits(logits)
        slots = rt.group
        elems = n * d * h * w * (1 if self.softmax else r)
        partial = rt.pool.flat("deyo_partial", ops.deyo_partials(logits), dtype=torch.float64)
        loss = rt.pool.flat("ent_loss", slots)
        kept = rt.pool.flat("deyo_kept", slots, dtype=torch.int64)
        kept_entropy = rt.pool.flat("deyo_kept_entropy", slots, dtype=torch.int64)
        keep = rt.pool.flat("deyo_keep", elems, dtype=torch.uint8)
        ops.deyo_loss_items(logits, logits_shuf, dlogits, self.patches, self._table, self.margin(r),
                            self.margin(r, self.e_margin0), self.plpd_threshold, keep, partial, loss, kept, kept_entropy,
                            softmax=self.softmax)
        self._backward_and_step(dlogits, n, fused=True)

    # ------------------------------------------------------------------ per volume
    def _stage(self, x_cl: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
        rt = self.rt
        n, d, h, w, c = x_cl.shape
        for extent, count, axis in zip((d, h, w), self.patches, "DHW"):
            if extent % count:
                raise ValueError(f"method.deyo.patches = {self.patches!r}: {count} patches do not divide the volume's {axis} "
                                 f"extent {extent} (the volume is not resampled)")
        patches = self.patches[0] * self.patches[1] * self.patches[2]
        if len(self._ordinals_host) != n:
            raise ValueError(f"deyo_tta: {n} volumes with the ordinals {self._ordinals_host!r} (one per volume)")
        host = ops.patch_table([draw_permutation(self.seed, o, patches) for o in self._ordinals_host])
        # a buffer with a stable address, filled outside the captured step
        table = rt.pool.flat("deyo_table", rt.group * 2 * patches, dtype=torch.int32, zero=True)
        self._table = table[:n * 2 * patches]
        self._table.copy_(host.reshape(-1))
        x_shuf = rt.pool.cl("deyo_x_shuf", n, d, h, w, c, ldc=(c + 3) // 4 * 4, zero=True, dtype=x_cl.dtype)
        ops.patch_shuffle(x_cl, x_shuf, self.patches, self._table)
        if hasattr(rt, "stage_family"):
            rt.stage_family(x_shuf, "deyo_xm_shuf")          # the family batch of the shuffled volume (deep fusion)
        return x_cl, (x_shuf,)

    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None,
                     ordinals: Optional[Sequence[int]] = None) -> Dict[str, Any]:
        """As ``entmin_tta.adapt_volume``, plus ``kept`` and ``kept_entropy`` per step ([steps], or [steps, B] for a group).
        ``ordinals``: one number per volume for the permutation draw (default: the volumes served so far), as for
        ``memo_tta``.  As for ``sar_tta``, a runtime without parameter sets (``group`` 1) takes one volume per call."""
        if self.rt is not None:
            self._take_ordinals(int(x.shape[0]), ordinals)
        return super().adapt_volume(x, steps)
