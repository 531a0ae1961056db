"""``window_tta``: sliding-window adaptation and inference - entropy minimisation (Tent) for a volume of ANY extents.  Every
other method here runs the network on the whole staged volume, which must then have the network's own shape; this one cuts
the volume into overlapping windows of the training patch size (``method.window.roi``), runs the network on every window as
a batch item, and lets the windows meet again under an importance weight - what MONAI's ``sliding_window_inference`` and
nnU-Net do for inference, here for the adaptation step as well.

Per axis, with volume extent n, roi r and ``overlap``:

    n < r:   the axis is padded to r, (r - n) // 2 in front and the rest behind; the one window starts at -front
    else:    interval = r if n == r else max(int(r (1 - overlap)), 1);  count = ceil((n - r) / interval) + 1;
             start_i = min(i interval, n - r)

The windows are the product of the three start lists, W fastest; W_n of them, at most 32.  (This restates MONAI's
``dense_patch_slices`` / ``_get_scan_interval`` and its padding from memory; nothing here checks it against MONAI.)

The importance weight is separable: w_axis[i] = max(exp(-(i - (r - 1) / 2)^2 / (2 (sigma_scale r)^2)), floor) per axis
(``mode: constant``: 1), the 3-D weight their product - MONAI clamps the 3-D product instead; per axis keeps the normaliser
separable too: S_axis[p] = the sum of w_axis[p - s] over the starts s that cover p, and A_axis[k][i] = w_axis[i] / S_axis[start_k
+ i], 0 where start_k + i lies outside the volume (float64 on the host, rounded to fp32).  Window (kd, kh, kw) weighs its voxel
(i, j, k) with a = A_d[kd][i] A_h[kh][j] A_w[kw][k]: the a of the windows that see a voxel sum to 1, a voxel one window alone
sees has a = 1 exactly, a pad voxel a = 0.

Per volume and step, with the weights shared by the windows (W_n consecutive batch items on the volume's replica, train-mode
norms):

    L = 1/(N R) sum_w sum_voxels a_w H_bern(sigmoid z_w)        N = D H W of the unpadded volume (softmax head: 1/N, categorical)
    one step of training.optimizer with dL/dw summed over the W_n windows

Every voxel of the volume counts once, shared among the windows that see it.  The returned logits are the eval-mode forward
of all windows blended in logit space, out(v) = sum_w a_w(v) z_w(v - o_w), at the volume's extents; with ``method.steps: 0``
that is plain sliding-window inference of the source model.

With roi equal to the volume's extents (one window, a = 1) the method IS ``entmin_tta``: the parent's staging, step and final
forward, bit for bit.  With several windows the fused weight-gradient update and the head-loss epilogue stay out of the step
(their reductions cover one batch item per set), as for ``memo_tta``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .config import expect, get_config, is_integer, is_number, method_block
from .models.unet import UNetRuntime
from .registry import register_plugin
from .tta import EntropyMinimizationTTA

MAX_WINDOWS = 32
KEY = "method.window"
MODES = ("gaussian", "constant")
KEYS = ("roi", "overlap", "mode", "sigma_scale", "floor", "pad_value")


@dataclass(frozen=True)
class WindowSpec:
    roi: Tuple[int, int, int]
    overlap: float = 0.5
    mode: str = "gaussian"
    sigma_scale: float = 0.125
    floor: float = 1e-3
    pad_value: float = 0.0


@dataclass(frozen=True)
class WindowGrid:
    """The windows of one volume shape: per axis the starts, for every window its origin, and the three tables A."""
    extents: Tuple[int, int, int]
    roi: Tuple[int, int, int]
    starts: Tuple[Tuple[int, ...], Tuple[int, ...], Tuple[int, ...]]
    origins: Tuple[Tuple[int, int, int], ...]          # [W_n][3], W fastest
    tables: Tuple[np.ndarray, np.ndarray, np.ndarray]      # fp32 [count, r] per axis

    @property
    def windows(self) -> int:
        return len(self.origins)


def parse_window(value: Any, key: str = KEY) -> WindowSpec:
    """The ``window`` block: ``roi`` (three positive extents, required) and the optional ``overlap``, ``mode``, ``sigma_scale``,
    ``floor``, ``pad_value``; ``key``: the config key it came from, for the messages."""
    if value is None or not hasattr(value, "keys"):
        raise ValueError(f"{key} = {value!r}: expected a mapping with the key roi ([d, h, w]) and optionally "
                         f"{', '.join(KEYS[1:])}")
    for name in value.keys():
        if name not in KEYS:
            raise ValueError(f"{key}.{name}: unknown key (expected one of {', '.join(KEYS)})")
    roi = get_config(value, "roi", None)
    if roi is None or isinstance(roi, (str, bytes)) or not hasattr(roi, "__iter__") or hasattr(roi, "keys"):
        raise ValueError(f"{key}.roi = {roi!r}: expected three window extents [d, h, w]")
    roi = list(roi)
    expect(len(roi) == 3 and all(is_integer(r) and r >= 1 for r in roi), f"{key}.roi", roi,
           "three window extents [d, h, w], each an integer >= 1")
    overlap = get_config(value, "overlap", 0.5)
    expect(is_number(overlap) and 0.0 <= overlap < 1.0, f"{key}.overlap", overlap, "a number with 0 <= overlap < 1")
    mode = get_config(value, "mode", "gaussian")
    expect(isinstance(mode, str) and mode.lower() in MODES, f"{key}.mode", mode, "gaussian or constant")
    sigma = get_config(value, "sigma_scale", 0.125)
    expect(is_number(sigma) and sigma > 0.0, f"{key}.sigma_scale", sigma, "a finite number > 0")
    floor = get_config(value, "floor", 1e-3)
    expect(is_number(floor) and 0.0 < floor <= 1.0, f"{key}.floor", floor,
           "a number with 0 < floor <= 1 (a weight of 0 has no normaliser)")
    pad = get_config(value, "pad_value", 0.0)
    expect(is_number(pad), f"{key}.pad_value", pad, "a finite number")
    return WindowSpec((int(roi[0]), int(roi[1]), int(roi[2])), float(overlap), mode.lower(), float(sigma), float(floor), float(pad))


def window_starts(n: int, r: int, overlap: float) -> List[int]:
    """The window starts along one axis of extent ``n`` for a roi of ``r`` (the module text): ascending, the last one at
    n - r; a single negative start where the axis is padded."""
    n, r = int(n), int(r)
    if n < 1 or r < 1:
        raise ValueError(f"window_starts: extent {n}, roi {r} (both >= 1)")
    if n < r:
        return [-((r - n) // 2)]
    interval = r if n == r else max(int(r * (1.0 - float(overlap))), 1)
    count = -(-(n - r) // interval) + 1
    return [min(i * interval, n - r) for i in range(count)]


def axis_weights(r: int, mode: str = "gaussian", sigma_scale: float = 0.125, floor: float = 1e-3) -> np.ndarray:
    """The importance weight along one axis of the roi, float64 [r]."""
    if mode == "constant":
        return np.ones(int(r), dtype=np.float64)
    i = np.arange(int(r), dtype=np.float64)
    sigma = float(sigma_scale) * int(r)
    return np.maximum(np.exp(-(i - (int(r) - 1) / 2.0) ** 2 / (2.0 * sigma * sigma)), float(floor))


def axis_tables(n: int, r: int, starts: Sequence[int], weights: np.ndarray) -> np.ndarray:
    """A[k][i] = weights[i] / S[starts[k] + i] with S[p] the sum of the weights of all windows over position p, and 0 where
    starts[k] + i lies outside [0, n): float64 arithmetic, rounded to fp32 [len(starts), r]."""
    n, r = int(n), int(r)
    total = np.zeros(n, dtype=np.float64)
    pos = np.arange(r)
    for s in starts:
        p = int(s) + pos
        inside = (p >= 0) & (p < n)
        total[p[inside]] += weights[inside]
    table = np.zeros((len(starts), r), dtype=np.float64)
    for k, s in enumerate(starts):
        p = int(s) + pos
        inside = (p >= 0) & (p < n)
        table[k, inside] = weights[inside] / total[p[inside]]
    return table.astype(np.float32)


def window_grid(extents: Sequence[int], spec: WindowSpec, key: str = KEY) -> WindowGrid:
    """The windows of a volume of ``extents`` (D, H, W) under ``spec``; more than 32 of them is a ValueError naming the keys."""
    extents = tuple(int(e) for e in extents)
    if len(extents) != 3:
        raise ValueError(f"window_grid: expected the three extents (D, H, W), got {extents!r}")
    starts = tuple(tuple(window_starts(n, r, spec.overlap)) for n, r in zip(extents, spec.roi))
    count = len(starts[0]) * len(starts[1]) * len(starts[2])
    if count > MAX_WINDOWS:
        raise ValueError(f"{key}.roi = {list(spec.roi)} with {key}.overlap = {spec.overlap} cuts a volume of {extents} into "
                         f"{count} windows ({' x '.join(str(len(s)) for s in starts)}); at most {MAX_WINDOWS} run as one batch "
                         "(a larger roi or a smaller overlap gives fewer)")
    origins = tuple((sd, sh, sw) for sd in starts[0] for sh in starts[1] for sw in starts[2])
    tables = tuple(axis_tables(n, r, s, axis_weights(r, spec.mode, spec.sigma_scale, spec.floor))
                   for n, r, s in zip(extents, spec.roi, starts))
    return WindowGrid(extents, tuple(spec.roi), starts, origins, tables)


@register_plugin("window_tta")
class SlidingWindowTTA(EntropyMinimizationTTA):
    """``method.window.roi`` (required), ``overlap`` (0.5), ``mode`` (gaussian | constant), ``sigma_scale`` (0.125), ``floor``
    (1e-3) and ``pad_value`` (0.0); the optimizer is ``training.optimizer`` exactly as for ``entmin_tta``."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        self.window = parse_window(get_config(method_block(config), "window", None))
        self._refuse_moddrop("true is not supported by window_tta (the windows are cropped once per volume; a volume re-staged "
                             "under every step's modality mask would need cropping again every step)")
        self._grid: Optional[WindowGrid] = None          # the current volume's windows; None: the volume is the roi
        self._graph_sets: Dict[Any, Dict[Tuple, Any]] = {}      # a captured step carries its grid: one set of graphs per grid

    def setup(self, model, device) -> "SlidingWindowTTA":
        super().setup(model, device)
        self._graph_sets.clear()
        self.rt.check_extent(*self.window.roi)          # the network runs on the roi: its own error, before anything is staged
        self._refuse_running_stats("window_tta", "the train-mode forward of the windows")
        if self.group > 1 and not isinstance(self.rt, UNetRuntime):
            raise NotImplementedError(f"method.group = {self.group}: {type(self.rt).__name__} (the deep-fusion family) takes the "
                                      "windows of a volume at group 1 only (its encoder families spend the set index on the "
                                      "modality)")
        return self

    # ------------------------------------------------------------------ one step
    def _update(self, xv: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        grid = self._grid
        if grid is None:
            super()._update(xv, present)          # entmin_tta's own step: its loss kernel, its fused update
            return
        rt = self.rt          # (batch items [g * W_n, (g + 1) * W_n) read / write parameter replica g)
        rt.pack_all()          # every layer: the fused update is not part of this step, the arena optimizer moves all of them
        logits = self._forward(xv, present)
        dlogits = self._dlogits(logits)
        partial = rt.pool.flat("win_partial", ops.window_partials(logits), dtype=torch.float64)
        loss = rt.pool.flat("ent_loss", rt.group)
        ops.window_entropy_items(logits, dlogits, grid, rt.win_origins, rt.win_tables, partial, loss, softmax=self.softmax)
        self._backward_and_step(dlogits, int(logits.shape[0]) // grid.windows)

    # ------------------------------------------------------------------ per volume
    def _stage(self, x_cl: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
        grid = self._grid
        self._graphs = self._graph_sets.setdefault(None if grid is None else grid.extents, {})
        if grid is None:
            return super()._stage(x_cl)
        self.rt.views = grid.windows          # every launch of the loop carries W_n consecutive batch items per volume
        return self.rt.stage_windows(x_cl, self.window, grid), ()

    def _final_logits(self, x_cl: torch.Tensor, xv: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        grid = self._grid
        if grid is None:
            return super()._final_logits(x_cl, xv, present)
        rt = self.rt
        rt.pack_all()          # (the loop's own pack leaves the layers of the fused update to their update, which did not run)
        zv = self._forward(xv, present)
        n, d, h, w = int(x_cl.shape[0]), *grid.extents
        r = int(zv.shape[-1])
        logits_cl = rt.pool.cl("win_blend", n, d, h, w, r, ldc=(r + 3) // 4 * 4, zero=True)
        ops.window_blend(zv, logits_cl, grid, rt.win_origins, rt.win_tables)
        return logits_cl

    @torch.no_grad()
    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """``EntropyMinimizationTTA.adapt_volume`` for volumes [B,C,D,H,W] of any extents: the logits come back at the volume's
        extents, ``losses`` as Tent's, plus ``windows`` (W_n).  The windows of a volume share its parameter replica: a call
        takes at most ``method.group`` volumes."""
        self._check_volumes(int(x.shape[0]), "window_tta adapts ", " (the windows of a volume share its parameter replica)")
        extents = tuple(int(e) for e in x.shape[2:])
        # the grid before anything is staged: its refusal names the keys
        self._grid = None if extents == tuple(self.window.roi) else window_grid(extents, self.window)
        out = super().adapt_volume(x, steps)
        out["windows"] = 1 if self._grid is None else self._grid.windows
        return out
