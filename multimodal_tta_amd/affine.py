"""Affine (rotate / scale / shift) teacher views for ``cotta_tta`` and ``petal_tta``: the ``affine`` block both methods
read (``method.cotta.affine`` / ``method.petal.affine``), the layout of the views and the per-view matrix draws.

The views of a volume are the V_g coded views (mirror / turn codes x intensity copies, ``intensity.py``, exactly as without
the block) followed by n = ``views`` affine views: V = V_g + n, 2 <= V <= 8, item ``g * V + v`` of a batch is view v of
volume g.  An affine view carries no mirror code and no intensity draw.  The teacher's predictions take no gradient, so an
affine view needs a gather forward (``ops.affine_views`` stages it) and a gather back (``ops.affine_ensemble`` brings its
prediction into the volume's frame): no adjoint, which is why ``memo_tta`` does not read this block.

The draws, on the host in float64, fixed per volume like the intensity draws: Philox4x32-10 (``intensity.philox4x32_10``)
with the key ``(seed & 0xffffffff, seed >> 32)``.  For affine view j = 1..n of the volume with the per-volume number
``ordinal`` the counters are ``(j, 0, ordinal, 3)`` and ``(j, 1, ordinal, 3)`` - the fourth counter word 3; 0, 1 and 2 belong
to the restore, noise and intensity draws - and ``u = (word >> 8) * 2^-24``.  The four words of the first call give the
angles ``theta_D, theta_H, theta_W = rotate[k] * (2u - 1)`` degrees and the zoom ``s = 1 + scale * (2u - 1)``; words 0..2 of
the second give the shifts ``t_k = translate[k] * (2u - 1)`` voxels.  Then

    A = s * R_D(theta_D) R_H(theta_H) R_W(theta_W)      each a right-handed rotation about that axis of (d, h, w) space
    c = (extent - 1) / 2 per axis,   b = c - A c + t
    M = [A | b]                                         3 x 4, row-major: 12 numbers

M maps a VIEW voxel to the FRAME coordinate it samples (the volume turns about its centre); its inverse, taken in float64,
maps a frame voxel to the view coordinate that shows it.  Both are rounded once to fp32.  The rotation acts in voxel space:
anisotropic spacing is not accounted for (a rotation of the grid is a shear of the anatomy where the spacings differ).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Sequence, Tuple

import numpy as np

from .config import expect, get_config, is_integer, is_number, seed_value
from .intensity import MAX_VIEWS, philox4x32_10

MAX_ROTATE, MAX_SCALE, MAX_TRANSLATE = 45.0, 0.25, 16.0
KEYS = ("views", "rotate", "scale", "translate", "seed")
DRAW = 3          # the fourth counter word of the draws


@dataclass
class AffineSpec:
    """The parsed ``affine`` block."""
    views: int = 0
    rotate: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    scale: float = 0.0
    translate: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    seed: int = 0

    @property
    def active(self) -> bool:
        """False: nothing of this module runs and the views are the coded views alone."""
        return self.views > 0


def _triple(value: Any, key: str, limit: float, unit: str) -> Tuple[float, float, float]:
    if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__") or hasattr(value, "keys") or len(list(value)) != 3:
        raise ValueError(f"{key} = {value!r}: expected three magnitudes (D, H, W axis), each 0 .. {limit:g} {unit}")
    out = []
    for v in value:
        if not (is_number(v) and 0.0 <= v <= limit):
            raise ValueError(f"{key} = {list(value)!r}: {v!r} is no magnitude with 0 <= value <= {limit:g} {unit}")
        out.append(float(v))
    return out[0], out[1], out[2]


def parse_affine(value: Any, coded_views: int, key: str = "method.cotta.affine") -> AffineSpec:
    """The ``affine`` block (a mapping, or None for the defaults) of a method with ``coded_views`` mirror / turn / intensity
    views; ``key``: the config key it came from, for the messages."""
    value = {} if value is None else value
    if not hasattr(value, "keys"):
        raise ValueError(f"{key} = {value!r}: expected a mapping with the keys {', '.join(KEYS)}")
    for k in value.keys():
        if k not in KEYS:
            raise ValueError(f"{key}.{k}: unknown key (expected one of {', '.join(KEYS)})")
    views = get_config(value, "views", 0)
    expect(is_integer(views) and 0 <= views < MAX_VIEWS, f"{key}.views", views,
           f"a number of affine views with 0 <= views <= {MAX_VIEWS - 1}")
    rotate = _triple(get_config(value, "rotate", [0.0, 0.0, 0.0]), f"{key}.rotate", MAX_ROTATE, "degrees")
    translate = _triple(get_config(value, "translate", [0.0, 0.0, 0.0]), f"{key}.translate", MAX_TRANSLATE, "voxels")
    scale = get_config(value, "scale", 0.0)
    expect(is_number(scale) and 0.0 <= scale <= MAX_SCALE, f"{key}.scale", scale, f"a magnitude with 0 <= scale <= {MAX_SCALE:g}")
    seed = seed_value(get_config(value, "seed", 0), f"{key}.seed")
    spec = AffineSpec(views=int(views), rotate=rotate, scale=float(scale), translate=translate, seed=seed)
    if spec.views > 0 and not (any(rotate) or any(translate) or spec.scale > 0.0):
        raise ValueError(f"{key}.views = {views} with rotate, scale and translate all 0: the affine views would be copies of "
                         "the volume")
    if spec.views > 0 and coded_views + spec.views > MAX_VIEWS:
        raise ValueError(f"{key}.views = {views} with {coded_views} mirrored / turned / intensity views: V = "
                         f"{coded_views + spec.views} views, at most {MAX_VIEWS}")
    return spec


def check_extents(extents: Sequence[int], key: str = "method.cotta.affine") -> None:
    """An affine view needs two voxels along every axis: raise before anything is staged or launched."""
    if any(int(e) < 2 for e in extents):
        raise ValueError(f"{key}.views: an affine view needs every extent of the volume >= 2, the volume is "
                         f"{' x '.join(str(int(e)) for e in extents)} (D x H x W)")


def rotation(axis: int, degrees: float) -> np.ndarray:
    """The right-handed rotation by ``degrees`` about axis 0 (D), 1 (H) or 2 (W) of (d, h, w) space, float64 3 x 3."""
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def view_matrix(angles: Sequence[float], zoom: float, shift: Sequence[float], extents: Sequence[int]) -> np.ndarray:
    """M = [A | b], float64 3 x 4: A = zoom * R_D R_H R_W of the ``angles`` (degrees), b = c - A c + shift with c the centre
    of a volume of ``extents`` - a view voxel -> the frame coordinate it samples."""
    a = float(zoom) * (rotation(0, angles[0]) @ rotation(1, angles[1]) @ rotation(2, angles[2]))
    c = (np.asarray(extents, dtype=np.float64) - 1.0) / 2.0
    return np.concatenate([a, (c - a @ c + np.asarray(shift, dtype=np.float64)).reshape(3, 1)], axis=1)


def inverse(m: np.ndarray) -> np.ndarray:
    """The inverse map of M = [A | b] in float64: [A^-1 | -A^-1 b]."""
    ai = np.linalg.inv(m[:, :3])
    return np.concatenate([ai, (-ai @ m[:, 3]).reshape(3, 1)], axis=1)


def view_draws(cfg: AffineSpec, ordinals: Sequence[int]) -> np.ndarray:
    """The draws of every (volume, affine view): float64 [B, n, 7] = (theta_D, theta_H, theta_W, s, t_D, t_H, t_W)."""
    B, n = len(ordinals), cfg.views
    ords = np.array([int(o) for o in ordinals], dtype=np.uint64).reshape(B, 1)
    if np.any(ords >> np.uint64(32)):
        raise ValueError(f"ordinals = {list(ordinals)!r}: expected 0 <= ordinal < 2^32")
    j = np.arange(1, n + 1, dtype=np.uint64).reshape(1, n)
    key = (cfg.seed & 0xFFFFFFFF, cfg.seed >> 32)
    first, second = philox4x32_10((j, 0, ords, DRAW), key), philox4x32_10((j, 1, ords, DRAW), key)
    u = [(w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 for w in (*first, *second[:3])]          # [B, n] each
    out = np.empty((B, n, 7), dtype=np.float64)
    for k in range(3):
        out[..., k] = cfg.rotate[k] * (2.0 * u[k] - 1.0)
        out[..., 4 + k] = cfg.translate[k] * (2.0 * u[4 + k] - 1.0)
    out[..., 3] = 1.0 + cfg.scale * (2.0 * u[3] - 1.0)
    return out


def view_matrices(cfg: AffineSpec, ordinals: Sequence[int], extents: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """What ``ops.affine_views`` and ``ops.affine_ensemble`` read: float32 [B, n, 12] each, the matrices M of every
    (volume, affine view) of volumes of ``extents`` (D, H, W) and their inverses; B = len(ordinals)."""
    check_extents(extents)
    draws = view_draws(cfg, ordinals)
    B, n = draws.shape[:2]
    m, inv = np.empty((B, n, 12), dtype=np.float64), np.empty((B, n, 12), dtype=np.float64)
    for b in range(B):
        for j in range(n):
            d = draws[b, j]
            mat = view_matrix(d[:3], d[3], d[4:], extents)
            m[b, j], inv[b, j] = mat.reshape(12), inverse(mat).reshape(12)
    return np.ascontiguousarray(m.astype(np.float32)), np.ascontiguousarray(inv.astype(np.float32))
