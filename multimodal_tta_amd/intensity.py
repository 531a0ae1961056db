"""Intensity-augmented views for ``memo_tta`` and ``cotta_tta``: the ``intensity`` block both methods read
(``method.memo.intensity`` / ``method.cotta.intensity``), the layout of the views, and the per-view parameter draws.

The views of a volume are the mirror group of ``mirror_axes`` times ``copies`` intensity copies: V = 2^k * copies <= 8,
view v has the mirror mask ``view_masks(mirror_axes)[v % 2^k]`` and the copy index ``v // 2^k``.  With the quarter turns of
the methods' ``rot90`` block the geometric views are ({identity} + the turns) x the mirror group, G of them, and view v has
the code ``view_layout(...)[v % G]`` and the copy index ``v // G``.  View 0 is the volume
itself; every view v >= 1 takes its own draw (g, a, b) and, per voxel, its own noise.  On a value, in this order:

    gamma      x <- ((x - lo) / (hi - lo))^g * (hi - lo) + lo     g = exp(gamma * (2u - 1)); lo / hi: the channel's range
    scale      x <- x * a                                          a = 1 + scale * (2u - 1)   (MONAI RandScaleIntensity)
    shift      x <- x + b                                          b = shift * (2u - 1)       (MONAI RandShiftIntensity)
    noise      x <- x + noise_std * n                              n ~ N(0, 1) per voxel and channel

The draws: Philox4x32-10 with the key ``(seed & 0xffffffff, seed >> 32)``.  The parameters of view v,
channel c of the volume with the per-volume number ``ordinal`` come from the counter ``(c, v, ordinal, 2)`` - c = 0 for every
channel unless ``per_channel`` - as ``u_j = (word_j >> 8) * 2^-24``, j = 0, 1, 2 for g, a, b, computed in float64 and rounded
once to fp32.  The noise is drawn on the device (``mmtta_augment_views``, counter word 1).  CoTTA's restore draw uses the
fourth counter word 0: the three never meet.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, List, Optional, Sequence

import numpy as np

from .config import expect, get_config, is_integer, is_number, seed_value

MAX_VIEWS = 8
COPIES = (1, 2, 4, 8)
MAGNITUDES = ("scale", "shift", "gamma", "noise_std")
IDENTITY = (1.0, 1.0, 0.0, 0.0)          # a table row (g, a, b, sigma) that moves the bits

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter: Sequence[Any], key: Sequence[int]) -> List[np.ndarray]:
    """Philox4x32-10 (Salmon et al., SC 2011; Random123's generator).  counter: four uint32 arrays (or scalars), key: two
    -> the four output words as uint32 arrays of the broadcast shape."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def view_layout(mirror_axes: Sequence[str], copies: int = 1, key: str = "intensity", rot90: Sequence[int] = ()) -> List[int]:
    """The code of every view: the masks of the mirror group - with quarter turns ``rot90`` (counts out of 1, 2, 3 in the
    (H, W) plane): ({identity} + the turns, in the listed order) x the mirror group, mirror index fastest - ``copies`` times
    over.  A code is a mirror mask (bit 0 = W, 1 = H, 2 = D) plus bit 4 = H and W transposed first."""
    from .memo import ROT90_CODES, rotated_code, view_masks
    base = view_masks(mirror_axes)
    expect(is_integer(copies) and copies in COPIES, f"{key}.copies", copies, "1, 2, 4 or 8")
    if len(base) * copies > MAX_VIEWS:
        raise ValueError(f"{key}.copies = {copies} with {len(base)} mirrored views: V = {len(base) * copies} views, at most "
                         f"{MAX_VIEWS}")
    turns = list(rot90)
    if not turns:
        return list(base) * copies
    rkey = key.rsplit(".", 1)[0] + ".rot90" if "." in key else "rot90"
    views = len(base) * (1 + len(turns)) * copies
    if views not in (1, 2, 4, 8):
        raise ValueError(f"{rkey}.k = {turns!r} with {len(base)} mirrored views and {copies} copies: V = {len(base)} * "
                         f"{1 + len(turns)} * {copies} = {views} views, expected 1, 2, 4 or 8 (one turn or all three)")
    codes: List[int] = []
    for t in [0] + turns:
        for m in base:
            code = rotated_code(ROT90_CODES[t] if t else 0, m)
            if code in codes:
                raise ValueError(f"{rkey}.k = {turns!r} with mirror_axes = {list(mirror_axes)!r}: views {codes.index(code)} and "
                                 f"{len(codes)} are the same view (code {code}) in every copy")
            codes.append(code)
    return codes * copies


@dataclass
class IntensitySpec:
    """The parsed ``intensity`` block, with the views it belongs to."""
    copies: int = 1
    scale: float = 0.0
    shift: float = 0.0
    gamma: float = 0.0
    noise_std: float = 0.0
    per_channel: bool = False
    seed: int = 0
    view_axes: List[int] = field(default_factory=lambda: [0])

    @property
    def views(self) -> int:
        return len(self.view_axes)

    @property
    def active(self) -> bool:
        """False: the views are the mirror group alone and nothing of this module runs."""
        return any(getattr(self, k) > 0.0 for k in MAGNITUDES)


def parse_intensity(value: Any, mirror_axes: Sequence[str], key: str = "method.memo.intensity",
                    rot90: Sequence[int] = ()) -> IntensitySpec:
    """The ``intensity`` block (a mapping, or None for the defaults) of a method whose views mirror ``mirror_axes`` and
    turn by the quarter turns ``rot90`` (``memo.parse_rot90``); ``key``: the config key it came from, for the messages."""
    value = {} if value is None else value
    if not hasattr(value, "keys"):
        raise ValueError(f"{key} = {value!r}: expected a mapping with the keys copies, scale, shift, gamma, noise_std, "
                         "per_channel, seed")
    known = ("copies", *MAGNITUDES, "per_channel", "seed")
    for k in value.keys():
        if k not in known:
            raise ValueError(f"{key}.{k}: unknown key (expected one of {', '.join(known)})")
    copies = get_config(value, "copies", 1)
    view_axes = view_layout(mirror_axes, copies, key, rot90)
    mags = {}
    for k in MAGNITUDES:
        v = get_config(value, k, 0.0)
        expect(is_number(v) and v >= 0.0, f"{key}.{k}", v, "a finite magnitude >= 0")
        mags[k] = float(v)
    if mags["scale"] >= 1.0:
        raise ValueError(f"{key}.scale = {mags['scale']!r}: expected scale < 1 (the factor 1 + scale * (2u - 1) stays positive)")
    per_channel = get_config(value, "per_channel", False)
    expect(isinstance(per_channel, bool), f"{key}.per_channel", per_channel, "true or false")
    seed = seed_value(get_config(value, "seed", 0), f"{key}.seed")
    spec = IntensitySpec(copies=copies, per_channel=per_channel, seed=seed, view_axes=view_axes, **mags)
    if copies > 1 and not spec.active:
        raise ValueError(f"{key}.copies = {copies} with scale, shift, gamma and noise_std all 0: the copies of a view would be "
                         "identical")
    return spec


def view_parameters(cfg: IntensitySpec, ordinals: Sequence[int], channels: int,
                    present: Optional[Sequence[bool]] = None) -> np.ndarray:
    """The table ``mmtta_augment_views`` reads: float32 [B, V, C, 4] with the row (g, a, b, sigma) of every (volume, view,
    channel); B = len(ordinals).  View 0 and the channels ``present`` marks absent carry the identity row (1, 1, 0, 0)."""
    B, V, C = len(ordinals), cfg.views, int(channels)
    if present is not None and len(present) != C:
        raise ValueError(f"modality mask has {len(present)} entries for {C} channels")
    ords = np.array([int(o) for o in ordinals], dtype=np.uint64).reshape(B, 1, 1)
    if np.any(ords >> np.uint64(32)):
        raise ValueError(f"ordinals = {list(ordinals)!r}: expected 0 <= ordinal < 2^32")
    v = np.arange(V, dtype=np.uint64).reshape(1, V, 1)
    c = np.arange(C, dtype=np.uint64).reshape(1, 1, C) * np.uint64(1 if cfg.per_channel else 0)
    words = philox4x32_10((c, v, ords, 2), (cfg.seed & 0xFFFFFFFF, cfg.seed >> 32))
    u = [(w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 for w in words[:3]]          # [B, V, C] each
    table = np.empty((B, V, C, 4), dtype=np.float64)
    table[..., 0] = np.exp(cfg.gamma * (2.0 * u[0] - 1.0))
    table[..., 1] = 1.0 + cfg.scale * (2.0 * u[1] - 1.0)
    table[..., 2] = cfg.shift * (2.0 * u[2] - 1.0) + 0.0          # (+ 0: a zero magnitude gives +0, never -0)
    table[..., 3] = cfg.noise_std
    table[:, 0] = IDENTITY
    if present is not None:
        table[:, :, [i for i in range(C) if not present[i]]] = IDENTITY
    return np.ascontiguousarray(table.astype(np.float32))
