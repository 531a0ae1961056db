"""``biasfield_tta``: entropy minimisation that adapts a smooth GAIN FIELD in front of the network.  The shift MRI volumes of
another scanner carry is spatial as well as global: the receive-coil intensity non-uniformity (the "bias field") is a smooth
multiplicative field that differs per sequence and per scanner - the reason N4 (Tustison et al., IEEE TMI 2010) sits in front
of every BraTS-style pipeline.  A residual or differently corrected field at the target centre is a covariate shift that
``innorm_tta``'s global (s, b, g) cannot express and that the random intensity views of MEMO and CoTTA do not average away.

Every volume of a group carries theta[c, k] per modality c and basis term k, 0 at the start and reset with the weights:

    F_c(z, y, x) = sum_k theta_ck phi_k(z, y, x)           the log-field
    x'_c         = (x_c - a_c) exp(F_c) + a_c              a_c: the intensity the field leaves fixed

phi_(a,b,c) = P_a(t_z) P_b(t_y) P_c(t_x): Legendre polynomials of the normalised voxel-centre coordinates t_i = (2 i + 1) / n - 1
of the STAGED volume, total degree <= ``order`` <= 3, ordered by (a + b + c, a, b, c): 1 / 4 / 10 / 20 terms.  Term 0 is the
constant - the global log-gain, ``innorm_tta``'s s.  ``anchor: min`` takes a_c = the channel's minimum over the raw volume (the
image's zero level in a z-scored MRI whose background is part of the volume: background voxels come through bit for bit),
``anchor: zero`` a_c = 0.

One step is ``innorm_tta``'s with another map: x' is written from the raw volume (``ops.bias_field_apply``), the parent's
sequence runs on x', theta takes one Adam step on dL/dtheta + 2 l2 theta (k >= 1) and is clamped (``ops.bias_field_grad``: the
first level's input gradient reduced against the basis, K numbers per modality, never stored as a volume).  With
``method.params: []`` the network is the source model bit for bit and only the field adapts.

Where this differs from N4 and from Karani et al.: the basis is polynomial, not B-spline; the field is driven by the network's
entropy, not by histogram sharpening or a denoising prior; the coordinates are those of the staged volume, not of the scanner,
and spacing is ignored.  It sits on top of Tent alone, on the ``unet`` model, and not together with modality dropout.

``lr: 0`` takes the parent's step untouched - nothing new is launched - and is ``entmin_tta`` bit for bit.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .config import expect, get_config, is_integer, is_number, method_block
from .innorm import InputMapTTA
from .registry import register_plugin

MAX_ORDER, MAX_EXTENT = 3, 512
MAX_BOUND_GAIN, MAX_BOUND_FIELD = 4.0, 1.0
ANCHORS = ("min", "zero")
DEFAULTS = {"lr": 1e-2, "order": 2, "anchor": "min", "l2": 0.0, "bound": {"gain": 0.7, "field": 0.2}}


# ----------------------------------------------------------------------------- the basis
def field_terms(order: int) -> List[Tuple[int, int, int]]:
    """The exponents (a, b, c) of phi = P_a(t_z) P_b(t_y) P_c(t_x) with a + b + c <= order, by (a + b + c, a, b, c) ascending:
    (order + 1)(order + 2)(order + 3) / 6 terms, term 0 the constant."""
    expect(is_integer(order) and 0 <= order <= MAX_ORDER, "order", order, f"an int in 0 .. {MAX_ORDER}")
    terms = [(a, b, c) for a in range(order + 1) for b in range(order + 1 - a) for c in range(order + 1 - a - b)]
    return sorted(terms, key=lambda t: (sum(t), t))


def legendre_tables64(n: int) -> np.ndarray:
    """T[a][i] = P_a(t_i), a = 0 .. 3, at the voxel centres t_i = (2 i + 1) / n - 1 of an axis of n voxels (n = 1: t = 0),
    float64 [4, n]."""
    if n < 1:
        raise ValueError(f"an axis of {n} voxels")
    t = (2.0 * np.arange(n, dtype=np.float64) + 1.0) / n - 1.0
    return np.stack([np.ones_like(t), t, (3.0 * t * t - 1.0) / 2.0, (5.0 * t * t * t - 3.0 * t) / 2.0])


def legendre_tables(extents: Sequence[int]) -> Tuple[np.ndarray, ...]:
    """The three tables the kernels read, one per axis of ``extents`` = (D, H, W): ``legendre_tables64`` rounded once to fp32."""
    return tuple(legendre_tables64(int(n)).astype(np.float32) for n in extents)


def evaluate_field(coeff, extents: Sequence[int]) -> np.ndarray:
    """exp(F) of the coefficients ``coeff`` [..., K] (K = 1, 4, 10 or 20: the order follows) on a grid of ``extents`` = (D, H, W)
    -> float64 [..., D, H, W], from the fp32 tables the kernels read.  Host-side: for looking at a field or saving it."""
    coeff = np.asarray(coeff.detach().cpu() if isinstance(coeff, torch.Tensor) else coeff, dtype=np.float64)
    counts = [len(field_terms(o)) for o in range(MAX_ORDER + 1)]
    if coeff.shape[-1] not in counts:
        raise ValueError(f"coeff has {coeff.shape[-1]} terms: expected one of {counts}")
    terms = field_terms(counts.index(coeff.shape[-1]))
    td, th, tw = (t.astype(np.float64) for t in legendre_tables(extents))
    F = np.zeros(coeff.shape[:-1] + tuple(int(n) for n in extents))
    for k, (a, b, c) in enumerate(terms):
        F += coeff[..., k, None, None, None] * (td[a][:, None, None] * th[b][None, :, None] * tw[c][None, None, :])
    return np.exp(F)


# ----------------------------------------------------------------------------- config
def parse_config(block: Any) -> Dict[str, Any]:
    """``method.biasfield`` -> {lr, order, anchor, l2, bound_gain, bound_field}; a missing key takes its default, an unknown
    key, a wrong type or a value out of range raises ValueError naming the key."""
    block = {} if block is None else block
    if not hasattr(block, "keys"):
        raise ValueError(f"method.biasfield = {block!r}: expected a mapping")
    for key in block.keys():
        if key not in DEFAULTS:
            raise ValueError(f"method.biasfield.{key} : unknown key (known: {', '.join(DEFAULTS)})")
    bound = get_config(block, "bound", None)
    bound = {} if bound is None else bound
    if not hasattr(bound, "keys"):
        raise ValueError(f"method.biasfield.bound = {bound!r}: expected a mapping")
    for key in bound.keys():
        if key not in DEFAULTS["bound"]:
            raise ValueError(f"method.biasfield.bound.{key} : unknown key (known: {', '.join(DEFAULTS['bound'])})")
    lr, order = get_config(block, "lr", DEFAULTS["lr"]), get_config(block, "order", DEFAULTS["order"])
    anchor, l2 = get_config(block, "anchor", DEFAULTS["anchor"]), get_config(block, "l2", DEFAULTS["l2"])
    expect(is_number(lr) and lr >= 0.0, "method.biasfield.lr", lr, "a finite number >= 0 (0: entmin_tta)")
    expect(is_integer(order) and 0 <= order <= MAX_ORDER, "method.biasfield.order", order, f"an int in 0 .. {MAX_ORDER}")
    expect(isinstance(anchor, str) and anchor in ANCHORS, "method.biasfield.anchor", anchor, f"one of {' | '.join(ANCHORS)}")
    expect(is_number(l2) and l2 >= 0.0, "method.biasfield.l2", l2, "a finite number >= 0")
    out = {"lr": float(lr), "order": order, "anchor": anchor, "l2": float(l2)}
    for key, top in (("gain", MAX_BOUND_GAIN), ("field", MAX_BOUND_FIELD)):
        val = get_config(bound, key, DEFAULTS["bound"][key])
        expect(is_number(val) and 0.0 < val <= top, f"method.biasfield.bound.{key}", val, f"a finite number in (0, {top:g}]")
        out[f"bound_{key}"] = float(val)
    return out


# ----------------------------------------------------------------------------- the plugin
@register_plugin("biasfield_tta")
class BiasFieldTTA(InputMapTTA):
    """``method.biasfield.lr`` (finite, >= 0, default 1e-2; 0: ``entmin_tta``), ``order`` (0 | 1 | 2 | 3, default 2), ``anchor``
    (min | zero, default min), ``l2`` (>= 0, default 0: a penalty l2 |theta_k|^2 on the non-constant coefficients),
    ``bound.gain`` ((0, 4], default 0.7: the clamp of the constant coefficient) and ``bound.field`` ((0, 1], default 0.2: of
    every other one).  theta's optimizer is Adam with torch's default betas and eps and no decay, whatever
    ``training.optimizer`` is.  Everything else is ``entmin_tta``'s, with one limit: every volume has its own theta, so a call
    takes at most ``method.group`` volumes.  Nobody has measured a Dice with the defaults."""
    plugin, prefix, row, record = "biasfield_tta", "biasfield", ops.BIAS_ROW, "field_grad"

    def __init__(self, config: Any = None):
        super().__init__(config)
        c = parse_config(get_config(method_block(config), "biasfield", None))          # (a disabled path still validates its block)
        self.lr, self.order, self.anchor, self.l2 = c["lr"], c["order"], c["anchor"], c["l2"]
        self.bounds = (c["bound_gain"], c["bound_field"])
        self.terms = field_terms(self.order)
        self._extents: Optional[Tuple[int, int, int]] = None
        self._filled: set = set()

    def setup(self, model, device) -> "BiasFieldTTA":
        self._filled = set()          # (a new runtime has a new pool)
        return super().setup(model, device)

    # ------------------------------------------------------------------ the tables
    def _field_tables(self) -> Tuple[torch.Tensor, ...]:
        """The three Legendre tables of the staged extents, in pool buffers (fixed addresses: the captured step reads them);
        built on the host in float64, rounded once and copied the first time an extent is seen."""
        rt = self.rt
        bufs = tuple(rt.pool.flat(f"biasfield_table_{n}", 4 * n).view(4, n) for n in self._extents)
        for n, buf in zip(self._extents, bufs):
            if n not in self._filled:
                buf.copy_(torch.from_numpy(legendre_tables((n,))[0]))
                self._filled.add(n)
        return bufs

    def _stage(self, x_cl: torch.Tensor):
        if self.lr > 0.0:
            d, h, w = (int(e) for e in x_cl.shape[1:4])
            if max(d, h, w) > MAX_EXTENT:
                raise NotImplementedError(f"biasfield_tta: a volume of {d} x {h} x {w} voxels; the field's tables hold at most "
                                          f"{MAX_EXTENT} per axis")
            self._extents = (d, h, w)
            self._field_tables()
        return super()._stage(x_cl)

    # ------------------------------------------------------------------ one step
    def _apply(self, raw: torch.Tensor, x: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        t = self._tables()
        ops.bias_field_apply(raw, x, t["theta"], t["range"], self._field_tables(), self.order, self.anchor, present=present)

    def _input_step(self, raw: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        """dL/dtheta from what the backward left, Adam's step on theta and the two clamps: two launches."""
        t = self._tables()
        partial = self.rt.pool.flat("biasfield_partial", ops.bias_field_grad_partials(raw, self.order), dtype=torch.float64)
        ops.bias_field_grad(raw, self._input_branches(), t["theta"], t["range"], self._field_tables(), self.order, partial, t["grad"],
                            anchor=self.anchor, present=present, exp_avg=t["exp_avg"], exp_avg_sq=t["exp_avg_sq"], step=t["step"],
                            lr=self.lr, bounds=self.bounds, l2=self.l2)

    # ------------------------------------------------------------------ per volume
    @torch.no_grad()
    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """``EntropyMinimizationTTA.adapt_volume`` plus ``field_grad`` [steps, B, C, K] (dL/dtheta of every step, the l2 term
        included), ``field_coeff`` [B, C, K] (theta at the end; ``evaluate_field`` turns it into exp(F)) and ``field_terms``, the
        (a, b, c) of the K terms."""
        B, C, K = int(x.shape[0]), int(x.shape[1]), len(self.terms)
        out = super().adapt_volume(x, steps)
        out["field_terms"] = list(self.terms)
        out["field_grad"] = out["field_grad"][..., :K]
        if self.lr == 0.0:
            out["field_coeff"] = torch.zeros((B, C, K), dtype=torch.float32, device=x.device)
            return out
        out["field_coeff"] = self._tables()["theta"].view(-1, C, self.row)[:B, :, :K].clone()
        return out
