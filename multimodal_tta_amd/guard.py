"""The do-no-harm guard: ``method.guard``, read by ``EntropyMinimizationTTA`` and so by every plugin.

Per volume the plugin predicts once before its first step (what it returns at ``steps = 0``: the reference), adapts, and
compares the two hard predictions on the device.  Where the adapted mask has collapsed or exploded relative to the
reference, the reference logits are returned instead.  This module holds the config, the integer rule as the kernel takes it
(``include/mmtta.h``, mmtta_guard_select) and ``decide``, the same rule in Python integers.

With Q = 2^16, A = round(min_agreement Q), G = round(max_growth Q), H = round(max_shrink Q), m = min_voxels and the counts
s = |reference mask|, a = |adapted mask|, i = |both|, region (b, r) fails iff

    A > 0 and max(s, a) >= max(m, 1) and 2 i Q < A (s + a)      the Dice of the two masks is below min_agreement
 or G > 0 and a Q > G max(s, m)                                  the region exploded
 or H > 0 and s Q > H max(a, m)                                  the region vanished

Equality passes in every clause; with all three thresholds 0 the guard only monitors.  The shipped numbers are choices:
nobody has measured a Dice with them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, NamedTuple, Optional

from . import _lib
from .config import as_cfg, expect, get_config, is_integer, is_number, method_block

Q = 1 << 16
MAX_RATIO = 1024
MAX_VOXELS = (1 << 31) - 1
SCOPES = ("volume", "region")
DEFAULTS = {"enable": False, "min_agreement": 0.5, "max_growth": 4.0, "max_shrink": 4.0, "min_voxels": 64, "scope": "volume",
            "threshold": None}


@dataclass(frozen=True)
class GuardRule:
    """The rule in the integers the kernel takes: A in [0, Q]; G and H 0 (off) or in [Q, 1024 Q]; m in [0, 2^31 - 1]."""
    A: int = 0
    G: int = 0
    H: int = 0
    m: int = 0
    scope: str = "volume"

    def __post_init__(self):
        expect(is_integer(self.A) and 0 <= self.A <= Q, "GuardRule.A", self.A, f"an integer of 0 .. {Q}")
        for key, v in (("G", self.G), ("H", self.H)):
            expect(is_integer(v) and (v == 0 or Q <= v <= MAX_RATIO * Q), f"GuardRule.{key}", v,
                   f"0 (off) or an integer of {Q} .. {MAX_RATIO * Q}")
        expect(is_integer(self.m) and 0 <= self.m <= MAX_VOXELS, "GuardRule.m", self.m, "an integer of 0 .. 2^31 - 1")
        expect(self.scope in SCOPES, "GuardRule.scope", self.scope, "volume or region")

    @property
    def monitors_only(self) -> bool:
        return self.A == 0 and self.G == 0 and self.H == 0

    def struct(self) -> _lib.GuardRule:
        return _lib.GuardRule(self.A, self.G, self.H, self.m, SCOPES.index(self.scope), 0)


class GuardSpec(NamedTuple):
    enable: bool
    rule: GuardRule
    threshold: float


def region_fails(s: int, a: int, i: int, rule: GuardRule) -> bool:
    """The rule on one region's counts, in Python integers."""
    s, a, i = int(s), int(a), int(i)
    if rule.A > 0 and max(s, a) >= max(rule.m, 1) and 2 * i * Q < rule.A * (s + a):
        return True
    if rule.G > 0 and a * Q > rule.G * max(s, rule.m):
        return True
    return rule.H > 0 and s * Q > rule.H * max(a, rule.m)


def decide(counts: Any, rule: GuardRule):
    """counts [B,R,3] = (s, a, i) (a tensor, an array or nested lists) -> fallback, nested lists [B][R] of 0 / 1: what
    mmtta_guard_select writes.  Under ``scope: volume`` a volume with a failing region has every flag set."""
    rows = counts.tolist() if hasattr(counts, "tolist") else counts
    out = []
    for vol in rows:
        flags = [1 if region_fails(s, a, i, rule) else 0 for s, a, i in vol]
        if rule.scope == "volume" and any(flags):
            flags = [1] * len(flags)
        out.append(flags)
    return out


def parse_guard(config: Any) -> GuardSpec:
    """``method.guard`` of the root config -> GuardSpec; a ``ValueError`` names the offending key.  ``threshold`` defaults to
    ``evaluation.seg.threshold``, else 0.5.  Refused with the guard enabled: ``method.episodic: false`` (the reference would
    be a moving model) and ``scope: region`` on a ``training.criterion.softmax`` head (channels of two softmax rows mixed
    are no prediction)."""
    cfg = as_cfg(config)
    g = method_block(cfg, "guard")
    val = lambda k: get_config(g, k, DEFAULTS[k])
    enable = val("enable")
    expect(isinstance(enable, bool), "method.guard.enable", enable, "true or false")
    agree, grow, shrink = val("min_agreement"), val("max_growth"), val("max_shrink")
    expect(is_number(agree) and 0.0 <= agree <= 1.0, "method.guard.min_agreement", agree, "a number of 0 (off) .. 1")
    for key, v in (("max_growth", grow), ("max_shrink", shrink)):
        expect(is_number(v) and (v == 0 or 1.0 <= v <= MAX_RATIO), f"method.guard.{key}", v,
               f"0 (off) or a ratio of 1 .. {MAX_RATIO}")
    mv = val("min_voxels")
    expect(is_integer(mv) and 0 <= mv <= MAX_VOXELS, "method.guard.min_voxels", mv, "an integer of 0 .. 2^31 - 1")
    scope = val("scope")
    expect(scope in SCOPES, "method.guard.scope", scope, "volume or region")
    thr = get_config(g, "threshold", None)
    if thr is None:
        thr = get_config(cfg, "evaluation.seg.threshold", 0.5)
    expect(is_number(thr) and 0.0 < thr < 1.0, "method.guard.threshold", thr, "a number with 0 < threshold < 1")
    if enable:
        episodic = get_config(method_block(cfg), "episodic", True)
        if not bool(episodic):
            raise ValueError("method.guard.enable = True with method.episodic = False: the guard compares a volume with the "
                             "prediction of the model it starts from, which without the episodic reset is a moving model")
        if scope == "region" and bool(get_config(cfg, "training.criterion.softmax", False)):
            raise ValueError("method.guard.scope = 'region' with training.criterion.softmax = True: channels of two softmax "
                             "rows mixed are no prediction; use scope: volume")
    rule = GuardRule(int(round(float(agree) * Q)), int(round(float(grow) * Q)), int(round(float(shrink) * Q)), int(mv), scope)
    return GuardSpec(enable, rule, float(thr))


def guard_enabled(config: Any) -> bool:
    """``method.guard.enable`` as the evaluator reads it (validated by the plugin's constructor)."""
    return bool(get_config(method_block(as_cfg(config), "guard"), "enable", False))
