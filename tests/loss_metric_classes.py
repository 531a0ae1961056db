"""Case tables, float64 references and bounds of the kernels of csrc/loss_optim_metric.hip (mask + Dice counts, DiceCE sums and
gradient, the arena optimizers) and csrc/preproc.hip (intensity normalisation), one case per launch class.

Used by tests/test_loss_metric_classes_host.py (no GPU: classes, references against torch / the oracle, what each bound
catches) and tests/test_hip_loss_metric_classes.py (the launches).  Nothing here touches the GPU.

Operands are float64 torch tensors whose values are exactly representable in fp32 (hyper-parameters included: the C entry
points take floats), so a reference and its kernel see the same numbers.  A reference that several tests share is cached by
case name (functools.lru_cache) and never modified.

Bounds (u = 2^-24; DESIGN.md, "Loss, metric, optimizer and pre-pass parity per launch class"), none tuned to a kernel's output:
  equality      counts, masks, and every bit-for-bit claim
  sums          fp64-accumulated sums of fp32 terms: |err| <= r u sum|term| + dhw 2^-53 sum|term| (the fp64 additions);
                r per sum in R_SUMS below, with its count
  measured      what passes through libm, and the optimizer updates: 4 x the distance between torch's own fp32 CPU evaluation
                of the same expression and the float64 reference, floored at 4 fp32 ulp of the quantity's scale; the distance
                is measured on the CPU reference, never on the kernel
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import oracle

U = 2.0 ** -24
D53 = 2.0 ** -53

# fp32 roundings on the kernel's path to one term of a sum (expf counts as 1 ulp: DESIGN.md section 6)
R_SUMS = {
    # sigmoid p: e = expf(-|z|) (1), 1 + e (1), the division (1)
    "p": 3,
    # p (3) and the product p * y (1)
    "py": 4,
    # p * p: twice the relative error of p (6) and the product (1)
    "pp": 7,
    # y is read, (double) y is exact
    "y": 0,
    # y * y (1)
    "yy": 1,
}


def f32(v) -> float:
    return float(np.float32(v))


def rf32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()


def ulp32(v) -> float:
    return float(np.spacing(np.float32(abs(float(v)))))


def measured_bound(v32: torch.Tensor, v64: torch.Tensor) -> float:
    """4 x max|fp32 evaluation - float64|, floored at 4 fp32 ulp of the scale max|v64|."""
    if not v64.numel():
        return 0.0
    return max(4.0 * (v32.double() - v64).abs().max().item(), 4.0 * ulp32(v64.abs().max().item()))


# ============================================================================= mask + Dice counts
@dataclass(frozen=True)
class DiceCase:
    name: str
    klass: str                                   # the launch class the case exists for
    R: int
    shape: Tuple[int, int, int, int]             # N, D, H, W
    layout: str                                  # cl | cl_pad | ncdhw
    mask: bool
    thr: float
    want: Tuple[Tuple[str, object], ...]         # fields of dice_geometry() the case exists for
    seed: int = 0


def dice_geometry(R: int, dhw: int) -> Dict[str, object]:
    """The launch of mmtta_mask_dice_counts, restated from its launcher."""
    rp = 1
    while rp < R:
        rp <<= 1
    nvl = 256 // rp
    full = -(-dhw // (nvl * 16))
    bpn = max(1, min(full, 1024))
    return dict(rp=rp, nvl=nvl, bpn=bpn, capped=full > 1024, trips=-(-dhw // (bpn * nvl)), idle_lanes=dhw < nvl)


MARGIN = 1e-6            # no float64 sigmoid within this of the threshold: the kernel's fp32 sigmoid is within 4 u of it
ODD_LABELS = (0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0))), 2.0, -1.0)     # only the 2nd and 3rd are foreground


def _dice_cases() -> List[DiceCase]:
    w = lambda **k: tuple(sorted(k.items()))
    big = (1, 104, 104, 104)
    return [
        DiceCase("r1_fewer_voxels_than_lanes", "rp 1, one block, idle voxel lanes", 1, (1, 3, 5, 7), "cl", True, 0.5,
                 w(rp=1, nvl=256, bpn=1, idle_lanes=True), 1),
        DiceCase("r1_thr03_ncdhw_nomask", "rp 1, NCDHW, no mask", 1, (2, 17, 18, 19), "ncdhw", False, 0.3, w(rp=1, nvl=256, bpn=2), 2),
        DiceCase("r2_cl", "rp 2", 2, (2, 17, 18, 19), "cl", True, 0.5, w(rp=2, nvl=128, bpn=3), 3),
        DiceCase("r3_cl_n3", "rp 4 with an idle lane per voxel, dense rows, three items", 3, (3, 17, 18, 19), "cl", True, 0.5,
                 w(rp=4, nvl=64, bpn=6), 4),
        DiceCase("r3_clpad_thr03_nomask", "rp 4, row-padded (ldc 4), no mask", 3, (2, 17, 18, 19), "cl_pad", False, 0.3,
                 w(rp=4, nvl=64, bpn=6), 5),
        DiceCase("r3_ncdhw", "rp 4, NCDHW", 3, (2, 9, 10, 11), "ncdhw", True, 0.3, w(rp=4, nvl=64, bpn=1), 6),
        DiceCase("r4_ncdhw_nomask", "rp 4 without idle lanes", 4, (2, 9, 10, 11), "ncdhw", False, 0.5, w(rp=4, nvl=64), 7),
        DiceCase("r5_cl", "rp 8", 5, (2, 9, 10, 11), "cl", True, 0.5, w(rp=8, nvl=32, bpn=2), 8),
        DiceCase("r8_cl_nomask", "rp 8 without idle lanes", 8, (2, 9, 10, 11), "cl", False, 0.3, w(rp=8, nvl=32, bpn=2), 9),
        DiceCase("r129_capped", "rp 256, one voxel lane, capped grid with 18 trips", 129, (1, 26, 26, 26), "cl", True, 0.5,
                 w(rp=256, nvl=1, bpn=1024, capped=True, trips=18), 10),
        DiceCase("r256_ncdhw", "rp 256 without idle lanes", 256, (1, 5, 6, 7), "ncdhw", True, 0.3, w(rp=256, nvl=1, bpn=14), 11),
        DiceCase("r3_capped_104", "rp 4, capped grid with a second trip", 3, big, "cl_pad", True, 0.5,
                 w(rp=4, nvl=64, bpn=1024, capped=True, trips=18), 12),
    ]


DICE_CASES = _dice_cases()
DICE_BY_NAME = {c.name: c for c in DICE_CASES}


def away_from_threshold(z: torch.Tensor, thr32: float, gen) -> Tuple[torch.Tensor, int]:
    """Resample the logits whose float64 sigmoid lies within MARGIN of the threshold -> (logits, how many were resampled)."""
    moved = 0
    for _ in range(20):
        near = (torch.sigmoid(z) - thr32).abs() < MARGIN
        k = int(near.sum())
        if k == 0:
            return z, moved
        moved += k
        z = torch.where(near, rf32(torch.randn(z.shape, generator=gen, dtype=torch.float64) * 2), z)
    raise AssertionError("could not seed the logits away from the threshold")


def dice_counts_reference(z: torch.Tensor, lab: torch.Tensor, thr32: float):
    pred = torch.sigmoid(z) >= thr32
    gt = lab > 0.5
    n, r = z.shape[:2]
    cnt = torch.stack([(pred & gt).reshape(n, r, -1).sum(-1), pred.reshape(n, r, -1).sum(-1), gt.reshape(n, r, -1).sum(-1)], -1)
    return pred.to(torch.uint8), cnt.long()


@functools.lru_cache(maxsize=None)
def make_dice(name: str) -> Dict[str, object]:
    c = DICE_BY_NAME[name]
    gen = torch.Generator().manual_seed(1000 + c.seed)
    n, (d, h, w) = c.shape[0], c.shape[1:]
    thr32 = f32(c.thr)
    z = rf32(torch.randn((n, c.R, d, h, w), generator=gen, dtype=torch.float64) * 2)
    lab = (torch.rand((n, c.R, d, h, w), generator=gen) > 0.6).double()
    odd = torch.rand(lab.shape, generator=gen) < 0.05
    pick = torch.randint(0, len(ODD_LABELS), lab.shape, generator=gen)
    lab = torch.where(odd, torch.tensor(ODD_LABELS, dtype=torch.float64)[pick], lab)
    # the items differ; one has an empty label region, one an empty prediction
    if n > 1 or c.R > 1:
        lab[n // 2, c.R - 1] = 0.0
        z[n - 1, 0] = -30.0
    z, moved = away_from_threshold(z, thr32, gen)
    pred, cnt = dice_counts_reference(z, lab, thr32)
    return dict(z=z, lab=lab, thr32=thr32, pred=pred, counts=cnt, resampled=moved)


# ============================================================================= DiceCE sums and gradient
CLASS_WEIGHTS = (0.5, 2.0, 1.0, 1.5, 0.75, 1.25, 3.0, 0.25)
DCE_DEFAULTS = dict(squared_pred=False, jaccard=False, include_background=True, weight=False, lambda_dice=1.0, lambda_ce=1.0,
                    smooth_nr=f32(1e-5), smooth_dr=f32(1e-5))
SMOOTH = (f32(1e-5), f32(1e-3), 1.0)


def _dce_options() -> Dict[str, Dict[str, object]]:
    """The four switches crossed (16 sets); lambda != 1 on every other set, smooth_nr / smooth_dr walk SMOOTH x SMOOTH."""
    out = {}
    for i in range(16):
        sq, jac, nobg, wt = (bool(i >> b & 1) for b in range(4))
        o = dict(squared_pred=sq, jaccard=jac, include_background=not nobg, weight=wt, smooth_nr=SMOOTH[i % 3], smooth_dr=SMOOTH[i // 3 % 3])
        if i % 2 == 0 and i:
            o.update(lambda_dice=2.0, lambda_ce=0.5)
        elif i % 4 == 3:
            o.update(lambda_dice=5.0, lambda_ce=0.25)
        out["".join(n for n, on in (("sq", sq), ("jac", jac), ("nobg", nobg), ("w", wt)) if on) or "plain"] = o
    return out


DCE_OPTIONS = _dce_options()
# the two criteria the configs ship (configs/_global_patches/brats.yaml, hecktor21.yaml)
SHIPPED = {"brats": ("sigmoid", 3, {}), "hecktor": ("sigmoid", 1, dict(include_background=False, weight=True, lambda_dice=5.0))}
BPN_CLASSES = {"bpn<64": lambda b: b < 64, "bpn>64": lambda b: 64 < b < 1024, "bpn=1024": lambda b: b == 1024}


@dataclass(frozen=True)
class DceCase:
    name: str
    klass: str                    # bpn<64 | bpn>64 (the finish kernel's second trip) | bpn=1024 (capped; gradient's second trip)
    N: int
    R: int
    shape: Tuple[int, int, int]
    head: str                     # sigmoid | softmax
    option: str                   # key of DCE_OPTIONS, or a SHIPPED name
    labels: str                   # nested | onehot | soft
    special: str = ""             # empty_label | dead_logits | both | saturated
    seed: int = 0

    @property
    def opts(self) -> Dict[str, object]:
        o = dict(DCE_DEFAULTS)
        o.update(SHIPPED[self.option][2] if self.option in SHIPPED else DCE_OPTIONS[self.option])
        return o

    @property
    def softmax(self) -> bool:
        return self.head == "softmax"


def _dce_cases() -> List[DceCase]:
    out = []
    heads = [("sigmoid", 1), ("sigmoid", 2), ("sigmoid", 3), ("sigmoid", 4), ("sigmoid", 8),
             ("softmax", 2), ("softmax", 3), ("softmax", 4), ("softmax", 8)]
    k = 0
    for head, R in heads:
        for opt in DCE_OPTIONS:
            shape = (3, 5, 7) if k % 2 else (6, 10, 12)                         # 105 and 720 voxels
            labels = ("soft", "onehot" if head == "softmax" else "nested", "nested" if head == "sigmoid" else "soft")[k % 3]
            out.append(DceCase(f"{head}_r{R}_{opt}_{shape[0] * shape[1] * shape[2]}", "bpn<64", 2, R, shape, head, opt, labels, seed=k))
            k += 1
    for i, special in enumerate(("empty_label", "dead_logits", "both", "saturated")):
        for head, R in (("sigmoid", 1), ("sigmoid", 3), ("softmax", 4)):
            opt = ("plain", "sq", "sqjacnobgw")[i % 3] if special != "saturated" else "w"
            out.append(DceCase(f"{head}_r{R}_{special}", "bpn<64", 2, R, (6, 10, 12), head, opt,
                               "onehot" if head == "softmax" else "nested", special, seed=200 + 3 * i + R))
    # more than 64 partials through the finish kernel: the two shipped criteria and a softmax head
    out.append(DceCase("brats_41", "bpn>64", 1, 3, (41, 41, 41), "sigmoid", "brats", "nested", seed=300))
    out.append(DceCase("hecktor_41", "bpn>64", 2, 1, (41, 41, 41), "sigmoid", "hecktor", "nested", seed=301))
    out.append(DceCase("softmax_r8_41", "bpn>64", 1, 8, (41, 41, 41), "softmax", "sqjacnobgw", "soft", seed=302))
    # the capped sums grid; 2 x 104^3 = 2 249 728 voxels > 8192 x 256 threads, the item index changes inside a trip
    out.append(DceCase("brats_104", "bpn=1024", 2, 3, (104, 104, 104), "sigmoid", "brats", "nested", seed=303))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


DCE_CASES = _dce_cases()
DCE_BY_NAME = {c.name: c for c in DCE_CASES}
SATURATED = (0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4)
PLANTED = 3.0            # the logits of the last voxel of the last item: every channel's p there is >= 1 / R


def dce_weight(c: DceCase) -> Optional[torch.Tensor]:
    if not c.opts["weight"]:
        return None
    return torch.tensor([50.0] if c.R == 1 else list(CLASS_WEIGHTS[:c.R]), dtype=torch.float64)


def dce_loss_module(c: DceCase, dtype, **override):
    o = dict(c.opts)
    o.update(override)
    w = dce_weight(c)
    m = oracle.DiceCELoss(include_background=o["include_background"], sigmoid=not c.softmax, softmax=c.softmax,
                          squared_pred=o["squared_pred"], jaccard=o["jaccard"], smooth_nr=o["smooth_nr"], smooth_dr=o["smooth_dr"],
                          weight=w, lambda_dice=o["lambda_dice"], lambda_ce=o["lambda_ce"])
    return m.to(dtype)


def dce_terms(c: DceCase, z: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor]):
    """Per-voxel terms [N, R, 3, V] of the three Dice sums and [N, V] of the CE numerator, in the dtype of `z`."""
    n, r = z.shape[:2]
    zf, yf = z.reshape(n, r, -1), y.reshape(n, r, -1)
    p = torch.softmax(zf, 1) if (c.softmax and r > 1) else torch.sigmoid(zf)
    sq = c.opts["squared_pred"]
    dice = torch.stack([p * yf, p * p if sq else p, yf * yf if sq else yf], 2)
    if r == 1:
        pw = 1.0 if w is None else w[0].to(z.dtype)
        ce = ((1 - yf) * zf + (1 + (pw - 1) * yf) * torch.nn.functional.softplus(-zf))[:, 0]
    else:
        wr = torch.ones(r, dtype=z.dtype) if w is None else w.to(z.dtype)
        ce = -(wr.view(1, r, 1) * yf * torch.log_softmax(zf, 1)).sum(1)
    return dice, ce


def dce_sums(c: DceCase, z, y, w):
    """-> (sums [N, 3R+1] float64, sum of |term| [N, 3R+1]) from terms evaluated in the dtype of `z`."""
    dice, ce = dce_terms(c, z, y, w)
    n, r = z.shape[:2]
    s = torch.cat([dice.double().sum(-1).reshape(n, 3 * r), ce.double().sum(-1, keepdim=True)], 1)
    a = torch.cat([dice.double().abs().sum(-1).reshape(n, 3 * r), ce.double().abs().sum(-1, keepdim=True)], 1)
    return s, a


def dce_sum_bounds(c: DceCase, s64, a64, s32) -> torch.Tensor:
    """[N, 3R+1]: the rule of each column (module docstring)."""
    n, r = s64.shape[0], c.R
    dhw = c.shape[0] * c.shape[1] * c.shape[2]
    sq = c.opts["squared_pred"]
    b = torch.empty_like(s64)
    lib = torch.maximum(4 * (s32 - s64).abs(), 4 * U * a64)                      # through logf / log1pf: measured
    for k in range(3 * r):
        if k % 3 == 2:
            rr = R_SUMS["yy" if sq else "y"]
        elif c.softmax and r > 1:
            rr = None                   # p = expf(z - max) / se: the rounding of z - max is amplified by |z - max|, no fixed r
        else:
            rr = R_SUMS["py"] if k % 3 == 0 else R_SUMS["pp" if sq else "p"]
        b[:, k] = lib[:, k] if rr is None else rr * U * a64[:, k]
    b[:, 3 * r] = lib[:, 3 * r]
    return b + dhw * D53 * a64


def dce_loss_from_sums(c: DceCase, s: torch.Tensor, ds: Optional[torch.Tensor] = None):
    """The loss the project reports from the kernel's sums (trainer.loss_value / DiceCEReport.value, with the case's smooth
    terms), in float64; with `ds` (bounds of the sums) also its first-order bound."""
    o, n, r = c.opts, s.shape[0], c.R
    dhw = c.shape[0] * c.shape[1] * c.shape[2]
    per = s[:, :3 * r].reshape(n, r, 3)
    dper = torch.zeros_like(per) if ds is None else ds[:, :3 * r].reshape(n, r, 3)
    r0 = 1 if (not o["include_background"] and r > 1) else 0
    I, Q, G = (per[:, r0:, j] for j in range(3))
    dI, dQ, dG = (dper[:, r0:, j] for j in range(3))
    den, dden = G + Q, dG + dQ
    if o["jaccard"]:
        den, dden = 2.0 * (den - I), 2.0 * (dden + dI)
    A, D = 2.0 * I + o["smooth_nr"], den + o["smooth_dr"]
    f, df = 1.0 - A / D, 2.0 * dI / D + A.abs() * dden / (D * D)
    w = dce_weight(c)
    if w is not None and f.shape[1] != 1:
        f, df = f * w[r0:], df * w[r0:]
    loss = o["lambda_dice"] * f.mean() + o["lambda_ce"] * s[:, 3 * r].sum() / (n * dhw)
    if ds is None:
        return loss.item()
    bound = o["lambda_dice"] * df.mean() + o["lambda_ce"] * ds[:, 3 * r].sum() / (n * dhw)
    return loss.item(), 1.001 * bound.item()


def dce_operands(c: DceCase):
    gen = torch.Generator().manual_seed(2000 + c.seed)
    n, r, (d, h, w) = c.N, c.R, c.shape
    shp = (n, r, d, h, w)
    if c.special == "saturated":
        z = torch.tensor(SATURATED, dtype=torch.float64)[torch.randint(0, len(SATURATED), shp, generator=gen)]
    else:
        z = rf32(torch.randn(shp, generator=gen, dtype=torch.float64) * 2)
    if c.labels == "onehot":
        y = torch.nn.functional.one_hot(torch.randint(0, r, (n, d, h, w), generator=gen), r).permute(0, 4, 1, 2, 3).double()
    elif c.labels == "nested":
        # nested binary regions (ET inside TC inside WT): region k = field > its own, falling level
        fld = torch.rand((n, 1, d, h, w), generator=gen, dtype=torch.float64)
        y = (fld > torch.linspace(0.9, 0.5, r, dtype=torch.float64).view(1, r, 1, 1, 1)).double()
    else:
        y = rf32(torch.rand(shp, generator=gen, dtype=torch.float64))
    if c.special in ("empty_label", "both"):
        y[:, r - 1] = 0.0
    if c.special in ("dead_logits", "both"):
        z[:, r - 1] = -30.0
    z[-1, :, -1, -1, -1] = PLANTED
    return z.contiguous(), y.contiguous()


@functools.lru_cache(maxsize=None)
def make_dce(name: str) -> Dict[str, object]:
    c = DCE_BY_NAME[name]
    z, y = dce_operands(c)
    w = dce_weight(c)
    s64, a64 = dce_sums(c, z, y, w)
    s32, _ = dce_sums(c, z.float(), y.float(), None if w is None else w.float())
    out = dict(z=z, y=y, w=w, sums=s64, terms=a64, sums32=s32, sum_bounds=dce_sum_bounds(c, s64, a64, s32))
    for dtype, key in ((torch.float64, "64"), (torch.float32, "32")):
        zz = z.to(dtype).clone().requires_grad_(True)
        loss = dce_loss_module(c, dtype)(zz, y.to(dtype))
        loss.backward()
        out["loss" + key], out["grad" + key] = loss.item(), zz.grad.detach()
    # the measured rule, and the bound the project already holds (tests/test_hip_tta.py): the gradient stays inside both
    out["grad_measured"] = measured_bound(out["grad32"], out["grad64"])
    out["grad_held"] = (5e-5 if c.softmax else 2e-5) * out["grad64"].abs().max().item()
    out["grad_bound"] = min(out["grad_measured"], out["grad_held"])
    return out


# ============================================================================= optimizers
HYPER = {
    "adam": ("adam", dict(lr=1e-3, betas=(0.9, 0.9999), eps=1e-8, weight_decay=5e-4)),
    "adam_wd0": ("adam", dict(lr=1e-3, betas=(0.9, 0.9999), eps=1e-8, weight_decay=0.0)),
    "adamw": ("adamw", dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)),
    "adamw_wd0": ("adamw", dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)),
    "sgd_mom": ("sgd", dict(lr=1e-2, momentum=0.9, weight_decay=1e-4, dampening=0.0, nesterov=False)),
    "sgd_nesterov": ("sgd", dict(lr=1e-2, momentum=0.9, weight_decay=1e-4, dampening=0.0, nesterov=True)),
    "sgd_damp": ("sgd", dict(lr=1e-2, momentum=0.8, weight_decay=0.0, dampening=0.3, nesterov=False)),
    "sgd_plain": ("sgd", dict(lr=1e-2, momentum=0.0, weight_decay=1e-3, dampening=0.0, nesterov=False)),
}


def hyper(key: str):
    """(kind, keyword arguments of torch.optim with every value rounded to fp32: what the C entry point receives)."""
    kind, kw = HYPER[key]
    out = {}
    for k, v in kw.items():
        out[k] = tuple(f32(b) for b in v) if k == "betas" else (v if isinstance(v, bool) else f32(v))
    return kind, out


GRID_ELEMS = 4096 * 256 * 4          # one trip of the capped optimizer grid


@dataclass(frozen=True)
class OptCase:
    name: str
    klass: str
    hp: str                                # key of HYPER
    mode: str                              # plain | sets | segments
    n: int = 0                             # plain / sets: trained elements per replica
    n_decay: int = 0
    steps: int = 5
    replicas: int = 1
    used: int = 1
    stride: int = 0
    segs: Tuple[Tuple[int, int, bool], ...] = ()
    step0: int = 0                         # the step counter before the first call (moments then hold valid state)
    seed: int = 0


def _opt_cases() -> List[OptCase]:
    out = []
    k = 0
    for hp in HYPER:
        for n in (36, 1036, 1037, 1038, 1039):
            for which, nd in (("nd0", 0), ("ndmid", (n // 2) // 4 * 4), ("ndall", n // 4 * 4)):
                tail = n % 4
                out.append(OptCase(f"{hp}_n{n}_{which}", f"one trip, ragged tail of {tail}" if tail else "one trip, whole quads", hp,
                                   "plain", n, nd, seed=k))
                k += 1
    big = GRID_ELEMS + 1028
    for hp in ("adam", "adamw", "sgd_nesterov"):
        out.append(OptCase(f"{hp}_second_trip", "capped grid, second trip, decay boundary inside it", hp, "plain", big, GRID_ELEMS + 512,
                           steps=2, seed=500 + len(out)))
    out.append(OptCase("sgd_plain_second_trip_ragged", "capped grid, second trip, ragged tail", "sgd_plain", "plain", big + 3, GRID_ELEMS,
                       steps=2, seed=510))
    out.append(OptCase("adam_step_9999", "late step: bias corrections through pow in double", "adam", "plain", 1036, 1000, steps=1,
                       step0=9999, seed=520))
    for hp in ("adam", "sgd_mom", "sgd_plain"):
        for n in (36, 1036):
            out.append(OptCase(f"{hp}_sets_n{n}", "two of three replicas, stride n + 64", hp, "sets", n, n // 2 // 4 * 4, steps=3,
                               replicas=3, used=2, stride=n + 64, seed=530 + len(out)))
    out.append(OptCase("adamw_one_segment", "one segment", "adamw", "segments", steps=3, replicas=2, used=2, stride=1100,
                       segs=((8, 1000, True),), seed=540))
    gaps = tuple((8 * i, 4, i % 2 == 0) for i in range(300))
    for hp in ("adam", "sgd_mom"):
        out.append(OptCase(f"{hp}_300_segments", "300 four-element segments with gaps, alternating decay", hp, "segments", steps=3,
                           replicas=3, used=2, stride=2464, segs=gaps, seed=541 + len(out)))
    out.append(OptCase("adam_segments_second_trip", "segment table longer than the capped grid", "adam", "segments", steps=2, replicas=1,
                       used=1, stride=4_200_320, segs=((0, 2_000_000, True), (2_000_064, 2_000_000, False), (4_000_256, 200_000, True)),
                       seed=550))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


OPT_CASES = _opt_cases()
OPT_BY_NAME = {c.name: c for c in OPT_CASES}


def opt_layout(c: OptCase, n_decay: Optional[int] = None):
    """(replicas, stride, used, active [stride] bool, decay [stride] bool): the elements of a used replica the call updates."""
    nd = c.n_decay if n_decay is None else n_decay
    if c.mode == "segments":
        active, decay = torch.zeros(c.stride, dtype=torch.bool), torch.zeros(c.stride, dtype=torch.bool)
        for a, n, dec in c.segs:
            active[a:a + n] = True
            decay[a:a + n] = dec
        return c.replicas, c.stride, c.used, active, decay
    stride = c.stride or c.n
    idx = torch.arange(stride)
    return c.replicas, stride, c.used, idx < c.n, idx < nd


def opt_restated(kind: str, kw: Dict[str, object], p, grads, m, v, decay, step0: int):
    """torch.optim.{Adam, AdamW, SGD} restated in float64 over flat tensors; `decay` [n] bool.  -> (p, m, v) after the steps;
    m is exp_avg or the momentum buffer (None while SGD keeps none), v is exp_avg_sq (None for SGD)."""
    p = p.clone()
    wd = kw.get("weight_decay", 0.0)
    if kind in ("adam", "adamw"):
        b1, b2 = kw["betas"]
        m = torch.zeros_like(p) if step0 == 0 else m.clone()
        v = torch.zeros_like(p) if step0 == 0 else v.clone()
        for t, g in enumerate(grads, start=step0 + 1):
            if kind == "adam":
                g = torch.where(decay, g + wd * p, g)
            else:
                p = torch.where(decay, p * (1.0 - kw["lr"] * wd), p)
            m = m + (1.0 - b1) * (g - m)
            v = b2 * v + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            p = p - (kw["lr"] / bc1) * m / (v.sqrt() / math.sqrt(bc2) + kw["eps"])
        return p, m, v
    mu, damp = kw["momentum"], kw["dampening"]
    buf = None if step0 == 0 else m.clone()
    for g in grads:
        g = torch.where(decay, g + wd * p, g)
        if mu != 0.0:
            buf = g.clone() if buf is None else mu * buf + (1.0 - damp) * g
            g = g + mu * buf if kw["nesterov"] else buf
        p = p - kw["lr"] * g
    return p, (buf if mu != 0.0 else None), None


def opt_torch(kind: str, kw: Dict[str, object], p, grads, m, v, decay, step0: int, dtype):
    """torch.optim itself in `dtype` on the CPU with the reference's two parameter groups -> (p, m, v) as above."""
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}[kind]
    tkw = dict(kw)
    wd = tkw.pop("weight_decay", 0.0)
    parts = [(decay, wd), (~decay, 0.0)]
    params = [torch.nn.Parameter(p[sel].to(dtype).clone()) for sel, _ in parts]
    groups = [{"params": [q], "weight_decay": w_} for q, (sel, w_) in zip(params, parts) if q.numel()]
    opt = cls(groups, **tkw)
    if step0:
        for q, (sel, _) in zip(params, parts):
            if not q.numel():
                continue
            if kind == "sgd":
                opt.state[q]["momentum_buffer"] = m[sel].to(dtype).clone()
            else:
                opt.state[q].update(step=torch.tensor(float(step0)), exp_avg=m[sel].to(dtype).clone(), exp_avg_sq=v[sel].to(dtype).clone())
    for g in grads:
        for q, (sel, _) in zip(params, parts):
            q.grad = g[sel].to(dtype).clone()
        opt.step()
    po = torch.empty(p.shape, dtype=dtype)
    mo = torch.empty(p.shape, dtype=dtype) if (kind != "sgd" or kw["momentum"] != 0.0) else None
    vo = torch.empty(p.shape, dtype=dtype) if kind != "sgd" else None
    for q, (sel, _) in zip(params, parts):
        if not q.numel():
            continue
        po[sel] = q.detach()
        if mo is not None:
            mo[sel] = opt.state[q]["momentum_buffer" if kind == "sgd" else "exp_avg"]
        if vo is not None:
            vo[sel] = opt.state[q]["exp_avg_sq"]
    return po, mo, vo


def opt_operands(c: OptCase):
    """p0, m0, v0 [replicas, stride] and the gradients of every step [steps][replicas, stride] (fp32 values in float64)."""
    gen = torch.Generator().manual_seed(3000 + c.seed)
    reps, stride = opt_layout(c)[:2]
    rnd = lambda: torch.randn((reps, stride), generator=gen, dtype=torch.float64)
    sgn = torch.where(torch.rand((reps, stride), generator=gen) < 0.5, -1.0, 1.0).double()
    p0 = rf32(sgn * (0.5 + torch.rand((reps, stride), generator=gen, dtype=torch.float64)))         # 0.5 <= |p| < 1.5
    grads = [rf32(rnd() * 10.0 ** (-t)) for t in range(c.steps)]
    m0 = rf32(rnd() * 0.1)
    v0 = rf32(torch.rand((reps, stride), generator=gen, dtype=torch.float64) * 0.01 + 1e-4)
    return p0, m0, v0, grads


def opt_flat(c: OptCase, t: torch.Tensor, active: torch.Tensor) -> torch.Tensor:
    return t[:c.used][:, active].reshape(-1)


def opt_reference(c: OptCase, n_decay: Optional[int] = None):
    """Float64 restatement and torch's fp32 evaluation over the updated elements (flat: used replicas x active elements)."""
    kind, kw = hyper(c.hp)
    reps, stride, used, active, decay = opt_layout(c, n_decay)
    p0, m0, v0, grads = opt_operands(c)
    fl = lambda t: opt_flat(c, t, active)
    dec = decay[active].repeat(used)
    args = (fl(p0), [fl(g) for g in grads], fl(m0), fl(v0), dec, c.step0)
    r64 = opt_restated(kind, kw, *args)
    r32 = opt_torch(kind, kw, *args, torch.float32)
    return dict(p=r64[0], m=r64[1], v=r64[2], p32=r32[0], m32=r32[1], v32=r32[2])


@functools.lru_cache(maxsize=None)
def make_opt(name: str):
    c = OPT_BY_NAME[name]
    ref = opt_reference(c)
    ref["bounds"] = {q: measured_bound(ref[q + "32"], ref[q]) for q in ("p", "m", "v") if ref[q] is not None}
    return ref


# ============================================================================= intensity normalisation
INF = float("inf")
RULES8 = (
    {"clip": [-2.0, 2.0], "zscore": {"masked": True, "mask_gt": -0.5}},            # 0 clip + masked z-score
    {"zscore": {"masked": False}},                                                    # 1 z-score of all voxels (mean 1e4)
    {"zscore": {"masked": True}},                                                     # 2 mask_gt = -inf: every voxel passes
    {"clip": [-1.0, 1.0]},                                                            # 3 clip only
    {},                                                                               # 4 no-op
    {"clip": [0.0, 5.0], "zscore": {"masked": True, "mask_gt": -1.0}},                # 5 lo > mask_gt: every CLIPPED voxel passes
    {"zscore": {"masked": True, "mask_gt": 0.0, "min_count": "count"}},               # 6 masked count == min_count
    {"zscore": {"masked": True, "mask_gt": 0.0, "min_count": "count+1"}},             # 7 masked count == min_count - 1
)
SPARSE = 37              # voxels above mask_gt in the channels of rules 6 and 7


@dataclass(frozen=True)
class IntCase:
    name: str
    klass: str
    C: int
    shape: Tuple[int, int, int]
    rules: Tuple[int, ...] = ()          # indices into RULES8, per channel; () = the legacy mean / std form
    const: Tuple[int, ...] = ()          # channels holding one value (sd -> eps)
    strided: bool = False                # the input is a non-contiguous view
    seed: int = 0


INT_CASES = [
    IntCase("c1_100", "one statistics block, partly idle", 1, (4, 5, 5), (0,), seed=1),
    IntCase("c8_100", "8 channels (PRE_MAXC), eight rules in one call", 8, (4, 5, 5), tuple(range(8)), seed=2),
    IntCase("c8_17280", "68 statistics blocks: the finalize wave's second trip", 8, (12, 36, 40), tuple(range(8)), seed=3),
    IntCase("c8_41", "all 256 statistics blocks with a second trip", 8, (41, 41, 41), tuple(range(8)), seed=4),
    IntCase("c1_104", "capped apply grid (4096 blocks) with a second trip", 1, (104, 104, 104), (0,), seed=5),
    IntCase("c2_const", "a constant channel: sd -> eps", 2, (12, 36, 40), (0, 2), const=(1,), seed=6),
    IntCase("c2_strided", "non-contiguous input", 2, (6, 10, 12), (0, 1), strided=True, seed=7),
    IntCase("legacy4", "legacy mean / std on 4 channels", 4, (6, 10, 12), (), seed=8),
]
INT_BY_NAME = {c.name: c for c in INT_CASES}
LEGACY_MEAN, LEGACY_STD = (f32(0.1), f32(0.2), f32(0.3), f32(0.4)), (1.0, 2.0, 0.5, 4.0)


def int_geometry(dhw: int) -> Dict[str, object]:
    """The launches of mmtta_intensity_normalize, restated from its launcher."""
    blocks = -(-dhw // 256)
    sblocks = min(blocks, 256)
    return dict(sblocks=sblocks, stats_second_trip=dhw > sblocks * 256, finalize_second_trip=sblocks > 64,
                apply_blocks=min(blocks, 4096), apply_second_trip=blocks > 4096)


def int_operands(c: IntCase) -> torch.Tensor:
    gen = torch.Generator().manual_seed(4000 + c.seed)
    d, h, w = c.shape
    x = rf32(torch.randn((c.C, d, h, w), generator=gen, dtype=torch.float64) * 1.5)
    for ch, r in enumerate(c.rules):
        if r == 1:
            x[ch] = rf32(1e4 + torch.randn((d, h, w), generator=gen, dtype=torch.float64))
        if r in (6, 7):
            flat = -x[ch].abs().reshape(-1)                       # nothing above mask_gt = 0 ...
            where = torch.randperm(flat.numel(), generator=gen)[:SPARSE]
            flat[where] = rf32(1.0 + torch.rand(SPARSE, generator=gen, dtype=torch.float64))      # ... but these
            x[ch] = flat.reshape(d, h, w)
    for ch in c.const:
        x[ch] = 7.0
    return x


def int_rules(c: IntCase) -> List[Dict[str, object]]:
    """The rule dictionaries of the case, with the symbolic min_count of rules 6 / 7 resolved."""
    out = []
    for r in c.rules:
        rule = {k: (dict(v) if isinstance(v, dict) else v) for k, v in RULES8[r].items()}
        mc = rule.get("zscore", {}).get("min_count")
        if mc is not None:
            rule["zscore"]["min_count"] = SPARSE + (1 if mc == "count+1" else 0)
        out.append(rule)
    return out


def int_policy(c: IntCase) -> Dict[str, object]:
    return {"enabled": True, "channels": {str(i): r for i, r in enumerate(int_rules(c))}}


def int_kwargs(c: IntCase) -> Dict[str, object]:
    return dict(intensity_policy=int_policy(c)) if c.rules else dict(mean=list(LEGACY_MEAN), std=list(LEGACY_STD))


def int_restated(x: torch.Tensor, rules: List[Dict[str, object]], mean=None, std=None, mask_before_clip=False, strict_count=False):
    """oracle.normalize_image restated in float64 -> (out, per-channel dict of the statistics used).  The two flags restate
    two mistakes a kernel could make (masking on the unclipped value; `>` for `>=` at min_count)."""
    out, stats = x.clone(), []
    if not rules:
        for ch in range(x.shape[0]):
            out[ch] = (x[ch] - mean[ch]) / std[ch]
        return out, stats
    for ch, rule in enumerate(rules):
        v = x[ch]
        raw = v
        if "clip" in rule:
            v = v.clamp(rule["clip"][0], rule["clip"][1])
        st = None
        if "zscore" in rule:
            zc = rule["zscore"]
            vals = allv = v.reshape(-1)
            sel = ((raw if mask_before_clip else v) > zc.get("mask_gt", -INF)).reshape(-1)
            n_m = int(sel.sum())
            mc = int(zc.get("min_count", 16))
            if zc.get("masked", True) and ((n_m > mc) if strict_count else (n_m >= mc)):
                vals = vals[sel]
            mu = vals.mean()
            sd = ((vals - mu) ** 2).mean().sqrt().clamp_min(f32(zc.get("eps", 1e-6)))
            mv = allv[sel]
            # the five sums of the kernel's statistics pass and the sum of |term| of each
            sums = [float(n_m), mv.sum().item(), (mv * mv).sum().item(), allv.sum().item(), (allv * allv).sum().item()]
            terms = [0.0, mv.abs().sum().item(), sums[2], allv.abs().sum().item(), sums[4]]
            st = dict(n=vals.numel(), mu=mu.item(), sd=sd.item(), sums=sums, terms=terms, masked_used=vals.numel() != allv.numel())
            v = (v - mu) / sd
        out[ch] = v
        stats.append(st)
    return out, stats


@functools.lru_cache(maxsize=None)
def make_int(name: str):
    c = INT_BY_NAME[name]
    x = int_operands(c)
    ref, stats = int_restated(x, int_rules(c), LEGACY_MEAN, LEGACY_STD)
    o32 = oracle.normalize_image(x.float(), **int_kwargs(c))
    exact = [bool(c.rules) and "zscore" not in RULES8[r] for r in c.rules] if c.rules else [False] * c.C
    bounds = [0.0 if exact[ch] else measured_bound(o32[ch], ref[ch]) for ch in range(c.C)]
    return dict(x=x, ref=ref, stats=stats, o32=o32, bounds=bounds, exact=exact)
