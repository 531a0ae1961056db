"""Evaluation plugins for the adaptation path.

``seg_eval`` is the reference's strategy under its own name (reference
src/evaluation/seg_eval.py:151, contract SURVEY.md section 8b): same constructor (root config),
same ``evaluate_epoch(model, data_loader, device) -> Dict[str, float]``, same metric keys and
float64 aggregation (:250-270, :363-378, :402-460), same errors (:279-302).  What changed is where
the voxel work runs: threshold + the three reductions of ``_binary_dice_iou`` (:41-68, :304-306)
are one HIP kernel returning exact integer counts, so a batch costs ONE device->host copy instead
of the reference's 3*B*R ``.item()`` syncs (:366-368).

``seg_tta_eval`` adapts every volume with the ``entmin_tta`` plugin before scoring it, shards
volumes across ranks (one process per GPU) and merges the per-volume table with a single
``all_gather`` - RCCL over xGMI on an MI355X node, gloo in the CPU tests.
"""
from __future__ import annotations

import math
from collections import defaultdict
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import ops
from .config import as_cfg, get_config
from .registry import get_plugin, register_evaluation_strategy

EPS = 1e-7


# ----------------------------------------------------------------------------- small host-side pieces
def as_list_str(x: Any, batch_size: int) -> List[str]:
    """batch['domain'] in any collated form -> list[str] of length B (reference seg_eval.py:19-38)."""
    if x is None:
        return [""] * batch_size
    if isinstance(x, (list, tuple)):
        return [str(v) for v in x]
    if isinstance(x, str):
        return [x] * batch_size
    if torch.is_tensor(x):
        if x.ndim == 0:
            return [str(int(x.item()))] * batch_size
        if x.numel() == batch_size:
            return [str(int(v.item())) for v in x.view(-1)]
    return [str(x)] * batch_size


def dice_iou_from_counts(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """counts int64 [B,R,3] = (inter, pred, gt) -> dice, iou, valid with the reference's fp32 formulas
    (seg_eval.py:55-66).  The counts are exact (< 2**24 per the shipped shapes), so the fp32 values equal
    the reference's sums of {0,1} floats bit for bit."""
    c = counts.to(torch.float32)
    inter, ps, gs = c[..., 0], c[..., 1], c[..., 2]
    valid = gs > 0
    dice = (2.0 * inter + EPS) / (ps + gs + EPS)
    iou = (inter + EPS) / (ps + gs - inter + EPS)
    return dice, iou, valid


CALIBRATION_SCOPES = ("volume", "union")
CALIBRATION_MAX_BINS = 64


def calibration_config(config: Any) -> Tuple[bool, int, str]:
    """``evaluation.calibration: {enable, bins, scope}`` -> (enable, bins, scope); off, 15 bins, ``volume`` when absent.
    A value the kernel cannot take is a ``ValueError`` that names its key, whether the block is enabled or not."""
    cal = get_config(config, "evaluation.calibration", {}) or {}
    enable = get_config(cal, "enable", False)
    if not isinstance(enable, bool):
        raise ValueError(f"evaluation.calibration.enable must be true or false, got {enable!r}")
    bins = get_config(cal, "bins", 15)
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= CALIBRATION_MAX_BINS:
        raise ValueError(f"evaluation.calibration.bins must be an integer in 1 ... {CALIBRATION_MAX_BINS}, got {bins!r}")
    scope = get_config(cal, "scope", "volume")
    if scope not in CALIBRATION_SCOPES:
        raise ValueError(f"evaluation.calibration.scope must be one of {list(CALIBRATION_SCOPES)}, got {scope!r}")
    return enable, int(bins), str(scope)


POSTPROCESS_CONNECTIVITIES = ops.COMPONENT_CONNECTIVITIES


def postprocess_config(config: Any) -> Tuple[bool, int, List[int], List[bool]]:
    """``evaluation.postprocess: {enable, connectivity, min_voxels, keep_largest}`` -> (enable, connectivity, min_voxels,
    keep_largest), the last two as one entry per region of ``evaluation.seg.region_order``; off, 26, 0 and false when
    absent.  ``min_voxels`` is an int or a list of ints, ``keep_largest`` a bool or a list of bools; a list has one entry
    per region.  A value the kernel cannot take is a ``ValueError`` that names its key, whether the block is enabled or not."""
    pp = get_config(config, "evaluation.postprocess", {}) or {}
    R = len(list(get_config(config, "evaluation.seg.region_order", ["ET", "TC", "WT"])))
    enable = get_config(pp, "enable", False)
    if not isinstance(enable, bool):
        raise ValueError(f"evaluation.postprocess.enable must be true or false, got {enable!r}")
    conn = get_config(pp, "connectivity", 26)
    if isinstance(conn, bool) or conn not in POSTPROCESS_CONNECTIVITIES:
        raise ValueError(f"evaluation.postprocess.connectivity must be one of {list(POSTPROCESS_CONNECTIVITIES)}, got {conn!r}")

    def per_region(key: str, default, ok, what: str) -> list:
        v = get_config(pp, key, default)
        scalar = isinstance(v, (bool, int))
        vals = [v] * R if scalar else (list(v) if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else None)
        if vals is None or not all(ok(x) for x in vals):
            raise ValueError(f"evaluation.postprocess.{key} must be {what} or a list of one per region, got {v!r}")
        if len(vals) != R:
            raise ValueError(f"evaluation.postprocess.{key} has {len(vals)} entries for the {R} regions of "
                             f"evaluation.seg.region_order")
        return vals

    mv = per_region("min_voxels", 0, lambda x: isinstance(x, int) and not isinstance(x, bool) and x >= 0, "a non-negative integer")
    kl = per_region("keep_largest", False, lambda x: isinstance(x, bool), "true or false")
    return enable, int(conn), [int(v) for v in mv], [bool(v) for v in kl]


# hole filling and region nesting, the second half of the block: the defaults leave the pass out altogether
POSTPROCESS_FILL_DEFAULTS = {"fill_holes": False, "fill_connectivity": 6, "max_hole_voxels": 0, "nesting": [],
                             "nesting_mode": "clip"}
POSTPROCESS_NESTING_MODES = ops.FILL_NEST_MODES
FILL_NEST_COLUMNS = len(ops.FILL_NEST_COLUMNS)      # table columns per region: holes, filled holes, filled voxels, nested voxels


def fill_nest_config(config: Any) -> Tuple[List[bool], int, List[int], List[int], str]:
    """``evaluation.postprocess: {fill_holes, fill_connectivity, max_hole_voxels, nesting, nesting_mode}`` -> (fill_holes,
    fill_connectivity, max_hole_voxels, nesting, nesting_mode); false, 6, 0, [] and ``clip`` when absent
    (``POSTPROCESS_FILL_DEFAULTS``).  ``fill_holes`` is a bool or a list of bools, ``max_hole_voxels`` an int >= 0 or a list of
    them (0: no cap), one entry per region of ``evaluation.seg.region_order``; ``nesting`` is a list of region names,
    innermost first, returned as indices into ``region_order``.  A value the kernel cannot take is a ``ValueError`` that
    names its key, whether the block is enabled or not."""
    pp = get_config(config, "evaluation.postprocess", {}) or {}
    regions = [str(x) for x in get_config(config, "evaluation.seg.region_order", ["ET", "TC", "WT"])]
    R = len(regions)
    dflt = POSTPROCESS_FILL_DEFAULTS

    def per_region(key: str, ok, what: str) -> list:
        v = get_config(pp, key, dflt[key])
        scalar = isinstance(v, (bool, int))
        vals = [v] * R if scalar else (list(v) if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else None)
        if vals is None or not all(ok(x) for x in vals):
            raise ValueError(f"evaluation.postprocess.{key} must be {what} or a list of one per region, got {v!r}")
        if len(vals) != R:
            raise ValueError(f"evaluation.postprocess.{key} has {len(vals)} entries for the {R} regions of "
                             f"evaluation.seg.region_order")
        return vals

    fh = per_region("fill_holes", lambda x: isinstance(x, bool), "true or false")
    conn = get_config(pp, "fill_connectivity", dflt["fill_connectivity"])
    if isinstance(conn, bool) or conn not in POSTPROCESS_CONNECTIVITIES:
        raise ValueError(f"evaluation.postprocess.fill_connectivity must be one of {list(POSTPROCESS_CONNECTIVITIES)}, got {conn!r}")
    cap = per_region("max_hole_voxels", lambda x: isinstance(x, int) and not isinstance(x, bool) and x >= 0, "a non-negative integer")
    nest = get_config(pp, "nesting", dflt["nesting"])
    nest = [] if nest is None else nest
    if isinstance(nest, (str, bytes)) or not hasattr(nest, "__iter__"):
        raise ValueError(f"evaluation.postprocess.nesting must be a list of region names, innermost first, got {nest!r}")
    names = list(nest)
    if not all(isinstance(x, str) and x in regions for x in names):
        raise ValueError(f"evaluation.postprocess.nesting must name regions of evaluation.seg.region_order {regions}, got {names!r}")
    if len(names) == 1 or len(set(names)) != len(names):
        raise ValueError(f"evaluation.postprocess.nesting must be empty or at least two distinct regions, got {names!r}")
    mode = get_config(pp, "nesting_mode", dflt["nesting_mode"])
    if mode not in POSTPROCESS_NESTING_MODES:
        raise ValueError(f"evaluation.postprocess.nesting_mode must be one of {list(POSTPROCESS_NESTING_MODES)}, got {mode!r}")
    return [bool(v) for v in fh], int(conn), [int(v) for v in cap], [regions.index(x) for x in names], str(mode)


LESIONWISE_CONNECTIVITIES = ops.COMPONENT_CONNECTIVITIES
LESIONWISE_MAX_DILATION = ops.LESIONWISE_MAX_DILATION
LESIONWISE_COLUMNS = 7       # table columns per region: lw_dc, valid, lesions kept, found, false-positive, matched, predicted components


def lesionwise_config(config: Any) -> Tuple[bool, int, int, List[int]]:
    """``evaluation.lesionwise: {enable, dilation, dilation_connectivity, min_lesion_voxels}`` -> (enable, dilation,
    dilation_connectivity, min_lesion_voxels), the last as one entry per region of ``evaluation.seg.region_order``; off, 3,
    18 and 0 when absent.  ``min_lesion_voxels`` is an int or a list of one int per region.  A value the kernel cannot take
    is a ``ValueError`` that names its key, whether the block is enabled or not."""
    lw = get_config(config, "evaluation.lesionwise", {}) or {}
    R = len(list(get_config(config, "evaluation.seg.region_order", ["ET", "TC", "WT"])))
    enable = get_config(lw, "enable", False)
    if not isinstance(enable, bool):
        raise ValueError(f"evaluation.lesionwise.enable must be true or false, got {enable!r}")
    dil = get_config(lw, "dilation", 3)
    if isinstance(dil, bool) or not isinstance(dil, int) or not 0 <= dil <= LESIONWISE_MAX_DILATION:
        raise ValueError(f"evaluation.lesionwise.dilation must be an integer in 0 ... {LESIONWISE_MAX_DILATION}, got {dil!r}")
    conn = get_config(lw, "dilation_connectivity", 18)
    if isinstance(conn, bool) or conn not in LESIONWISE_CONNECTIVITIES:
        raise ValueError(f"evaluation.lesionwise.dilation_connectivity must be one of {list(LESIONWISE_CONNECTIVITIES)}, "
                         f"got {conn!r}")
    v = get_config(lw, "min_lesion_voxels", 0)
    scalar = isinstance(v, (bool, int))
    vals = [v] * R if scalar else (list(v) if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else None)
    if vals is None or not all(isinstance(x, int) and not isinstance(x, bool) and x >= 0 for x in vals):
        raise ValueError(f"evaluation.lesionwise.min_lesion_voxels must be a non-negative integer or a list of one per region, "
                         f"got {v!r}")
    if len(vals) != R:
        raise ValueError(f"evaluation.lesionwise.min_lesion_voxels has {len(vals)} entries for the {R} regions of "
                         f"evaluation.seg.region_order")
    return enable, int(dil), int(conn), [int(x) for x in vals]


def lesionwise_columns(stats: torch.Tensor) -> torch.Tensor:
    """stats int64 [R,7] of one volume (``ops.LESIONWISE_COLUMNS``) -> its table columns float64 [7*R]: lw_dc[R], valid[R],
    lesions kept[R], lesions found[R], false-positive components[R], matched components[R], predicted components[R].

        lw_dc = dice_q / 2^30 / (lesions kept + false-positive components),   valid = that denominator > 0

    ``dice_q`` is an integer beyond what a double of the table could carry across a sum, so the volume's score is formed
    here, from the integers, and only small counts travel beside it."""
    s = stats.to(torch.int64)
    kept, found, pred, matched = s[:, 1], s[:, 2], s[:, 3], s[:, 4]
    fp = pred - matched
    den = kept + fp
    valid = den > 0
    safe = torch.where(valid, den, torch.ones_like(den)).to(torch.float64)
    lw = torch.where(valid, s[:, 5].to(torch.float64) / float(ops.LESIONWISE_Q_ONE) / safe, torch.zeros_like(safe))
    return torch.cat([lw, valid.to(torch.float64)] + [c.to(torch.float64) for c in (kept, found, fp, matched, pred)])


LESIONWISE_HD95_COLUMNS = 2  # table columns per region: lw_hd95, state (1 valid, 0 undefined, -1 the region's surface lists overflowed)


def lesionwise_hd95_config(config: Any) -> Tuple[bool, float, Any]:
    """``evaluation.lesionwise.hd95: {enable, percentile, penalty}`` -> (enable, percentile, penalty); off, 95.0 and
    ``"diagonal"`` when absent.  ``penalty`` is what a missed lesion and a false-positive component cost: ``diagonal`` (the
    volume diagonal in mm, the penalty of ``evaluation.surface``) or a positive number (BraTS-2023 uses 374).  A bad value is
    a ``ValueError`` that names its key, whether the block is enabled or not; so is ``hd95.enable`` without
    ``evaluation.lesionwise.enable``."""
    lw = get_config(config, "evaluation.lesionwise", {}) or {}
    hd = get_config(lw, "hd95", {}) or {}
    enable = get_config(hd, "enable", False)
    if not isinstance(enable, bool):
        raise ValueError(f"evaluation.lesionwise.hd95.enable must be true or false, got {enable!r}")
    pct = get_config(hd, "percentile", 95.0)
    if isinstance(pct, bool) or not isinstance(pct, (int, float)) or not 0.0 <= float(pct) <= 100.0:
        raise ValueError(f"evaluation.lesionwise.hd95.percentile must be a number in [0, 100], got {pct!r}")
    pen = get_config(hd, "penalty", "diagonal")
    if isinstance(pen, str):
        if pen != "diagonal":
            raise ValueError(f"evaluation.lesionwise.hd95.penalty must be 'diagonal' or a positive number, got {pen!r}")
    elif isinstance(pen, bool) or not isinstance(pen, (int, float)) or not (math.isfinite(float(pen)) and float(pen) > 0.0):
        raise ValueError(f"evaluation.lesionwise.hd95.penalty must be 'diagonal' or a positive number, got {pen!r}")
    else:
        pen = float(pen)
    if enable and get_config(lw, "enable", False) is not True:
        raise ValueError("evaluation.lesionwise.hd95.enable needs evaluation.lesionwise.enable: the HD95 pass reads what the "
                         "lesion-wise Dice pass leaves on the device")
    return enable, float(pct), pen


def volume_diagonal_mm(shape: Sequence[int], spacing: Sequence[float]) -> float:
    """The diagonal of a D x H x W volume in mm, between the centres of its corner voxels (reference
    src/evaluation/seg_eval.py:89-103): the penalty of the surface metrics."""
    D, H, W = (int(v) for v in shape)
    sd, sh, sw = spacing
    dd, hh, ww = max(D - 1, 0) * sd, max(H - 1, 0) * sh, max(W - 1, 0) * sw
    return float(math.sqrt(dd * dd + hh * hh + ww * ww))


def lesionwise_hd95_columns(stats: torch.Tensor, hd_stats: torch.Tensor, penalty: float) -> torch.Tensor:
    """stats int64 [R,7] (``ops.LESIONWISE_COLUMNS``) and hd_stats int64 [R,3] (``ops.LESIONWISE_HD_COLUMNS``) of one volume
    -> its table columns float64 [2*R]: lw_hd95[R], state[R].

        lw_hd95 = (hd_q / 2^20 + penalty ((kept - found) + false-positive components)) / (kept + false-positive components)

    state is 1 where that denominator is > 0 (a GT-empty region with false positives IS scored, with the penalty), 0 where
    there is nothing to find and nothing predicted, and -1 where the region's surface lists overflowed on the device: then
    the score reads 0, stays out of the mean and the volume is counted under ``*_lw_hd95_overflow``."""
    s, h = stats.to(torch.int64), hd_stats.to(torch.int64)
    kept, found, pred, matched = s[:, 1], s[:, 2], s[:, 3], s[:, 4]
    fp = pred - matched
    den = kept + fp
    over = h[:, 2] > 0
    valid = (den > 0) & ~over
    safe = torch.where(den > 0, den, torch.ones_like(den)).to(torch.float64)
    num = h[:, 0].to(torch.float64) / float(ops.LESIONWISE_HD_Q_ONE) + float(penalty) * ((kept - found) + fp).to(torch.float64)
    lw = torch.where(valid, num / safe, torch.zeros_like(safe))
    state = torch.where(over, -torch.ones_like(safe), valid.to(torch.float64))
    return torch.cat([lw, state])


NSD_MAX_TOLERANCES = ops.SURFACE_DICE_MAX_TOLERANCES


def _nsd_block(config: Any, block: Any, key: str, default: Sequence[float]) -> Tuple[bool, List[float]]:
    """``{enable, tolerances}`` of an NSD block named ``key`` -> (enable, tolerances in mm).  1 ... 4 distinct tolerances, each
    finite and >= 0: checked whether the block is enabled or not.  An enabled block's search window at
    ``evaluation.seg.spacing`` must stay within 8 voxels per axis as well; the window depends on the spacing, so a disabled
    block - the shipped configs carry one, with the default tolerances - never stands in the way of an evaluation at a fine
    spacing."""
    enable = get_config(block, "enable", False)
    if not isinstance(enable, bool):
        raise ValueError(f"{key}.enable must be true or false, got {enable!r}")
    tol = get_config(block, "tolerances", None)
    tol = list(default) if tol is None else tol
    vals = list(tol) if hasattr(tol, "__iter__") and not isinstance(tol, (str, bytes)) else None
    if (vals is None or not 1 <= len(vals) <= NSD_MAX_TOLERANCES or
            not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(float(v)) and float(v) >= 0.0
                    for v in vals)):
        raise ValueError(f"{key}.tolerances must be a list of 1 ... {NSD_MAX_TOLERANCES} finite numbers >= 0 (mm), got {tol!r}")
    vals = [float(v) for v in vals]
    names = [nsd_suffix(v) for v in vals]
    if len(set(names)) != len(names):
        raise ValueError(f"{key}.tolerances must be distinct (their metric keys {names} collide), got {tol!r}")
    sp = get_config(config, "evaluation.seg.spacing", [1.0, 1.0, 1.0])
    sp = [float(v) for v in sp] if sp is not None else [1.0, 1.0, 1.0]
    if enable and len(sp) == 3 and all(math.isfinite(v) and v > 0.0 for v in sp):
        rad = ops.surface_dice_radius(sp, max(vals))
        if max(rad) > ops.SURFACE_DICE_MAX_RADIUS:
            raise ValueError(f"{key}.tolerances {vals} need a search window of more than {ops.SURFACE_DICE_MAX_RADIUS} voxels at "
                             f"evaluation.seg.spacing {sp}; evaluation.surface (HD95 / ASD), whose distance transform is exact "
                             f"at any distance, is the tool for large distances")
    return enable, vals


def nsd_suffix(tolerance: float) -> str:
    """The tolerance as the metric keys carry it: ``%g`` (0.5 -> ``0.5``, 1.0 -> ``1``)."""
    return "%g" % float(tolerance)


def surface_dice_config(config: Any) -> Tuple[bool, List[float]]:
    """``evaluation.surface_dice: {enable, tolerances}`` -> (enable, tolerances); off and [1.0] when absent.  A bad value is a
    ``ValueError`` that names its key, whether the block is enabled or not."""
    return _nsd_block(config, get_config(config, "evaluation.surface_dice", {}) or {}, "evaluation.surface_dice", [1.0])


def lesionwise_nsd_config(config: Any) -> Tuple[bool, List[float]]:
    """``evaluation.lesionwise.nsd: {enable, tolerances}`` -> (enable, tolerances); off and [0.5, 1.0] (BraTS-2024) when
    absent.  A bad value is a ``ValueError`` that names its key, whether the block is enabled or not; so is ``nsd.enable``
    without ``evaluation.lesionwise.enable``."""
    lw = get_config(config, "evaluation.lesionwise", {}) or {}
    enable, tol = _nsd_block(config, get_config(lw, "nsd", {}) or {}, "evaluation.lesionwise.nsd", [0.5, 1.0])
    if enable and get_config(lw, "enable", False) is not True:
        raise ValueError("evaluation.lesionwise.nsd.enable needs evaluation.lesionwise.enable: the NSD pass reads what the "
                         "lesion-wise Dice pass leaves on the device")
    return enable, tol


def surface_dice_columns(counts: torch.Tensor) -> torch.Tensor:
    """counts int64 [R,T,4] of one volume (``ops.SURFACE_DICE_COLUMNS``) -> its table columns float64 [T*R], one tolerance's
    regions after another:

        NSD = (hits P->G + hits G->P) / (|edge P| + |edge G|),   0 where both surfaces are empty

    A region counts iff its ground truth is non-empty - the ``valid`` column of Dice, which the table already carries."""
    c = counts.to(torch.int64)
    num, den = c[..., 0] + c[..., 2], c[..., 1] + c[..., 3]
    safe = torch.where(den > 0, den, torch.ones_like(den)).to(torch.float64)
    nsd = torch.where(den > 0, num.to(torch.float64) / safe, torch.zeros_like(safe))
    return nsd.t().reshape(-1)


def lesionwise_nsd_columns(stats: torch.Tensor, nsd_stats: torch.Tensor) -> torch.Tensor:
    """stats int64 [R,7] (``ops.LESIONWISE_COLUMNS``) and nsd_stats int64 [R,T] of one volume -> its table columns float64
    [T*R], one tolerance's regions after another:

        lw_nsd = nsd_q / 2^30 / (lesions kept + false-positive components),   0 where that denominator is 0

    valid where the denominator is > 0: the ``valid`` column of ``lesionwise_columns``, which the table already carries."""
    s, q = stats.to(torch.int64), nsd_stats.to(torch.int64)
    den = s[:, 1] + (s[:, 3] - s[:, 4])
    safe = torch.where(den > 0, den, torch.ones_like(den)).to(torch.float64)
    lw = torch.where((den > 0)[:, None], q.to(torch.float64) / float(ops.LESIONWISE_NSD_Q_ONE) / safe[:, None],
                     torch.zeros_like(q, dtype=torch.float64))
    return lw.t().reshape(-1)


def calibration_from_bins(table: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The table of ``ops.calibration_bins`` (float64 [..., 3*bins + 2]: per bin count, sum of confidence, correct count;
    then the Brier sum, then the NLL sum) -> (ece, brier, nll, valid), float64 / bool of the leading shape.

        ECE = sum_b (n_b / n) |correct_b / n_b - conf_b / n_b|,   Brier = sum / n,   NLL = sum / n,   valid = n > 0

    An entry without elements (``scope: union`` where neither the prediction nor the ground truth has foreground) is
    invalid and reads 0; it stays out of the means like a Dice with an empty ground truth."""
    t = table.to(torch.float64)
    bins = (t.shape[-1] - 2) // 3
    if bins < 1 or 3 * bins + 2 != t.shape[-1]:
        raise ValueError(f"calibration table rows must hold 3*bins + 2 entries, got {t.shape[-1]}")
    per = t[..., :3 * bins].reshape(*t.shape[:-1], bins, 3)
    cnt, conf, cor = per[..., 0], per[..., 1], per[..., 2]
    n = cnt.sum(-1)
    valid = n > 0
    safe = torch.where(valid, n, torch.ones_like(n))
    # (n_b / n) |correct_b / n_b - conf_b / n_b| = |correct_b - conf_b| / n: an empty bin adds nothing
    ece = (cor - conf).abs().sum(-1) / safe
    brier = t[..., 3 * bins] / safe
    nll = t[..., 3 * bins + 1] / safe
    zero = torch.zeros_like(n)
    return torch.where(valid, ece, zero), torch.where(valid, brier, zero), torch.where(valid, nll, zero), valid


def calibration_width(bins: int, rout: int) -> int:
    """Doubles a volume's calibration adds to its table row."""
    return int(rout) * (3 * int(bins) + 2) if bins else 0


class RegionAccumulator:
    """float64 sums / counts per region, overall and per domain (reference seg_eval.py:250-270,363-378).  ``bins`` > 0
    adds the calibration figures: ``calibration_regions`` names their rows (default: the regions; ``["all"]`` for a softmax
    head), ``reliability`` pools the bins of every row.  ``components`` adds the connected-component figures of the
    post-processing: per-volume means over ALL volumes of components found, components kept and voxels removed.
    ``lesionwise`` adds the lesion-wise figures: the lesion-wise Dice averaged over the volumes where it is defined (a
    GT-empty region with false-positive components IS one of them, with 0), per-volume means of kept lesions, found
    lesions and false-positive components, and recall / precision pooled over all volumes.  ``fill_nest`` adds the figures
    of the hole filling and nesting pass: per-volume means over all volumes of holes, filled holes, filled voxels and voxels
    the nesting changed.  ``lesionwise_hd95`` adds the lesion-wise HD95 averaged over the volumes where it is defined and did
    not overflow, and the per-volume mean of overflowed volumes."""

    def __init__(self, region_order: Sequence[str], surface: bool = False, bins: int = 0,
                 calibration_regions: Optional[Sequence[str]] = None, components: bool = False, lesionwise: bool = False,
                 fill_nest: bool = False, lesionwise_hd95: bool = False, surface_dice: Sequence[float] = (),
                 lesionwise_nsd: Sequence[float] = ()):
        self.regions = list(region_order)
        # NSD: the tolerances (mm) of the region-wise and of the lesion-wise figure; empty = off.  Sums and counts [2, T, R]
        self.surface_dice = [float(t) for t in surface_dice]
        self.lesionwise_nsd = [float(t) for t in lesionwise_nsd]
        nR = len(self.regions)
        self._zsd = lambda: torch.zeros((2, len(self.surface_dice), nR), dtype=torch.float64)
        self.sd_tot = self._zsd()
        self.sd_dom: Dict[str, torch.Tensor] = defaultdict(self._zsd)
        self._zln = lambda: torch.zeros((2, len(self.lesionwise_nsd), nR), dtype=torch.float64)
        self.ln_tot = self._zln()
        self.ln_dom: Dict[str, torch.Tensor] = defaultdict(self._zln)
        self.surface = bool(surface)
        R = len(self.regions)
        self._z = lambda: torch.zeros(R, dtype=torch.float64)
        # sum_dice, cnt_dice, sum_iou, cnt_iou, then (surface) sum_hd95, cnt_hd95, sum_asd, cnt_asd
        self.tot = [self._z() for _ in range(8)]
        self.dom: Dict[str, List[torch.Tensor]] = defaultdict(lambda: [self._z() for _ in range(8)])
        self.total_loss, self.n_samples = 0.0, 0
        self.bins = int(bins)
        self.cal_regions = list(calibration_regions) if calibration_regions is not None else list(self.regions)
        Rc = len(self.cal_regions)
        self._zc = lambda: torch.zeros((4, Rc), dtype=torch.float64)         # sum_ece, sum_brier, sum_nll, count
        self.cal_tot = self._zc()
        self.cal_dom: Dict[str, torch.Tensor] = defaultdict(self._zc)
        self.reliability = torch.zeros((Rc, max(self.bins, 0), 3), dtype=torch.float64)
        self.components = bool(components)
        self._zp = lambda: torch.zeros((4, R), dtype=torch.float64)          # sum_components, sum_kept, sum_removed, volumes
        self.pp_tot = self._zp()
        self.pp_dom: Dict[str, torch.Tensor] = defaultdict(self._zp)
        self.lesionwise = bool(lesionwise)
        # the 7 table columns summed (lw_dc, valid, kept, found, false-positive, matched, predicted), then the volumes
        self._zl = lambda: torch.zeros((LESIONWISE_COLUMNS + 1, R), dtype=torch.float64)
        self.lw_tot = self._zl()
        self.lw_dom: Dict[str, torch.Tensor] = defaultdict(self._zl)
        self.lesionwise_hd95 = bool(lesionwise_hd95)
        self._zh = lambda: torch.zeros((4, R), dtype=torch.float64)          # sum_lw_hd95, valid volumes, overflowed volumes, volumes
        self.lh_tot = self._zh()
        self.lh_dom: Dict[str, torch.Tensor] = defaultdict(self._zh)
        self.fill_nest = bool(fill_nest)
        self._zf = lambda: torch.zeros((FILL_NEST_COLUMNS + 1, R), dtype=torch.float64)      # the 4 columns summed, then the volumes
        self.fn_tot = self._zf()
        self.fn_dom: Dict[str, torch.Tensor] = defaultdict(self._zf)

    def add_fill_nest(self, stats: Any, domain: str) -> None:
        """One volume's fill / nest figures, [4*R] as the table holds them: holes[R], filled holes[R], filled voxels[R],
        nested voxels[R]."""
        st = torch.as_tensor(stats, dtype=torch.float64).reshape(FILL_NEST_COLUMNS, len(self.regions))
        for acc in (self.fn_tot, self.fn_dom[domain]):
            acc[:FILL_NEST_COLUMNS] += st
            acc[FILL_NEST_COLUMNS] += 1.0

    def _fill_nest_keys(self, out: Dict[str, float], prefix: str, acc: torch.Tensor) -> None:
        for row, key in enumerate(ops.FILL_NEST_COLUMNS):
            for name, v in zip(self.regions, self._fin(acc[row], acc[FILL_NEST_COLUMNS])):
                out[f"{prefix}{name.lower()}_{key}"] = v

    def add_lesionwise(self, cols: Any, domain: str) -> None:
        """One volume's lesion-wise columns, [7*R] as the table holds them (``lesionwise_columns``)."""
        c = torch.as_tensor(cols, dtype=torch.float64).reshape(LESIONWISE_COLUMNS, len(self.regions))
        for acc in (self.lw_tot, self.lw_dom[domain]):
            acc[0] += c[0] * c[1]
            acc[1:LESIONWISE_COLUMNS] += c[1:]
            acc[LESIONWISE_COLUMNS] += 1.0

    def _lesionwise_keys(self, out: Dict[str, float], prefix: str, acc: torch.Tensor) -> None:
        means = self._fin(acc[0], acc[1])
        for name, v in zip(self.regions, means):
            out[f"{prefix}{name.lower()}_lw_dc"] = v
        out[f"{prefix}avg_lw_dc"] = self._avg(means, acc[1])
        for row, key in ((2, "lesions"), (3, "lesions_found"), (4, "fp_components")):
            for name, v in zip(self.regions, self._fin(acc[row], acc[LESIONWISE_COLUMNS])):
                out[f"{prefix}{name.lower()}_{key}"] = v
        for k, name in enumerate(self.regions):       # pooled over the volumes; absent where there is nothing to divide by
            if acc[2][k] > 0:
                out[f"{prefix}{name.lower()}_lesion_recall"] = float((acc[3][k] / acc[2][k]).item())
            if acc[6][k] > 0:
                out[f"{prefix}{name.lower()}_lesion_precision"] = float((acc[5][k] / acc[6][k]).item())

    def add_lesionwise_hd95(self, cols: Any, domain: str) -> None:
        """One volume's lesion-wise HD95 columns, [2*R] as the table holds them (``lesionwise_hd95_columns``)."""
        c = torch.as_tensor(cols, dtype=torch.float64).reshape(LESIONWISE_HD95_COLUMNS, len(self.regions))
        ok, over = (c[1] > 0.5).to(torch.float64), (c[1] < -0.5).to(torch.float64)
        for acc in (self.lh_tot, self.lh_dom[domain]):
            acc[0] += c[0] * ok
            acc[1] += ok
            acc[2] += over
            acc[3] += 1.0

    def _lesionwise_hd95_keys(self, out: Dict[str, float], prefix: str, acc: torch.Tensor) -> None:
        means = self._fin(acc[0], acc[1])
        for name, v in zip(self.regions, means):
            out[f"{prefix}{name.lower()}_lw_hd95"] = v
        out[f"{prefix}avg_lw_hd95"] = self._avg(means, acc[1])
        for name, v in zip(self.regions, self._fin(acc[2], acc[3])):
            out[f"{prefix}{name.lower()}_lw_hd95_overflow"] = v

    def add_surface_dice(self, cols: Any, valid: Sequence[bool], domain: str) -> None:
        """One volume's NSD columns, [T*R] as the table holds them (``surface_dice_columns``); ``valid`` is Dice's."""
        c = torch.as_tensor(cols, dtype=torch.float64).reshape(len(self.surface_dice), len(self.regions))
        ok = torch.tensor([1.0 if bool(v) else 0.0 for v in valid], dtype=torch.float64)
        for acc in (self.sd_tot, self.sd_dom[domain]):
            acc[0] += c * ok
            acc[1] += ok

    def add_lesionwise_nsd(self, cols: Any, lesionwise: Any, domain: str) -> None:
        """One volume's lesion-wise NSD columns, [T*R] as the table holds them (``lesionwise_nsd_columns``); defined where the
        volume's lesion-wise Dice is (the ``valid`` row of its ``lesionwise_columns``)."""
        c = torch.as_tensor(cols, dtype=torch.float64).reshape(len(self.lesionwise_nsd), len(self.regions))
        ok = torch.as_tensor(lesionwise, dtype=torch.float64).reshape(LESIONWISE_COLUMNS, len(self.regions))[1]
        for acc in (self.ln_tot, self.ln_dom[domain]):
            acc[0] += c * ok
            acc[1] += ok

    def _nsd_keys(self, out: Dict[str, float], prefix: str, acc: torch.Tensor, tolerances: Sequence[float], stem: str) -> None:
        for t, tau in enumerate(tolerances):
            means = self._fin(acc[0][t], acc[1][t])
            for name, v in zip(self.regions, means):
                out[f"{prefix}{name.lower()}_{stem}_{nsd_suffix(tau)}"] = v
            out[f"{prefix}avg_{stem}_{nsd_suffix(tau)}"] = self._avg(means, acc[1][t])

    def add_components(self, stats: Any, domain: str) -> None:
        """One volume's component figures, [3*R] as the table holds them: components[R], kept[R], removed voxels[R]."""
        st = torch.as_tensor(stats, dtype=torch.float64).reshape(3, len(self.regions))
        for acc in (self.pp_tot, self.pp_dom[domain]):
            acc[:3] += st
            acc[3] += 1.0

    def _component_keys(self, out: Dict[str, float], prefix: str, acc: torch.Tensor) -> None:
        for row, key in enumerate(("components", "kept_components", "removed_voxels")):
            means = self._fin(acc[row], acc[3])
            for name, v in zip(self.regions, means):
                out[f"{prefix}{name.lower()}_{key}"] = v
            if row == 0:
                out[f"{prefix}avg_components"] = self._avg(means, acc[3])

    def add_calibration(self, raw: torch.Tensor, domain: str) -> None:
        """One volume's table, float64 [Rout, 3*bins + 2] (or flat)."""
        raw = raw.to(torch.float64).reshape(len(self.cal_regions), 3 * self.bins + 2)
        ece, brier, nll, valid = calibration_from_bins(raw)
        ok = valid.to(torch.float64)
        for acc in (self.cal_tot, self.cal_dom[domain]):
            acc[0] += ece * ok
            acc[1] += brier * ok
            acc[2] += nll * ok
            acc[3] += ok
        self.reliability += raw[:, :3 * self.bins].reshape(-1, self.bins, 3)

    def _calibration_keys(self, out: Dict[str, float], prefix: str, acc: torch.Tensor) -> None:
        for row, key in enumerate(("ece", "brier", "nll")):
            means = self._fin(acc[row], acc[3])
            for name, v in zip(self.cal_regions, means):
                out[f"{prefix}{name.lower()}_{key}"] = v
            out[f"{prefix}avg_{key}"] = self._avg(means, acc[3])

    def add_row(self, dice: Sequence[float], iou: Sequence[float], valid: Sequence[bool], domain: str,
                hd95: Optional[Sequence[float]] = None, asd: Optional[Sequence[float]] = None,
                calibration: Optional[torch.Tensor] = None, components: Any = None, lesionwise: Any = None,
                fill_nest: Any = None, lesionwise_hd95: Any = None, surface_dice: Any = None,
                lesionwise_nsd: Any = None) -> None:
        d = self.dom[domain]
        if self.surface_dice:
            self.add_surface_dice(surface_dice, valid, domain)
        if self.lesionwise_nsd:
            self.add_lesionwise_nsd(lesionwise_nsd, lesionwise, domain)
        if self.components:
            self.add_components(components, domain)
        if self.fill_nest:
            self.add_fill_nest(fill_nest, domain)
        if self.lesionwise:
            self.add_lesionwise(lesionwise, domain)
        if self.lesionwise_hd95:
            self.add_lesionwise_hd95(lesionwise_hd95, domain)
        if self.bins:
            self.add_calibration(calibration, domain)
        for c in range(len(self.regions)):
            if bool(valid[c]):
                dv, iv = float(dice[c]), float(iou[c])
                for acc in (self.tot, d):
                    acc[0][c] += dv
                    acc[1][c] += 1.0
                    acc[2][c] += iv
                    acc[3][c] += 1.0
                if self.surface:
                    hv, av = float(hd95[c]), float(asd[c])
                    for acc in (self.tot, d):
                        acc[4][c] += hv
                        acc[5][c] += 1.0
                        acc[6][c] += av
                        acc[7][c] += 1.0

    def add_loss(self, loss: float, batch: int) -> None:
        self.total_loss += float(loss) * batch
        self.n_samples += batch

    @staticmethod
    def _fin(s: torch.Tensor, c: torch.Tensor) -> List[float]:
        return [float((s[k] / c[k]).item()) if c[k] > 0 else 0.0 for k in range(len(s))]

    @staticmethod
    def _avg(means: List[float], cnt: torch.Tensor) -> float:
        ok = [k for k in range(len(means)) if cnt[k] > 0]
        return float(sum(means[k] for k in ok) / max(1, len(ok)))

    def metrics(self, report_loss: bool) -> Dict[str, float]:
        md, mi = self._fin(self.tot[0], self.tot[1]), self._fin(self.tot[2], self.tot[3])
        out: Dict[str, float] = {}
        for name, v in zip(self.regions, md):
            out[f"{name.lower()}_dc"] = v
        out["avg_dc"] = self._avg(md, self.tot[1])
        out["miou"] = self._avg(mi, self.tot[3])
        out["jc"] = out["miou"]
        out["loss"] = float(self.total_loss / max(1, self.n_samples)) if report_loss else 0.0
        if self.surface:        # reference seg_eval.py:424-440
            self._surface_keys(out, "", self.tot)
        if self.components:
            self._component_keys(out, "", self.pp_tot)
        if self.fill_nest:
            self._fill_nest_keys(out, "", self.fn_tot)
        if self.lesionwise:
            self._lesionwise_keys(out, "", self.lw_tot)
        if self.lesionwise_hd95:
            self._lesionwise_hd95_keys(out, "", self.lh_tot)
        if self.lesionwise_nsd:
            self._nsd_keys(out, "", self.ln_tot, self.lesionwise_nsd, "lw_nsd")
        if self.surface_dice:
            self._nsd_keys(out, "", self.sd_tot, self.surface_dice, "nsd")
        if self.bins:
            self._calibration_keys(out, "", self.cal_tot)
        for dom in sorted(self.dom.keys()):
            sd, cd, si, ci = self.dom[dom][:4]
            safe = dom if dom != "" else "unknown"
            dm, dim_ = self._fin(sd, cd), self._fin(si, ci)
            for name, v in zip(self.regions, dm):
                out[f"dom/{safe}/{name.lower()}_dc"] = v
            out[f"dom/{safe}/avg_dc"] = self._avg(dm, cd)
            out[f"dom/{safe}/miou"] = self._avg(dim_, ci)
            if self.surface:    # reference seg_eval.py:459-476
                self._surface_keys(out, f"dom/{safe}/", self.dom[dom])
            if self.components:
                self._component_keys(out, f"dom/{safe}/", self.pp_dom[dom])
            if self.fill_nest:
                self._fill_nest_keys(out, f"dom/{safe}/", self.fn_dom[dom])
            if self.lesionwise:
                self._lesionwise_keys(out, f"dom/{safe}/", self.lw_dom[dom])
            if self.lesionwise_hd95:
                self._lesionwise_hd95_keys(out, f"dom/{safe}/", self.lh_dom[dom])
            if self.lesionwise_nsd:
                self._nsd_keys(out, f"dom/{safe}/", self.ln_dom[dom], self.lesionwise_nsd, "lw_nsd")
            if self.surface_dice:
                self._nsd_keys(out, f"dom/{safe}/", self.sd_dom[dom], self.surface_dice, "nsd")
            if self.bins:
                self._calibration_keys(out, f"dom/{safe}/", self.cal_dom[dom])
        return out

    def _surface_keys(self, out: Dict[str, float], prefix: str, acc: List[torch.Tensor]) -> None:
        mh, ma = self._fin(acc[4], acc[5]), self._fin(acc[6], acc[7])
        for name, v in zip(self.regions, mh):
            out[f"{prefix}{name.lower()}_hd95"] = v
        out[f"{prefix}avg_hd95"] = self._avg(mh, acc[5])
        for name, v in zip(self.regions, ma):
            out[f"{prefix}{name.lower()}_asd"] = v
        out[f"{prefix}avg_asd"] = self._avg(ma, acc[7])


class DiceCEReport:
    """monai DiceCELoss(sigmoid=True, ...) value for ``report_loss`` from the HIP sums kernel
    (reference seg_eval.py:198-220,395-400)."""

    def __init__(self, crit_cfg: Any):
        crit_cfg = as_cfg(crit_cfg)
        self.include_background = bool(get_config(crit_cfg, "include_background", True))
        self.squared_pred = bool(get_config(crit_cfg, "squared_pred", False))
        self.jaccard = bool(get_config(crit_cfg, "jaccard", False))
        self.lambda_dice = float(get_config(crit_cfg, "lambda_dice", 1.0))
        self.lambda_ce = float(get_config(crit_cfg, "lambda_ce", 1.0))
        w = get_config(crit_cfg, "weight", None)
        self.weight = [float(x) for x in list(w)] if w is not None and len(list(w)) > 0 else None
        self._w_dev: Optional[torch.Tensor] = None

    def launch(self, logits: torch.Tensor, label: torch.Tensor, channels_last: bool = False):
        """Queue the sums kernel on the current stream; ``value`` turns the result into the loss later (one host sync)."""
        B, R = (logits.shape[0], logits.shape[-1]) if channels_last else logits.shape[:2]
        nvox = logits.numel() // (B * R)
        if self.weight is not None and self._w_dev is None:
            if len(self.weight) != R:
                raise ValueError(f"criterion.weight has {len(self.weight)} entries for {R} channels")
            self._w_dev = torch.tensor(self.weight, dtype=torch.float32, device=logits.device)
        out = torch.empty(B * (R * 3 + 1), dtype=torch.float64, device=logits.device)
        ops.dice_ce_sums(logits, label, self._w_dev, self.squared_pred, out, logits_channels_last=channels_last)
        return out, B, R, nvox

    def value(self, pending) -> float:
        out, B, R, nvox = pending
        s = out.cpu().view(B, R * 3 + 1)
        per = s[:, :R * 3].view(B, R, 3).to(torch.float32)
        inter, ps, gs = per[..., 0], per[..., 1], per[..., 2]
        if not self.include_background and R > 1:
            inter, ps, gs = inter[:, 1:], ps[:, 1:], gs[:, 1:]
        den = gs + ps
        if self.jaccard:
            den = 2.0 * (den - inter)
        f = 1.0 - (2.0 * inter + 1e-5) / (den + 1e-5)
        if self.weight is not None and f.shape[1] != 1:
            dw = torch.tensor(self.weight[1:] if not self.include_background else self.weight, dtype=torch.float32)
            if dw.numel() == f.shape[1]:
                f = f * dw
        dice = float(f.mean().item())
        ce = float((s[:, R * 3].sum() / (B * nvox * (R if R == 1 else 1))).item())
        return self.lambda_dice * dice + self.lambda_ce * ce

    def values_per_volume(self, pending) -> List[float]:
        """The same loss for every volume of the batch on its own (reduction 'mean' makes the batch value their mean):
        what a rank contributes per row to the gathered table."""
        out, B, R, nvox = pending
        return [self.value((out.view(B, R * 3 + 1)[b:b + 1].reshape(-1), 1, R, nvox)) for b in range(B)]

    def __call__(self, logits: torch.Tensor, label: torch.Tensor, channels_last: bool = False) -> float:
        return self.value(self.launch(logits, label, channels_last))


# ----------------------------------------------------------------------------- seg_eval
@register_evaluation_strategy("seg_eval")
class SegmentationEvaluationStrategy:
    def __init__(self, config: Any = None):
        self.config = as_cfg(config)
        seg = get_config(self.config, "evaluation.seg", {}) or {}
        self.threshold = float(get_config(seg, "threshold", 0.5))
        self.region_order = list(get_config(seg, "region_order", ["ET", "TC", "WT"]))
        sp = get_config(seg, "spacing", [1.0, 1.0, 1.0])
        sp = list(sp) if sp is not None else [1.0, 1.0, 1.0]
        if len(sp) != 3:
            raise ValueError(f"[BratsSegEval] evaluation.seg.spacing must have length 3, got {sp}")
        self.spacing = tuple(float(v) for v in sp)
        self.report_loss = bool(get_config(self.config, "evaluation.loss.report_loss", False))
        # HD95 / ASD, off by default like the reference (src/evaluation/seg_eval.py:193-196)
        surf = get_config(self.config, "evaluation.surface", {}) or {}
        self.enable_surface = bool(get_config(surf, "enable", False))
        self.asd_symmetric = bool(get_config(surf, "asd_symmetric", False))
        self.loss_fn = DiceCEReport(get_config(self.config, "training.criterion", {}) or {})
        # ECE / Brier / NLL from a reliability histogram taken on the GPU, off by default.  The head follows
        # `training.criterion.softmax` as the plugins do: one table row per region, or the single row "all"
        self.enable_calibration, self.calibration_bins, self.calibration_scope = calibration_config(self.config)
        self.calibration_softmax = bool(get_config(self.config, "training.criterion.softmax", False))
        self.calibration_regions = ["all"] if self.calibration_softmax else list(self.region_order)
        self.last_reliability: Optional[torch.Tensor] = None
        # connected-component filtering of the thresholded mask on the GPU, off by default: small components dropped,
        # optionally only the largest kept, per region; Dice, the surface distances and the gathered masks then describe
        # the filtered mask (calibration and the reported loss stay on the logits)
        (self.enable_postprocess, self.postprocess_connectivity, self.postprocess_min_voxels,
         self.postprocess_keep_largest) = postprocess_config(self.config)
        self._stats: Optional[torch.Tensor] = None
        # hole filling and ET < TC < WT nesting of the filtered mask, in place right after the filter; the pass is queued
        # only when post-processing is on and a region fills or a chain is given, and only then do its keys appear
        (self.postprocess_fill_holes, self.postprocess_fill_connectivity, self.postprocess_max_hole_voxels,
         self.postprocess_nesting, self.postprocess_nesting_mode) = fill_nest_config(self.config)
        self.enable_fill_nest = self.enable_postprocess and (any(self.postprocess_fill_holes) or bool(self.postprocess_nesting))
        self._fill: Optional[torch.Tensor] = None
        # lesion-wise Dice and detection counts on the GPU, off by default: ground-truth lesions (dilated, 26-connected)
        # against the predicted components of the mask that is scored (the filtered one with post-processing on)
        (self.enable_lesionwise, self.lesionwise_dilation, self.lesionwise_connectivity,
         self.lesionwise_min_voxels) = lesionwise_config(self.config)
        if self.enable_lesionwise and bool(get_config(self.config, "training.criterion.softmax", False)):
            raise NotImplementedError("evaluation.lesionwise.enable: lesion-wise scores are defined for the sigmoid-region head "
                                      "only (training.criterion.softmax is set)")
        self._lw: Optional[torch.Tensor] = None
        # lesion-wise HD95 on top of that, off by default: one more pass behind the lesion-wise scores, on their scratch
        (self.enable_lesionwise_hd95, self.lesionwise_hd95_percentile,
         self.lesionwise_hd95_penalty) = lesionwise_hd95_config(self.config)
        self._lwhd: Optional[torch.Tensor] = None
        # normalised surface Dice at tolerances in mm, off by default: region-wise on the final mask (one bounded search over
        # bit-packed edge masks, no distance transform), and lesion-wise behind the lesion-wise scores, on their scratch
        self.enable_surface_dice, self.surface_dice_tolerances = surface_dice_config(self.config)
        self.enable_lesionwise_nsd, self.lesionwise_nsd_tolerances = lesionwise_nsd_config(self.config)
        for on, key in ((self.enable_surface_dice, "evaluation.surface_dice.enable"),
                        (self.enable_lesionwise_nsd, "evaluation.lesionwise.nsd.enable")):
            if on and bool(get_config(self.config, "training.criterion.softmax", False)):
                raise NotImplementedError(f"{key}: the normalised surface Dice is defined for the sigmoid-region head only "
                                          f"(training.criterion.softmax is set)")
        self._sd: Optional[torch.Tensor] = None
        self._lwnsd: Optional[torch.Tensor] = None
        # input pre-pass on the GPU (raw volumes in, the reference's `_normalize_img` applied here instead of in the
        # dataset worker; reference src/datasets/transforms.py:129-223).  The NIfTI datasets of this package hand over
        # raw intensities, so the pre-pass defaults to on for them and to off for the synthetic source (already
        # normalised); `training.data.transforms.normalize_on_device` overrides either way.
        tcfg = get_config(self.config, "training.data.transforms", {}) or {}
        synthetic = bool(get_config(self.config, "dataset.synthetic.enabled", True))
        nod = get_config(tcfg, "normalize_on_device", None)
        self.normalize_on_device = (not synthetic) if nod is None else bool(nod)
        self._tcfg = tcfg

    @property
    def cal_bins(self) -> int:
        """The bin count as the table helpers take it: 0 = calibration off."""
        return self.calibration_bins if self.enable_calibration else 0

    def prepare_image(self, x: torch.Tensor) -> torch.Tensor:
        if not self.normalize_on_device:
            return x
        from .transforms import normalize_image
        t = self._tcfg
        names = get_config(self.config, "dataset.modality_order", None)
        return torch.stack([normalize_image(x[b].float(), bool(get_config(t, "normalize", True)),
                                            get_config(t, "intensity_policy", None), get_config(t, "mean", None),
                                            get_config(t, "std", None), list(names) if names else None)
                            for b in range(x.size(0))], 0)

    # -- per batch
    def check_batch(self, batch: Dict[str, Any], device) -> Tuple[torch.Tensor, torch.Tensor]:
        x = self.prepare_image(batch["image"].to(device))
        B = x.size(0)
        if "label" not in batch:
            raise KeyError("[BratsSegEval] batch must contain 'label' for region-based eval.")
        y = batch["label"]
        y = y.to(device) if torch.is_tensor(y) else torch.as_tensor(y, device=device)
        if y.ndim == 4:
            y = y.unsqueeze(0).expand(B, -1, -1, -1, -1)
        if y.ndim != 5:
            raise ValueError(f"[BratsSegEval] label must be 5D, got {tuple(y.shape)}")
        R = int(y.size(1))
        if R != len(self.region_order):
            raise ValueError(f"[BratsSegEval] label channels={R} but region_order={len(self.region_order)}")
        return x, y.float()

    def postprocess_launch(self, mask: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Queue the component filter on the current stream, in place on ``mask`` -> device (counts [B,R,3] of the filtered
        mask, stats [B,R,3] = components, kept, removed voxels), both int64."""
        res = ops.components_filter(mask, y, self.postprocess_connectivity, self.postprocess_min_voxels,
                                    self.postprocess_keep_largest, out=mask)
        return res["counts"], res["stats"]

    def fill_nest_launch(self, mask: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Queue hole filling and nesting on the current stream, in place on ``mask`` -> device (counts [B,R,3] of the final
        mask, stats [B,R,4] = holes, filled holes, filled voxels, nested voxels), both int64."""
        res = ops.fill_nest(mask, y, self.postprocess_fill_holes, self.postprocess_fill_connectivity,
                            self.postprocess_max_hole_voxels, self.postprocess_nesting, self.postprocess_nesting_mode)
        return res["counts"], res["stats"]

    @staticmethod
    def fill_nest_columns(stats: torch.Tensor) -> torch.Tensor:
        """stats int64 [R,4] of one volume -> its table columns float64 [4*R], one column's regions after another."""
        return stats.to(torch.float64).t().reshape(-1)

    def lesionwise_launch(self, mask: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Queue the lesion-wise scores of (mask, y) on the current stream -> device stats int64 [B,R,7]."""
        return ops.lesionwise_scores(mask, y, self.lesionwise_dilation, self.lesionwise_connectivity,
                                     self.lesionwise_min_voxels)["stats"]

    def lesionwise_hd95_launch(self, mask: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Queue the lesion-wise scores AND the lesion-wise HD95 of (mask, y) on the current stream -> device (stats int64
        [B,R,7], hd_stats int64 [B,R,3])."""
        res = ops.lesionwise_hd95(mask, y, self.lesionwise_dilation, self.lesionwise_connectivity, self.lesionwise_min_voxels,
                                  self.spacing, self.lesionwise_hd95_percentile)
        return res["stats"], res["hd_stats"]

    def lesionwise_nsd_launch(self, mask: torch.Tensor) -> torch.Tensor:
        """Queue the lesion-wise NSD of ``mask`` on the current stream, behind the lesion-wise scores queued there for it ->
        device nsd_stats int64 [B,R,T]."""
        return ops.lesionwise_nsd_after_scores(mask, self.lesionwise_min_voxels, self.spacing,
                                               self.lesionwise_nsd_tolerances)["nsd_stats"]

    def surface_dice_launch(self, mask: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Queue the NSD counts of (mask, y) on the current stream -> device counts int64 [B,R,T,4]."""
        return ops.surface_dice(mask, y, self.spacing, self.surface_dice_tolerances)

    @property
    def sd_tolerances(self) -> List[float]:
        """The tolerances as the table helpers take them: empty = region-wise NSD off."""
        return self.surface_dice_tolerances if self.enable_surface_dice else []

    @property
    def ln_tolerances(self) -> List[float]:
        return self.lesionwise_nsd_tolerances if self.enable_lesionwise_nsd else []

    def lesionwise_hd95_penalty_mm(self, shape) -> float:
        """The penalty of a missed lesion or a false-positive component for a volume of this shape."""
        if self.lesionwise_hd95_penalty == "diagonal":
            return volume_diagonal_mm(shape, self.spacing)
        return float(self.lesionwise_hd95_penalty)

    @staticmethod
    def component_columns(stats: torch.Tensor) -> torch.Tensor:
        """stats int64 [R,3] of one volume -> its table columns float64 [3*R]: components[R], kept[R], removed voxels[R]."""
        return stats.to(torch.float64).t().reshape(-1)

    def score(self, logits: torch.Tensor, y: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
        """logits [B,R,D,H,W] (or channels-last view) + labels -> exact counts int64 [B,R,3] on the host.
        With ``evaluation.surface.enable`` the prediction mask is kept for :meth:`surface`.  With
        ``evaluation.postprocess.enable`` the mask is filtered in place, the counts are those of the filtered mask and
        ``self._stats`` holds the component figures int64 [B,R,3] (host); with hole filling or nesting on top the counts
        are those of the final mask and ``self._fill`` holds that pass's figures int64 [B,R,4] (host)."""
        R = y.shape[1]
        shape_ok = (logits.ndim == 5 and (logits.shape[-1] if channels_last else logits.shape[1]) == R)
        if not shape_ok:
            raise ValueError(f"[BratsSegEval] model logits must be [B,{R},D,H,W], got {tuple(logits.shape)}")
        counts = torch.empty((y.shape[0], R, 3), dtype=torch.int64, device=y.device)
        need_mask = self.enable_surface or self.enable_postprocess or self.enable_lesionwise or self.enable_surface_dice
        self._mask = torch.empty(tuple(y.shape), dtype=torch.uint8, device=y.device) if need_mask else None
        ops.mask_dice_counts(logits, y, self.threshold, counts, self._mask, logits_channels_last=channels_last)
        self._stats = self._fill = None
        if self.enable_postprocess:
            counts, stats = self.postprocess_launch(self._mask, y)
            if self.enable_fill_nest:
                counts, fill = self.fill_nest_launch(self._mask, y)
                self._fill = fill.cpu()
            self._stats = stats.cpu()
        self._lw = self._lwhd = self._sd = self._lwnsd = None
        lw = lwhd = None
        if self.enable_lesionwise_hd95:
            lw, lwhd = self.lesionwise_hd95_launch(self._mask, y)
        elif self.enable_lesionwise:
            lw = self.lesionwise_launch(self._mask, y)
        # the NSD passes are queued behind the lesion-wise ones, before the first host read
        lwnsd = self.lesionwise_nsd_launch(self._mask) if self.enable_lesionwise_nsd else None
        sd = self.surface_dice_launch(self._mask, y) if self.enable_surface_dice else None
        if lw is not None:
            self._lw = lw.cpu()
        if lwhd is not None:
            self._lwhd = lwhd.cpu()
        if lwnsd is not None:
            self._lwnsd = lwnsd.cpu()
        if sd is not None:
            self._sd = sd.cpu()
        return counts.cpu()

    def calibration_launch(self, logits: torch.Tensor, y: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
        """Queue the reliability histogram of (logits, y) on the current stream -> device table float64 [B, Rout, 3*bins + 2]."""
        out = torch.empty((y.shape[0], len(self.calibration_regions), 3 * self.calibration_bins + 2), dtype=torch.float64,
                          device=y.device)
        ops.calibration_bins(logits, y, self.calibration_bins, out, softmax=self.calibration_softmax,
                             scope=self.calibration_scope, logits_channels_last=channels_last)
        return out

    def surface_launch(self, mask: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Queue HD95 / ASD of (mask, y) on the current stream -> device tensors [B,R] as MONAI would return them."""
        return ops.surface_distances(mask, y, self.spacing, 95.0, self.asd_symmetric)

    def surface_fix(self, hd: torch.Tensor, asd: torch.Tensor, counts: torch.Tensor, shape) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's penalty (GT non-empty, prediction empty -> volume diagonal in mm) and sanitising (non-finite ->
        diagonal) on the valid entries (reference src/evaluation/seg_eval.py:342-355); host tensors out."""
        diag_mm = volume_diagonal_mm(shape, self.spacing)
        hd, asd = hd.cpu(), asd.cpu()
        valid = counts[..., 2] > 0
        pred_empty = counts[..., 1] == 0
        pen = valid & pred_empty
        hd[pen] = diag_mm
        asd[pen] = diag_mm
        hd[(~torch.isfinite(hd)) & valid] = diag_mm
        asd[(~torch.isfinite(asd)) & valid] = diag_mm
        return hd, asd

    def surface(self, y: torch.Tensor, counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """HD95 / ASD [B,R] (host, fp32) of the masks of the last :meth:`score` call (reference seg_eval.py:312-355)."""
        hd, asd = self.surface_launch(self._mask, y)
        return self.surface_fix(hd, asd, counts, y.shape[2:])

    @torch.no_grad()
    def evaluate_epoch(self, model: torch.nn.Module, data_loader: Iterable, device) -> Dict[str, float]:
        """Single process: the reference's loop and aggregation (seg_eval.py:276-460).  Under an initialised
        ``torch.distributed`` group with more than one rank ``data_loader`` is this rank's shard: every volume becomes a
        row of the per-volume table, the tables are merged (``merge_rank_tables``) and every rank reports the metrics of
        the WHOLE split - a rank never prints the metrics of its shard as if they were the test set."""
        import torch.distributed as dist

        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        model.eval()
        model.to(device)
        acc = RegionAccumulator(self.region_order, self.enable_surface, self.cal_bins, self.calibration_regions,
                                self.enable_postprocess, self.enable_lesionwise, self.enable_fill_nest,
                                self.enable_lesionwise_hd95, self.sd_tolerances, self.ln_tolerances)
        rows: List[torch.Tensor] = []
        domain_names: List[str] = []
        n_local = 0
        for batch in data_loader:
            x, y = self.check_batch(batch, device)
            logits = model(x)
            counts = self.score(logits.float(), y)
            dice, iou, valid = dice_iou_from_counts(counts)
            hd, asd = self.surface(y, counts) if self.enable_surface else (None, None)
            cal = self.calibration_launch(logits.float(), y).cpu() if self.enable_calibration else None
            comp = [self.component_columns(st) for st in self._stats] if self.enable_postprocess else None
            lw = [lesionwise_columns(st) for st in self._lw] if self.enable_lesionwise else None
            lh = ([lesionwise_hd95_columns(st, hs, self.lesionwise_hd95_penalty_mm(y.shape[2:]))
                   for st, hs in zip(self._lw, self._lwhd)] if self.enable_lesionwise_hd95 else None)
            fn = [self.fill_nest_columns(st) for st in self._fill] if self.enable_fill_nest else None
            ln = ([lesionwise_nsd_columns(st, ns) for st, ns in zip(self._lw, self._lwnsd)] if self.enable_lesionwise_nsd
                  else None)
            sdc = [surface_dice_columns(c) for c in self._sd] if self.enable_surface_dice else None
            domains = as_list_str(batch.get("domain", None), batch_size=x.size(0))
            if world == 1:
                for i in range(x.size(0)):
                    acc.add_row(dice[i].tolist(), iou[i].tolist(), valid[i].tolist(), domains[i],
                                hd[i].tolist() if hd is not None else None, asd[i].tolist() if asd is not None else None,
                                cal[i] if cal is not None else None, comp[i] if comp is not None else None,
                                lw[i] if lw is not None else None, fn[i] if fn is not None else None,
                                lh[i] if lh is not None else None, sdc[i] if sdc is not None else None,
                                ln[i] if ln is not None else None)
                if self.report_loss:
                    acc.add_loss(self.loss_fn(logits.float(), y), x.size(0))
                continue
            losses = (self.loss_fn.values_per_volume(self.loss_fn.launch(logits.float(), y)) if self.report_loss
                      else [0.0] * x.size(0))
            idx = batch.get("index", None)
            if idx is None:
                raise KeyError("[seg_eval] a sharded evaluation needs batch['index'] (the volume's position in the whole split): "
                               "rank-local counters collide across ranks")
            for i in range(x.size(0)):
                if domains[i] not in domain_names:
                    domain_names.append(domains[i])
                parts = [torch.tensor([int(idx[i]), domain_names.index(domains[i]),
                                       losses[i]], dtype=torch.float64),
                         dice[i].double(), iou[i].double(), valid[i].double()]
                if self.enable_surface:
                    parts += [hd[i].double(), asd[i].double()]
                if comp is not None:
                    parts.append(comp[i])
                if fn is not None:
                    parts.append(fn[i])
                if lw is not None:
                    parts.append(lw[i])
                if lh is not None:
                    parts.append(lh[i])
                if ln is not None:
                    parts.append(ln[i])
                if sdc is not None:
                    parts.append(sdc[i])
                if cal is not None:
                    parts.append(cal[i].reshape(-1))
                rows.append(torch.cat(parts))
                n_local += 1
        if world == 1:
            if self.enable_calibration:
                self.last_reliability = acc.reliability
            return acc.metrics(self.report_loss)
        table = torch.stack(rows) if rows else torch.empty((0, self._table_width()), dtype=torch.float64)
        table, domain_names = merge_rank_tables(table, domain_names, device)
        self.last_table = table
        return self._metrics_of(table, domain_names)

    def _table_width(self) -> int:
        return table_width(len(self.region_order), self.enable_surface, self.cal_bins, len(self.calibration_regions),
                           components=self.enable_postprocess, lesionwise=self.enable_lesionwise,
                           fill_nest=self.enable_fill_nest, lesionwise_hd95=self.enable_lesionwise_hd95,
                           surface_dice=len(self.sd_tolerances), lesionwise_nsd=len(self.ln_tolerances))

    def _metrics_of(self, table: torch.Tensor, domain_names: Sequence[str]) -> Dict[str, float]:
        """Metrics of the whole split from its per-volume table (and ``last_reliability`` with calibration on)."""
        if self.enable_calibration:
            self.last_reliability = reliability_from_table(table, self.calibration_bins, len(self.calibration_regions))
        return metrics_from_table(table, self.region_order, domain_names, self.report_loss, self.enable_surface,
                                  self.cal_bins, self.calibration_regions, components=self.enable_postprocess,
                                  lesionwise=self.enable_lesionwise, fill_nest=self.enable_fill_nest,
                                  lesionwise_hd95=self.enable_lesionwise_hd95, surface_dice=self.sd_tolerances,
                                  lesionwise_nsd=self.ln_tolerances)


# ----------------------------------------------------------------------------- sharding
def shard_indices(n_items: int, rank: int, world: int) -> List[int]:
    """Round-robin, deterministic: volume i -> rank i mod W."""
    return list(range(rank, n_items, world))


def table_width(R: int, surface: bool = False, bins: int = 0, rout: Optional[int] = None, components: bool = False,
                lesionwise: bool = False, fill_nest: bool = False, lesionwise_hd95: bool = False, surface_dice: int = 0,
                lesionwise_nsd: int = 0) -> int:
    """index, domain_id, loss, then dice[R], iou[R], valid[R] (, hd95[R], asd[R]) (, with ``components`` the figures of the
    post-processing: components[R], kept[R], removed voxels[R]) (, with ``fill_nest`` the figures of the hole filling and
    nesting: holes[R], filled holes[R], filled voxels[R], nested voxels[R]) (, with ``lesionwise`` the 7*R columns of
    ``lesionwise_columns``) (, with ``lesionwise_hd95`` the 2*R columns of ``lesionwise_hd95_columns``) (, with ``lesionwise_nsd`` = T > 0 tolerances the T*R columns of ``lesionwise_nsd_columns``)
    (, with ``surface_dice`` = T > 0 tolerances the T*R columns of ``surface_dice_columns``) (, with ``bins`` > 0 the volume's raw calibration table: ``rout`` rows - default R - of
    3*bins + 2 doubles, always last)."""
    return (3 + (5 if surface else 3) * R + (3 * R if components else 0) + (FILL_NEST_COLUMNS * R if fill_nest else 0) +
            (LESIONWISE_COLUMNS * R if lesionwise else 0) + (LESIONWISE_HD95_COLUMNS * R if lesionwise_hd95 else 0) +
            (int(lesionwise_nsd) + int(surface_dice)) * R + calibration_width(bins, R if rout is None else rout))


def reliability_from_table(table: torch.Tensor, bins: int, rout: int) -> torch.Tensor:
    """The pooled reliability diagram of the gathered rows: float64 [rout, bins, 3] = (count, sum of confidence, correct
    count), summed over the volumes in row order."""
    out = torch.zeros((rout, bins, 3), dtype=torch.float64)
    w = calibration_width(bins, rout)
    for row in table:
        out += row[row.numel() - w:].to(torch.float64).reshape(rout, 3 * bins + 2)[:, :3 * bins].reshape(rout, bins, 3)
    return out


def gather_table(rows: torch.Tensor, n_items: int, world: int, group=None) -> torch.Tensor:
    """all_gather the fixed-shape per-volume table [ceil(N/W), width] (float64; unused rows have index -1)
    and return the rows sorted by volume index.  The only collective of the path."""
    import torch.distributed as dist

    per = (n_items + world - 1) // world
    pad = torch.full((per, rows.shape[1]), -1.0, dtype=torch.float64, device=rows.device)
    pad[:rows.shape[0]] = rows
    if not (dist.is_available() and dist.is_initialized()):
        allrows = pad
    else:
        bufs = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(bufs, pad, group=group)
        allrows = torch.cat(bufs, dim=0)
    allrows = allrows.cpu()
    allrows = allrows[allrows[:, 0] >= 0]
    order = torch.argsort(allrows[:, 0], stable=True)
    allrows = allrows[order]
    if allrows.shape[0] > 1:          # a sampler that pads the last shard repeats volumes: keep the first row per index
        keep = torch.ones(allrows.shape[0], dtype=torch.bool)
        keep[1:] = allrows[1:, 0] != allrows[:-1, 0]
        allrows = allrows[keep]
    return allrows


def gather_masks(local: Sequence[Tuple[int, torch.Tensor]], device, group=None) -> Dict[int, torch.Tensor]:
    """The optional second collective of a sharded evaluation (north star: "all-gather final
    Dice/logits"): every rank's thresholded masks uint8 [R,D,H,W], keyed by volume index, gathered to every rank.
    One ``all_reduce(MAX)`` agrees on the pad shape (ranks may hold unequal shares and ragged extents), one ``all_gather``
    moves the index / extent rows, one the padded masks (6 MB per 128^3 BraTS volume).  Single process: the local dict."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return {int(i): m for i, m in local}
    world = dist.get_world_size()
    dev = device if dist.get_backend() == "nccl" else "cpu"
    ext = torch.zeros(5, dtype=torch.int64)                   # rows, R, D, H, W: the maxima over ranks
    ext[0] = len(local)
    for _, m in local:
        ext[1:] = torch.maximum(ext[1:], torch.tensor(list(m.shape), dtype=torch.int64))
    ext = ext.to(dev)
    dist.all_reduce(ext, op=dist.ReduceOp.MAX, group=group)
    per, R, D, H, W = (int(v) for v in ext.tolist())
    meta = torch.full((max(per, 1), 5), -1, dtype=torch.int64)
    buf = torch.zeros((max(per, 1), R, D, H, W), dtype=torch.uint8)
    for k, (i, m) in enumerate(local):
        meta[k] = torch.tensor([int(i), *m.shape], dtype=torch.int64)
        buf[k, :m.shape[0], :m.shape[1], :m.shape[2], :m.shape[3]] = m
    meta, buf = meta.to(dev), buf.to(dev)
    metas = [torch.empty_like(meta) for _ in range(world)]
    bufs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(metas, meta, group=group)
    dist.all_gather(bufs, buf, group=group)
    out: Dict[int, torch.Tensor] = {}
    for mt, bf in zip(metas, bufs):
        mt, bf = mt.cpu(), bf.cpu()
        for k in range(mt.shape[0]):
            i, r, d, h, w = (int(v) for v in mt[k].tolist())
            if i >= 0 and i not in out:
                out[i] = bf[k, :r, :d, :h, :w].clone()
    return out


def metrics_from_table(table: torch.Tensor, region_order: Sequence[str], domain_names: Sequence[str],
                       report_loss: bool, surface: bool = False, bins: int = 0,
                       calibration_regions: Optional[Sequence[str]] = None, components: bool = False,
                       lesionwise: bool = False, fill_nest: bool = False, lesionwise_hd95: bool = False,
                       surface_dice: Sequence[float] = (), lesionwise_nsd: Sequence[float] = ()) -> Dict[str, float]:
    """Replay the reference aggregation over gathered rows in volume-index order: the result is
    identical to a single-process run (float64 sums, order fixed by index).  ``bins`` > 0: the rows end in the raw
    calibration table of their volume (``table_width``), one row of it per name in ``calibration_regions``.
    ``components``: the 3*R component columns sit behind the surface columns (``table_width``); ``fill_nest``: the 4*R
    columns of the hole filling and nesting sit behind those; ``lesionwise``: the 7*R lesion-wise columns sit behind those;
    ``lesionwise_hd95``: the 2*R lesion-wise HD95 columns sit directly behind those; ``lesionwise_nsd`` and ``surface_dice``
    (their tolerances): the T*R lesion-wise NSD columns, then the T*R region-wise NSD columns, behind those."""
    R = len(region_order)
    acc = RegionAccumulator(region_order, surface, bins, calibration_regions, components, lesionwise, fill_nest, lesionwise_hd95,
                            surface_dice, lesionwise_nsd)
    c0 = 3 + (5 if surface else 3) * R
    f0 = c0 + (3 * R if components else 0)
    l0 = f0 + (FILL_NEST_COLUMNS * R if fill_nest else 0)
    h0 = l0 + (LESIONWISE_COLUMNS * R if lesionwise else 0)
    n0 = h0 + (LESIONWISE_HD95_COLUMNS * R if lesionwise_hd95 else 0)
    s0 = n0 + len(acc.lesionwise_nsd) * R
    cal_w = calibration_width(bins, len(acc.cal_regions))
    for row in table:
        dom = domain_names[int(row[1].item())] if 0 <= int(row[1].item()) < len(domain_names) else ""
        dice = row[3:3 + R].to(torch.float32).tolist()
        iou = row[3 + R:3 + 2 * R].to(torch.float32).tolist()
        valid = (row[3 + 2 * R:3 + 3 * R] > 0.5).tolist()
        hd = row[3 + 3 * R:3 + 4 * R].to(torch.float32).tolist() if surface else None
        asd = row[3 + 4 * R:3 + 5 * R].to(torch.float32).tolist() if surface else None
        acc.add_row(dice, iou, valid, dom, hd, asd, row[row.numel() - cal_w:] if bins else None,
                    row[c0:c0 + 3 * R] if components else None,
                    row[l0:l0 + LESIONWISE_COLUMNS * R] if lesionwise else None,
                    row[f0:f0 + FILL_NEST_COLUMNS * R] if fill_nest else None,
                    row[h0:h0 + LESIONWISE_HD95_COLUMNS * R] if lesionwise_hd95 else None,
                    row[s0:s0 + len(acc.surface_dice) * R] if acc.surface_dice else None,
                    row[n0:s0] if acc.lesionwise_nsd else None)
        if report_loss:
            acc.add_loss(float(row[2].item()), 1)
    return acc.metrics(report_loss)


def merge_rank_tables(table: torch.Tensor, domain_names: List[str], device) -> Tuple[torch.Tensor, List[str]]:
    """Merge the ranks' per-volume tables into the table of the whole split, identical on every rank.

    THREE collectives, all outside the data path and all tiny: ``all_gather_object`` of the domain-name lists (domain
    ids must mean the same on every rank), ``all_reduce`` of the row counts (ranks may hold unequal shares), then the
    ``all_gather`` of the fixed-shape table (``gather_table``) - RCCL over xGMI with the ``nccl`` backend, gloo in the
    CPU tests.  Rows come back sorted by volume index, so the aggregation that follows is order-identical to a
    single-process run."""
    import torch.distributed as dist

    world = dist.get_world_size()
    names: List[Optional[List[str]]] = [None] * world
    dist.all_gather_object(names, list(domain_names))
    merged = sorted({n for lst in names for n in (lst or [])})
    remap = {i: merged.index(n) for i, n in enumerate(domain_names)}
    table = table.clone()
    for r in range(table.shape[0]):
        table[r, 1] = remap[int(table[r, 1].item())]
    dev = device if dist.get_backend() == "nccl" else "cpu"
    counts_t = torch.tensor([table.shape[0]], dtype=torch.int64, device=dev)
    per_max = counts_t.clone()
    dist.all_reduce(counts_t)
    dist.all_reduce(per_max, op=dist.ReduceOp.MAX)
    # gather_table pads every rank to ceil(N/W) rows; with an arbitrary (not round-robin) shard the largest share can
    # exceed that, so size the pad by the largest share
    n_items = max(int(counts_t.item()), int(per_max.item()) * world, 1)
    table = gather_table(table.to(dev), n_items, world)
    return table, merged


@register_evaluation_strategy("seg_tta_eval")
class TTASegmentationEvaluationStrategy(SegmentationEvaluationStrategy):
    """Adapt each volume (plugin ``method.name``, default ``entmin_tta``), then score it."""

    def __init__(self, config: Any = None):
        super().__init__(config)
        self.plugin_name = str(get_config(self.config, "method.name", "entmin_tta"))
        # volumes adapted concurrently on this GPU, each with its own weights, buffers, graph and stream: episodic
        # adaptation has no cross-volume state, and one volume alone leaves most CUs waiting at the lower U-Net levels
        # (measured, unet 4x128^3, S = 10: 29.6 / 39.7 / 35.7 volumes/s for 1 / 2 / 3 lanes)
        self.lanes = max(1, int(get_config(self.config, "method.lanes", 1)))
        # volumes that adapt TOGETHER as the batch items of one launch sequence, each on its own replica of the weights
        # (the plugin's `method.group`); lanes x group volumes are in flight per GPU
        self.group = max(1, int(get_config(self.config, "method.group", 1)))
        # north star: "RCCL ... used only to all-gather final Dice/logits": with `evaluation.gather_masks` the thresholded
        # uint8 masks [R,D,H,W] of every volume are gathered to every rank as well (a second all_gather, off by default)
        self.gather_masks = bool(get_config(self.config, "evaluation.gather_masks", False))
        self.local_masks: List[Tuple[int, torch.Tensor]] = []
        self.last_masks: Dict[int, torch.Tensor] = {}
        self.plugin = None
        self.plugins: List[Any] = []
        self.streams: List[Any] = []

    def _setup_lanes(self, model: torch.nn.Module, device) -> None:
        from .registry import get_model
        self.plugin = get_plugin(self.plugin_name)(self.config).setup(model, device)
        self.group = int(getattr(self.plugin, "group", 1))       # what the plugin settled on (1 for models whose norms carry parameters)
        self.plugins, self.streams = [self.plugin], [None]
        if self.lanes > 1:
            pool = ops.lane_streams(self.lanes, device)          # one hardware queue per lane
            self.streams = [pool[0]]
            mcfg = get_config(self.config, "model", None)
            for lane in range(1, self.lanes):
                twin = get_model(str(get_config(mcfg, "name", "unet")))(mcfg)
                twin.load_state_dict(model.state_dict())
                p = get_plugin(self.plugin_name)(self.config)
                p.lane = lane
                self.plugins.append(p.setup(twin, device))
                self.streams.append(pool[lane])

    def _provide_fisher(self, data_loader: Iterable, device) -> Iterable:
        """A Fisher estimate for a plugin that asks for one (``needs_fisher``), before the first volume adapts: the file
        ``method.eata.fisher.path`` names, else an estimate on lane 0's plugin from the first ``fisher.volumes`` volumes of the
        loader (this rank's shard).  One span serves every lane.  Returns the loader to evaluate: the batches drawn for the
        estimate come first again, so every volume is still evaluated once and in order."""
        import itertools

        plugin = self.plugin
        buffered: List[Any] = []
        it = iter(data_loader)
        if getattr(plugin, "fisher_path", None):
            plugin.load_fisher(plugin.fisher_path)
        else:
            want, vols = int(plugin.fisher_volumes), []
            while len(vols) < want:
                batch = next(it, None)
                if batch is None:
                    break
                buffered.append(batch)
                x = self.prepare_image(batch["image"].to(device))
                vols += [x[i:i + 1] for i in range(x.size(0))]
            vols = vols[:want]
            if vols:
                plugin.estimate_fisher(torch.cat(vols[i:i + self.group]) for i in range(0, len(vols), self.group))
        if plugin.fisher is not None:
            for other in self.plugins[1:]:
                other.set_fisher(plugin.fisher, plugin.fisher_count)
        return itertools.chain(buffered, it)

    def _submit(self, lane: int, xb: torch.Tensor, yb: torch.Tensor) -> Dict[str, Any]:
        """Queue adaptation + scoring of one volume - or of one GROUP of volumes (``method.group``, batch items that adapt
        independently) - on the lane's stream; nothing here waits for the GPU."""
        B, R = yb.shape[0], yb.shape[1]
        res = self.plugins[lane].adapt_volume(xb)
        counts = torch.empty((B, R, 3), dtype=torch.int64, device=yb.device)
        need_mask = (self.enable_surface or self.gather_masks or self.enable_postprocess or self.enable_lesionwise or
                     self.enable_surface_dice)
        mask = torch.empty(tuple(yb.shape), dtype=torch.uint8, device=yb.device) if need_mask else None
        ops.mask_dice_counts(res["logits_cl"], yb, self.threshold, counts, mask, logits_channels_last=True)
        stats = None
        if self.enable_postprocess:      # in place: the surface pass and the gathered masks below take the filtered mask
            counts, stats = self.postprocess_launch(mask, yb)
        fill = None
        if self.enable_fill_nest:        # likewise in place, right behind the filter: its counts replace the filter's
            counts, fill = self.fill_nest_launch(mask, yb)
        job: Dict[str, Any] = {"counts": counts, "shape": tuple(yb.shape[2:]), "keep": (xb, yb, mask, res), "mask": mask}
        if stats is not None:
            job["components"] = stats
        if fill is not None:
            job["fill_nest"] = fill
        if self.enable_lesionwise_hd95:  # right behind the counts, on the mask they describe; the HD95 pass on the same scratch
            job["lesionwise"], job["lesionwise_hd95"] = self.lesionwise_hd95_launch(mask, yb)
        elif self.enable_lesionwise:
            job["lesionwise"] = self.lesionwise_launch(mask, yb)
        if self.enable_lesionwise_nsd:   # behind the lesion-wise passes, on their scratch
            job["lesionwise_nsd"] = self.lesionwise_nsd_launch(mask)
        if self.enable_surface_dice:     # on the final mask, like the surface distances
            job["surface_dice"] = self.surface_dice_launch(mask, yb)
        if self.report_loss:
            job["loss"] = self.loss_fn.launch(res["logits_cl"], yb, channels_last=True)
        if self.enable_surface:
            job["surface"] = self.surface_launch(mask, yb)
        if self.enable_calibration:
            job["calibration"] = self.calibration_launch(res["logits_cl"], yb, channels_last=True)
        return job

    def _finish(self, job: Dict[str, Any]) -> List[torch.Tensor]:
        """First host read of a queued group -> the table rows of its volumes."""
        counts = job["counts"].cpu()
        dice, iou, valid = dice_iou_from_counts(counts)
        B = counts.shape[0]
        losses = self.loss_fn.values_per_volume(job["loss"]) if self.report_loss else [0.0] * B
        if self.enable_surface:
            hd, asd = self.surface_fix(job["surface"][0], job["surface"][1], counts, job["shape"])
        cal = job["calibration"].cpu() if self.enable_calibration else None
        comp = job["components"].cpu() if self.enable_postprocess else None
        lw = job["lesionwise"].cpu() if self.enable_lesionwise else None
        lh = job["lesionwise_hd95"].cpu() if self.enable_lesionwise_hd95 else None
        pen = self.lesionwise_hd95_penalty_mm(job["shape"]) if self.enable_lesionwise_hd95 else 0.0
        fn = job["fill_nest"].cpu() if self.enable_fill_nest else None
        ln = job["lesionwise_nsd"].cpu() if self.enable_lesionwise_nsd else None
        sdc = job["surface_dice"].cpu() if self.enable_surface_dice else None
        rows = []
        for b in range(B):
            parts = [torch.tensor([job["index"][b], job["domain_id"][b], losses[b]], dtype=torch.float64),
                     dice[b].double(), iou[b].double(), valid[b].double()]
            if self.enable_surface:
                parts += [hd[b].double(), asd[b].double()]
            if comp is not None:
                parts.append(self.component_columns(comp[b]))
            if fn is not None:
                parts.append(self.fill_nest_columns(fn[b]))
            if lw is not None:
                parts.append(lesionwise_columns(lw[b]))
            if lh is not None:
                parts.append(lesionwise_hd95_columns(lw[b], lh[b], pen))
            if ln is not None:
                parts.append(lesionwise_nsd_columns(lw[b], ln[b]))
            if sdc is not None:
                parts.append(surface_dice_columns(sdc[b]))
            if cal is not None:
                parts.append(cal[b].reshape(-1))
            rows.append(torch.cat(parts))
        if self.gather_masks:
            mk = job["mask"].cpu()
            for b in range(B):
                self.local_masks.append((int(job["index"][b]), mk[b]))
        return rows

    @torch.no_grad()
    def evaluate_epoch(self, model: torch.nn.Module, data_loader: Iterable, device) -> Dict[str, float]:
        """``data_loader`` yields this rank's shard (any batch size).  ``method.group`` volumes adapt together in one launch
        sequence (each on its own replica of the weights), ``method.lanes`` such groups are in flight on their own streams;
        results are read back when a lane is needed again."""
        import torch.distributed as dist

        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if self.plugin is None:
            self._setup_lanes(model, device)
        if getattr(self.plugin, "needs_fisher", False):      # (eata_tta with its regulariser on and no estimate yet)
            data_loader = self._provide_fisher(data_loader, device)
        done: List[Tuple[int, torch.Tensor]] = []          # (submission order, row)
        pending: List[Optional[Dict[str, Any]]] = [None] * self.lanes
        domain_names: List[str] = []
        self.local_masks = []
        n_local = 0
        n_groups = 0
        group: List[Tuple[torch.Tensor, torch.Tensor, int, int, int]] = []      # (x1, y1, order, index, domain id)
        keep_alive: List[torch.Tensor] = []

        def flush(lane: int) -> None:
            job = pending[lane]
            if job is not None:
                if self.streams[lane] is not None:
                    self.streams[lane].synchronize()         # host reads below are issued from the main stream
                for order, row in zip(job["order"], self._finish(job)):
                    done.append((order, row))
                pending[lane] = None

        def dispatch() -> None:
            nonlocal n_groups
            lane = n_groups % self.lanes
            flush(lane)                                      # the lane's buffers are about to be reused
            xb = torch.cat([g[0] for g in group]) if len(group) > 1 else group[0][0]
            yb = torch.cat([g[1] for g in group]) if len(group) > 1 else group[0][1]
            stream = self.streams[lane]
            if stream is None:
                job = self._submit(lane, xb, yb)
            else:
                stream.wait_stream(torch.cuda.current_stream(device))      # inputs were prepared on the main stream
                with torch.cuda.stream(stream):
                    job = self._submit(lane, xb, yb)
                for t in (xb, yb, *keep_alive):
                    t.record_stream(stream)
            job.update(order=[g[2] for g in group], index=[g[3] for g in group], domain_id=[g[4] for g in group])
            pending[lane] = job
            n_groups += 1
            group.clear()
            keep_alive.clear()

        for batch in data_loader:
            x, y = self.check_batch(batch, device)
            domains = as_list_str(batch.get("domain", None), batch_size=x.size(0))
            idx = batch.get("index", None)
            if idx is None and world > 1:
                raise KeyError("[seg_tta_eval] a sharded evaluation needs batch['index'] (the volume's position in the whole "
                               "split): rank-local counters collide across ranks")
            keep_alive += [x, y]
            for i in range(x.size(0)):
                if domains[i] not in domain_names:
                    domain_names.append(domains[i])
                group.append((x[i:i + 1], y[i:i + 1], n_local, int(idx[i]) if idx is not None else n_local,
                              domain_names.index(domains[i])))
                n_local += 1
                if len(group) == self.group:
                    dispatch()
        if group:
            dispatch()
        for lane in range(self.lanes):
            flush(lane)
        rows = [row for _, row in sorted(done, key=lambda t: t[0])]
        table = torch.stack(rows) if rows else torch.empty((0, self._table_width()), dtype=torch.float64)
        if world > 1:
            table, domain_names = merge_rank_tables(table, domain_names, device)
        self.last_table = table
        if self.gather_masks:
            self.last_masks = gather_masks(self.local_masks, device)
        return self._metrics_of(table, domain_names)
