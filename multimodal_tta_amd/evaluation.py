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
from typing import Any, Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import ops
from .config import as_cfg, get_config
from .guard import guard_enabled
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


def _enable(block: Any, key: str) -> bool:
    """``block.enable`` of the config block at ``key``: a bool, false when absent."""
    enable = get_config(block, "enable", False)
    if not isinstance(enable, bool):
        raise ValueError(f"{key}.enable must be true or false, got {enable!r}")
    return enable


def _is_count(x: Any) -> bool:
    return isinstance(x, int) and not isinstance(x, bool) and x >= 0


def _per_region(block: Any, key: str, name: str, default: Any, R: int, ok: Callable[[Any], bool], what: str) -> list:
    """``block[name]`` of the config block at ``key`` as one value per region: a scalar stands for every region, a list has
    one entry per region of ``evaluation.seg.region_order``."""
    v = get_config(block, name, default)
    scalar = isinstance(v, (bool, int))
    vals = [v] * R if scalar else (list(v) if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else None)
    if vals is None or not all(ok(x) for x in vals):
        raise ValueError(f"{key}.{name} must be {what} or a list of one per region, got {v!r}")
    if len(vals) != R:
        raise ValueError(f"{key}.{name} has {len(vals)} entries for the {R} regions of evaluation.seg.region_order")
    return vals


CALIBRATION_SCOPES = ("volume", "union")
CALIBRATION_MAX_BINS = 64


def calibration_config(config: Any) -> Tuple[bool, int, str]:
    """``evaluation.calibration: {enable, bins, scope}`` -> (enable, bins, scope); off, 15 bins, ``volume`` when absent.
    A value the kernel cannot take is a ``ValueError`` that names its key, whether the block is enabled or not."""
    cal = get_config(config, "evaluation.calibration", {}) or {}
    enable = _enable(cal, "evaluation.calibration")
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
    enable = _enable(pp, "evaluation.postprocess")
    conn = get_config(pp, "connectivity", 26)
    if isinstance(conn, bool) or conn not in POSTPROCESS_CONNECTIVITIES:
        raise ValueError(f"evaluation.postprocess.connectivity must be one of {list(POSTPROCESS_CONNECTIVITIES)}, got {conn!r}")
    mv = _per_region(pp, "evaluation.postprocess", "min_voxels", 0, R, _is_count, "a non-negative integer")
    kl = _per_region(pp, "evaluation.postprocess", "keep_largest", False, R, lambda x: isinstance(x, bool), "true or false")
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
    fh = _per_region(pp, "evaluation.postprocess", "fill_holes", dflt["fill_holes"], R, lambda x: isinstance(x, bool),
                     "true or false")
    conn = get_config(pp, "fill_connectivity", dflt["fill_connectivity"])
    if isinstance(conn, bool) or conn not in POSTPROCESS_CONNECTIVITIES:
        raise ValueError(f"evaluation.postprocess.fill_connectivity must be one of {list(POSTPROCESS_CONNECTIVITIES)}, got {conn!r}")
    cap = _per_region(pp, "evaluation.postprocess", "max_hole_voxels", dflt["max_hole_voxels"], R, _is_count,
                      "a non-negative integer")
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
    enable = _enable(lw, "evaluation.lesionwise")
    dil = get_config(lw, "dilation", 3)
    if isinstance(dil, bool) or not isinstance(dil, int) or not 0 <= dil <= LESIONWISE_MAX_DILATION:
        raise ValueError(f"evaluation.lesionwise.dilation must be an integer in 0 ... {LESIONWISE_MAX_DILATION}, got {dil!r}")
    conn = get_config(lw, "dilation_connectivity", 18)
    if isinstance(conn, bool) or conn not in LESIONWISE_CONNECTIVITIES:
        raise ValueError(f"evaluation.lesionwise.dilation_connectivity must be one of {list(LESIONWISE_CONNECTIVITIES)}, "
                         f"got {conn!r}")
    vals = _per_region(lw, "evaluation.lesionwise", "min_lesion_voxels", 0, R, _is_count, "a non-negative integer")
    return enable, int(dil), int(conn), [int(x) for x in vals]


def stat_columns(stats: torch.Tensor) -> torch.Tensor:
    """stats int64 [R,C] of one volume, as the component filter (components, kept, removed voxels) and the fill / nest pass
    (holes, filled holes, filled voxels, nested voxels) leave them -> its table columns float64 [C*R], one column's regions
    after another."""
    return stats.to(torch.float64).t().reshape(-1)


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
    enable = _enable(hd, "evaluation.lesionwise.hd95")
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
    enable = _enable(block, key)
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


# ----------------------------------------------------------------------------- the per-volume table and its blocks
class Block(NamedTuple):
    """One optional group of columns of the per-volume table, and what becomes of it.  ``p`` is the block's parameter
    (``table_layout``): ``True``, the tolerances of an NSD block, (bins, rows) of the calibration."""
    name: str
    width: Callable[[int, Any], int]                  # (R, p) -> doubles per row
    shape: Callable[[int, Any], Tuple[int, ...]]      # (R, p) -> shape of the float64 accumulator
    columns: Callable[[Dict[str, Any]], torch.Tensor]         # what the passes left of one volume, by pass -> its columns
    add: Callable[[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]], None]     # accumulator += columns; the whole row by block
    keys: Callable[[Dict[str, float], str, torch.Tensor, Sequence[str], Any], None]        # out, prefix, accumulator, regions, p


def _n(p: Any) -> int:
    """A count, or the length of a list."""
    return p if isinstance(p, int) else len(p)


def _fin(s: torch.Tensor, c: torch.Tensor) -> List[float]:
    return [float((s[k] / c[k]).item()) if c[k] > 0 else 0.0 for k in range(len(s))]


def _avg(means: List[float], cnt: torch.Tensor) -> float:
    ok = [k for k in range(len(means)) if cnt[k] > 0]
    return float(sum(means[k] for k in ok) / max(1, len(ok)))


def _mean_keys(out: Dict[str, float], prefix: str, names: Sequence[str], key: str, s: torch.Tensor, c: torch.Tensor,
               avg: bool = True) -> None:
    """``{name}_{key}`` = s / c (0 where c is 0) and, with ``avg``, ``avg_{key}``: their mean over the names with c > 0."""
    means = _fin(s, c)
    for name, v in zip(names, means):
        out[f"{prefix}{name.lower()}_{key}"] = v
    if avg:
        out[f"{prefix}avg_{key}"] = _avg(means, c)


def _add_surface(acc: torch.Tensor, c: torch.Tensor, vol: Dict[str, torch.Tensor]) -> None:
    """sum_hd95, sum_asd, count: over the volumes where Dice is valid (an invalid entry may hold anything)."""
    acc[:2] += torch.where(vol["valid"] > 0, c.reshape(2, -1), 0.0)
    acc[2] += vol["valid"]


def _surface_keys(out, prefix, acc, regions, p) -> None:      # reference seg_eval.py:424-440, :459-476
    _mean_keys(out, prefix, regions, "hd95", acc[0], acc[2])
    _mean_keys(out, prefix, regions, "asd", acc[1], acc[2])


def _add_sums(acc: torch.Tensor, c: torch.Tensor, vol: Dict[str, torch.Tensor]) -> None:
    """The columns summed, then the volumes: per-volume means over ALL volumes."""
    acc[:-1] += c.reshape(acc.shape[0] - 1, -1)
    acc[-1] += 1.0


def _component_keys(out, prefix, acc, regions, p) -> None:
    for row, key in enumerate(("components", "kept_components", "removed_voxels")):
        _mean_keys(out, prefix, regions, key, acc[row], acc[-1], avg=row == 0)


def _fill_nest_keys(out, prefix, acc, regions, p) -> None:
    for row, key in enumerate(ops.FILL_NEST_COLUMNS):
        _mean_keys(out, prefix, regions, key, acc[row], acc[-1], avg=False)


def _add_lesionwise(acc: torch.Tensor, c: torch.Tensor, vol: Dict[str, torch.Tensor]) -> None:
    """The 7 columns summed (lw_dc where valid, valid, kept, found, false-positive, matched, predicted), then the volumes."""
    c = c.reshape(LESIONWISE_COLUMNS, -1)
    acc[0] += c[0] * c[1]
    acc[1:LESIONWISE_COLUMNS] += c[1:]
    acc[LESIONWISE_COLUMNS] += 1.0


def _lesionwise_keys(out, prefix, acc, regions, p) -> None:
    """The lesion-wise Dice averaged over the volumes where it is defined (a GT-empty region with false-positive components
    IS one of them, with 0), per-volume means of kept lesions, found lesions and false-positive components, and recall /
    precision pooled over all volumes."""
    _mean_keys(out, prefix, regions, "lw_dc", acc[0], acc[1])
    for row, key in ((2, "lesions"), (3, "lesions_found"), (4, "fp_components")):
        _mean_keys(out, prefix, regions, key, acc[row], acc[LESIONWISE_COLUMNS], avg=False)
    for k, name in enumerate(regions):       # pooled over the volumes; absent where there is nothing to divide by
        if acc[2][k] > 0:
            out[f"{prefix}{name.lower()}_lesion_recall"] = float((acc[3][k] / acc[2][k]).item())
        if acc[6][k] > 0:
            out[f"{prefix}{name.lower()}_lesion_precision"] = float((acc[5][k] / acc[6][k]).item())


def _add_lesionwise_hd95(acc: torch.Tensor, c: torch.Tensor, vol: Dict[str, torch.Tensor]) -> None:
    """sum_lw_hd95, valid volumes, overflowed volumes, volumes."""
    c = c.reshape(LESIONWISE_HD95_COLUMNS, -1)
    ok, over = (c[1] > 0.5).to(torch.float64), (c[1] < -0.5).to(torch.float64)
    acc[0] += c[0] * ok
    acc[1] += ok
    acc[2] += over
    acc[3] += 1.0


def _lesionwise_hd95_keys(out, prefix, acc, regions, p) -> None:
    """The lesion-wise HD95 averaged over the volumes where it is defined and did not overflow, and the per-volume mean of
    overflowed volumes."""
    _mean_keys(out, prefix, regions, "lw_hd95", acc[0], acc[1])
    _mean_keys(out, prefix, regions, "lw_hd95_overflow", acc[2], acc[3], avg=False)


def _add_nsd(acc: torch.Tensor, c: torch.Tensor, ok: torch.Tensor) -> None:
    """Sums and counts [2, T, R] over the volumes where ``ok`` [R] is 1."""
    acc[0] += c.reshape(acc.shape[1:]) * ok
    acc[1] += ok


def _nsd_keys(stem: str) -> Callable:
    def keys(out, prefix, acc, regions, tolerances) -> None:
        for t, tau in enumerate(tolerances):
            _mean_keys(out, prefix, regions, f"{stem}_{nsd_suffix(tau)}", acc[0][t], acc[1][t])
    return keys


def _add_calibration(acc: torch.Tensor, c: torch.Tensor, vol: Dict[str, torch.Tensor]) -> None:
    """Per row of the head: sum_ece, sum_brier, sum_nll, count, then its 3*bins reliability entries pooled."""
    raw = c.reshape(acc.shape[0], -1)
    ece, brier, nll, valid = calibration_from_bins(raw)
    ok = valid.to(torch.float64)
    acc[:, 0] += ece * ok
    acc[:, 1] += brier * ok
    acc[:, 2] += nll * ok
    acc[:, 3] += ok
    acc[:, 4:] += raw[:, :-2]


GUARD_COLUMNS = 5          # per region: fallback flag, flips s + a - 2i, agreement numerator 2i and denominator s + a, source Dice
GUARD_RAW = 7              # what a volume's passes leave per region: fallback, s, a, i, then (inter, pred, gt) of the reference


def guard_columns(raw: torch.Tensor) -> torch.Tensor:
    """raw int64 [R,7] = (fallback, s, a, i, inter, pred, gt of the reference's scored mask) -> float64 [5 R]: one column's
    regions after another.  The source Dice is formed as ``dice_iou_from_counts`` forms Dice (fp32), so sharded, grouped and
    single runs agree bit for bit."""
    raw = raw.to(torch.int64).reshape(-1, GUARD_RAW)
    s, a, i = raw[:, 1], raw[:, 2], raw[:, 3]
    src = dice_iou_from_counts(raw[:, 4:7])[0]
    return torch.cat([raw[:, 0].double(), (s + a - 2 * i).double(), (2 * i).double(), (s + a).double(), src.double()])


def _add_guard(acc: torch.Tensor, c: torch.Tensor, vol: Dict[str, torch.Tensor]) -> None:
    """Rows: fallbacks, flips, sum of agreement and its count (s + a > 0), sum of source Dice, sum of Dice - source Dice,
    harmed volumes, valid volumes (Dice's own rule: a non-empty ground truth), volumes."""
    fb, flips, num, den, src = c.reshape(GUARD_COLUMNS, -1)
    valid, dice = vol["valid"], vol["dice"]
    ok = (den > 0).to(torch.float64)
    acc[0] += fb
    acc[1] += flips
    acc[2] += torch.where(den > 0, num / torch.where(den > 0, den, 1.0), 0.0)
    acc[3] += ok
    acc[4] += torch.where(valid > 0, src, 0.0)
    acc[5] += torch.where(valid > 0, dice - src, 0.0)
    acc[6] += ((valid > 0) & (dice < src)).to(torch.float64)
    acc[7] += valid
    acc[8] += 1.0


def _guard_keys(out, prefix, acc, regions, p) -> None:
    _mean_keys(out, prefix, regions, "guard_fallback", acc[0], acc[8])
    _mean_keys(out, prefix, regions, "guard_agreement", acc[2], acc[3], avg=False)
    _mean_keys(out, prefix, regions, "guard_flips", acc[1], acc[8], avg=False)
    _mean_keys(out, prefix, regions, "src_dc", acc[4], acc[7])
    _mean_keys(out, prefix, regions, "dc_gain", acc[5], acc[7], avg=False)
    _mean_keys(out, prefix, regions, "harmed", acc[6], acc[7], avg=False)


def _calibration_keys(out, prefix, acc, regions, p) -> None:
    for col, key in enumerate(("ece", "brier", "nll")):
        _mean_keys(out, prefix, p[1], key, acc[:, col], acc[:, 3])


# The optional blocks of a table row, in column order; the same order governs the metric keys.  A row is
#     index, domain_id, loss, dice[R], iou[R], valid[R]
# and then, for every enabled block, what its ``*_columns`` function makes of one volume (one column's or one tolerance's
# regions after another).  Region-wise NSD is valid where Dice's ``valid`` is, lesion-wise NSD where the ``valid`` row of the
# volume's lesion-wise columns is.  The calibration, the volume's raw table of ``ops.calibration_bins``, is last, so
# ``reliability_from_table`` finds it at the row's end; the guard's block (``method.guard``, switched on by ``seg_tta_eval``
# alone and passed to ``add_row`` by name only) sits right before it.
BLOCKS: Tuple[Block, ...] = (
    Block("surface", lambda R, p: 2 * R, lambda R, p: (3, R), lambda v: v["surface"], _add_surface, _surface_keys),
    Block("components", lambda R, p: 3 * R, lambda R, p: (4, R), lambda v: stat_columns(v["components"]), _add_sums,
          _component_keys),
    Block("fill_nest", lambda R, p: FILL_NEST_COLUMNS * R, lambda R, p: (FILL_NEST_COLUMNS + 1, R),
          lambda v: stat_columns(v["fill_nest"]), _add_sums, _fill_nest_keys),
    Block("lesionwise", lambda R, p: LESIONWISE_COLUMNS * R, lambda R, p: (LESIONWISE_COLUMNS + 1, R),
          lambda v: lesionwise_columns(v["lesionwise"]), _add_lesionwise, _lesionwise_keys),
    Block("lesionwise_hd95", lambda R, p: LESIONWISE_HD95_COLUMNS * R, lambda R, p: (4, R),
          lambda v: lesionwise_hd95_columns(v["lesionwise"], v["lesionwise_hd95"], v["penalty"]), _add_lesionwise_hd95,
          _lesionwise_hd95_keys),
    Block("lesionwise_nsd", lambda R, p: _n(p) * R, lambda R, p: (2, _n(p), R),
          lambda v: lesionwise_nsd_columns(v["lesionwise"], v["lesionwise_nsd"]),
          lambda acc, c, vol: _add_nsd(acc, c, vol["lesionwise"].reshape(LESIONWISE_COLUMNS, -1)[1]), _nsd_keys("lw_nsd")),
    Block("surface_dice", lambda R, p: _n(p) * R, lambda R, p: (2, _n(p), R), lambda v: surface_dice_columns(v["surface_dice"]),
          lambda acc, c, vol: _add_nsd(acc, c, vol["valid"]), _nsd_keys("nsd")),
    Block("guard", lambda R, p: GUARD_COLUMNS * R, lambda R, p: (9, R), lambda v: guard_columns(v["guard"]), _add_guard,
          _guard_keys),
    Block("calibration", lambda R, p: _n(p[1]) * (3 * p[0] + 2), lambda R, p: (_n(p[1]), 4 + 3 * p[0]),
          lambda v: v["calibration"].reshape(-1), _add_calibration, _calibration_keys),
)


class Layout(NamedTuple):
    width: int                      # doubles per row
    slices: Dict[str, slice]        # the enabled blocks' columns, in column order
    params: Dict[str, Any]          # every block's parameter; false or empty = off


def table_layout(regions: Any, surface: bool = False, bins: int = 0, calibration_regions: Any = None,
                 components: bool = False, lesionwise: bool = False, fill_nest: bool = False, lesionwise_hd95: bool = False,
                 surface_dice: Any = (), lesionwise_nsd: Any = (), guard: bool = False) -> Layout:
    """Where the enabled blocks sit in a row.  ``regions`` and ``calibration_regions`` are names, or just how many there are;
    ``bins`` > 0 switches the calibration on, with one row per calibration region (default: the regions; ``["all"]`` for a
    softmax head); ``surface_dice`` and ``lesionwise_nsd`` are tolerances in mm, or their number; ``guard``: the guard's
    block (fall-backs, agreement with and Dice of the pre-adaptation prediction)."""
    R = _n(regions)
    params = {"surface": surface, "components": components, "fill_nest": fill_nest, "lesionwise": lesionwise,
              "lesionwise_hd95": lesionwise_hd95, "lesionwise_nsd": lesionwise_nsd, "surface_dice": surface_dice,
              "guard": bool(guard),
              "calibration": (int(bins), regions if calibration_regions is None else calibration_regions) if bins else None}
    at, slices = 3 + 3 * R, {}
    for b in BLOCKS:
        if params[b.name]:
            slices[b.name] = slice(at, at + b.width(R, params[b.name]))
            at = slices[b.name].stop
    return Layout(at, slices, params)


def table_width(R: int, surface: bool = False, bins: int = 0, rout: Optional[int] = None, **switches) -> int:
    """Doubles per table row for the switches of ``table_layout``; ``rout``: the calibration's rows, default R."""
    return table_layout(R, surface, bins, rout, **switches).width


ADD_ROW_POSITIONAL = ("calibration", "components", "lesionwise", "fill_nest", "lesionwise_hd95", "surface_dice", "lesionwise_nsd")


class RegionAccumulator:
    """float64 sums / counts per region, overall and per domain (reference seg_eval.py:250-270,363-378), for Dice / IoU and
    for every block the switches of ``table_layout`` enable; ``reliability`` pools the calibration bins of every row."""

    def __init__(self, region_order: Sequence[str], *switches, **named):
        self.regions = list(region_order)
        self.layout = table_layout(self.regions, *switches, **named)
        self.blocks = [b for b in BLOCKS if b.name in self.layout.slices]
        for name, p in self.layout.params.items():       # acc.lesionwise, acc.surface_dice, ...: the switches as given
            setattr(self, name, p)
        self.bins, self.cal_regions = self.layout.params["calibration"] or (0, self.regions)
        R = len(self.regions)
        shapes = {"dice": (3, R)}            # sum_dice, sum_iou, count
        shapes.update({b.name: b.shape(R, self.layout.params[b.name]) for b in self.blocks})
        # one accumulator per block and domain; the key None holds the whole split
        self.acc = {name: defaultdict(lambda s=s: torch.zeros(s, dtype=torch.float64)) for name, s in shapes.items()}
        self.total_loss, self.n_samples = 0.0, 0

    @property
    def reliability(self) -> torch.Tensor:
        """The pooled reliability diagram, float64 [rows, bins, 3] = (count, sum of confidence, correct count)."""
        if not self.bins:
            return torch.zeros((_n(self.cal_regions), 0, 3), dtype=torch.float64)
        return self.acc["calibration"][None][:, 4:].reshape(-1, self.bins, 3).clone()

    def add_row(self, dice: Sequence[float], iou: Sequence[float], valid: Sequence[bool], domain: str,
                hd95: Optional[Sequence[float]] = None, asd: Optional[Sequence[float]] = None, *earlier: Any, **cols: Any) -> None:
        """One volume.  ``cols``: the columns of every enabled block under the block's name, as the table holds them
        (``hd95`` and ``asd`` together are the ``surface`` block's).  ``earlier``: callers from before the block list pass
        some columns by position (``ADD_ROW_POSITIONAL``); that order is frozen, a new block is passed by name only."""
        if len(earlier) > len(ADD_ROW_POSITIONAL):
            raise TypeError(f"add_row takes at most {len(ADD_ROW_POSITIONAL)} columns by position, got {len(earlier)}")
        cols.update(zip(ADD_ROW_POSITIONAL, earlier))
        unknown = set(cols) - set(self.layout.params)
        if unknown:
            raise TypeError(f"add_row: no such block {sorted(unknown)}")
        vol = {k: torch.as_tensor(v, dtype=torch.float64).reshape(-1) for k, v in cols.items() if v is not None}
        if hd95 is not None:
            vol["surface"] = torch.cat([torch.as_tensor(hd95, dtype=torch.float64), torch.as_tensor(asd, dtype=torch.float64)])
        vol["valid"] = torch.tensor([1.0 if bool(v) else 0.0 for v in valid], dtype=torch.float64)
        both = torch.stack([torch.as_tensor(dice, dtype=torch.float64), torch.as_tensor(iou, dtype=torch.float64)])
        vol["dice"] = both[0]
        for dom in (None, domain):
            acc = self.acc["dice"][dom]
            acc[:2] += torch.where(vol["valid"] > 0, both, 0.0)
            acc[2] += vol["valid"]
            for b in self.blocks:
                b.add(self.acc[b.name][dom], vol[b.name], vol)

    def add_table(self, table: torch.Tensor, domain_names: Sequence[str], with_loss: bool) -> None:
        """The rows of a per-volume table, in their order; ``with_loss``: each row's loss as one sample."""
        R = len(self.regions)
        for row in table:
            d = int(row[1].item())
            cols = {name: row[s] for name, s in self.layout.slices.items()}
            if "surface" in cols:               # Dice, IoU, HD95 and ASD are fp32 values, read as such
                cols["surface"] = cols["surface"].to(torch.float32)
            self.add_row(row[3:3 + R].to(torch.float32), row[3 + R:3 + 2 * R].to(torch.float32),
                         (row[3 + 2 * R:3 + 3 * R] > 0.5).tolist(), domain_names[d] if 0 <= d < len(domain_names) else "", **cols)
            if with_loss:
                self.add_loss(float(row[2].item()), 1)

    def add_loss(self, loss: float, batch: int) -> None:
        self.total_loss += float(loss) * batch
        self.n_samples += batch

    def _keys(self, out: Dict[str, float], prefix: str, dom: Optional[str], loss: Optional[float] = None) -> None:
        acc = self.acc["dice"][dom]
        _mean_keys(out, prefix, self.regions, "dc", acc[0], acc[2])
        out[f"{prefix}miou"] = _avg(_fin(acc[1], acc[2]), acc[2])
        if loss is not None:
            out["jc"] = out["miou"]
            out["loss"] = loss
        for b in self.blocks:
            b.keys(out, prefix, self.acc[b.name][dom], self.regions, self.layout.params[b.name])

    def metrics(self, report_loss: bool) -> Dict[str, float]:
        out: Dict[str, float] = {}
        self._keys(out, "", None, float(self.total_loss / max(1, self.n_samples)) if report_loss else 0.0)
        for dom in sorted(d for d in self.acc["dice"] if d is not None):
            self._keys(out, f"dom/{dom if dom != '' else 'unknown'}/", dom)
        return out


def metrics_from_table(table: torch.Tensor, region_order: Sequence[str], domain_names: Sequence[str], report_loss: bool,
                       *switches, **named) -> Dict[str, float]:
    """Replay the reference aggregation over gathered rows in volume-index order: the result is identical to a
    single-process run (float64 sums, order fixed by index).  The switches are those of ``table_layout``."""
    acc = RegionAccumulator(region_order, *switches, **named)
    acc.add_table(table, domain_names, report_loss)
    return acc.metrics(report_loss)


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
    gather_masks = False         # seg_tta_eval's `evaluation.gather_masks`: keep the scored mask for the second collective

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
        # hole filling and ET < TC < WT nesting of the filtered mask, in place right after the filter; the pass is queued
        # only when post-processing is on and a region fills or a chain is given, and only then do its keys appear
        (self.postprocess_fill_holes, self.postprocess_fill_connectivity, self.postprocess_max_hole_voxels,
         self.postprocess_nesting, self.postprocess_nesting_mode) = fill_nest_config(self.config)
        self.enable_fill_nest = self.enable_postprocess and (any(self.postprocess_fill_holes) or bool(self.postprocess_nesting))
        # lesion-wise Dice and detection counts on the GPU, off by default: ground-truth lesions (dilated, 26-connected)
        # against the predicted components of the mask that is scored (the filtered one with post-processing on)
        (self.enable_lesionwise, self.lesionwise_dilation, self.lesionwise_connectivity,
         self.lesionwise_min_voxels) = lesionwise_config(self.config)
        if self.enable_lesionwise and bool(get_config(self.config, "training.criterion.softmax", False)):
            raise NotImplementedError("evaluation.lesionwise.enable: lesion-wise scores are defined for the sigmoid-region head "
                                      "only (training.criterion.softmax is set)")
        # lesion-wise HD95 on top of that, off by default: one more pass behind the lesion-wise scores, on their scratch
        (self.enable_lesionwise_hd95, self.lesionwise_hd95_percentile,
         self.lesionwise_hd95_penalty) = lesionwise_hd95_config(self.config)
        # normalised surface Dice at tolerances in mm, off by default: region-wise on the final mask (one bounded search over
        # bit-packed edge masks, no distance transform), and lesion-wise behind the lesion-wise scores, on their scratch
        self.enable_surface_dice, self.surface_dice_tolerances = surface_dice_config(self.config)
        self.enable_lesionwise_nsd, self.lesionwise_nsd_tolerances = lesionwise_nsd_config(self.config)
        for on, key in ((self.enable_surface_dice, "evaluation.surface_dice.enable"),
                        (self.enable_lesionwise_nsd, "evaluation.lesionwise.nsd.enable")):
            if on and bool(get_config(self.config, "training.criterion.softmax", False)):
                raise NotImplementedError(f"{key}: the normalised surface Dice is defined for the sigmoid-region head only "
                                          f"(training.criterion.softmax is set)")
        # input pre-pass on the GPU (raw volumes in, the reference's `_normalize_img` applied here instead of in the
        # dataset worker; reference src/datasets/transforms.py:129-223).  The NIfTI datasets of this package hand over
        # raw intensities, so the pre-pass defaults to on for them and to off for the synthetic source (already
        # normalised); `training.data.transforms.normalize_on_device` overrides either way.
        tcfg = get_config(self.config, "training.data.transforms", {}) or {}
        synthetic = bool(get_config(self.config, "dataset.synthetic.enabled", True))
        nod = get_config(tcfg, "normalize_on_device", None)
        self.normalize_on_device = (not synthetic) if nod is None else bool(nod)
        self._tcfg = tcfg
        self.enable_guard = False          # seg_tta_eval with ``method.guard.enable``: the guard's block of the table

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

    component_columns = fill_nest_columns = staticmethod(stat_columns)

    def switches(self) -> Dict[str, Any]:
        """The table's switches as ``table_layout`` takes them, from the ``enable_*`` attributes as they stand now."""
        return dict(surface=self.enable_surface, bins=self.cal_bins, calibration_regions=self.calibration_regions,
                    components=self.enable_postprocess, fill_nest=self.enable_fill_nest, lesionwise=self.enable_lesionwise,
                    lesionwise_hd95=self.enable_lesionwise_hd95, surface_dice=self.sd_tolerances,
                    lesionwise_nsd=self.ln_tolerances, guard=self.enable_guard)

    def layout(self) -> Layout:
        return table_layout(self.region_order, **self.switches())

    def queue_passes(self, logits: torch.Tensor, y: torch.Tensor, channels_last: bool = False) -> Dict[str, Any]:
        """Queue every enabled pass over logits [B,R,D,H,W] (or their channels-last view) and labels on the current stream ->
        the job: device tensors, nothing read.  ``counts`` int64 [B,R,3] are those of the mask that is scored - thresholded,
        then filtered in place with ``evaluation.postprocess.enable``, then filled and nested - and ``raw`` holds what each
        further pass left, by block; calibration and the reported loss stay on the logits.  ``table_rows`` reads it."""
        B, R = y.shape[0], y.shape[1]
        if not (logits.ndim == 5 and (logits.shape[-1] if channels_last else logits.shape[1]) == R):
            raise ValueError(f"[BratsSegEval] model logits must be [B,{R},D,H,W], got {tuple(logits.shape)}")
        on = self.layout().slices
        counts = torch.empty((B, R, 3), dtype=torch.int64, device=y.device)
        need_mask = self.gather_masks or bool(on.keys() - {"calibration", "guard"})       # every other block reads the mask
        mask = torch.empty(tuple(y.shape), dtype=torch.uint8, device=y.device) if need_mask else None
        ops.mask_dice_counts(logits, y, self.threshold, counts, mask, logits_channels_last=channels_last)
        raw: Dict[str, Any] = {}
        if "components" in on:           # in place: every pass below and the gathered masks take the filtered mask
            counts, raw["components"] = self.postprocess_launch(mask, y)
        if "fill_nest" in on:            # likewise in place, right behind the filter: its counts replace the filter's
            counts, raw["fill_nest"] = self.fill_nest_launch(mask, y)
        if "lesionwise_hd95" in on:      # right behind the counts, on the mask they describe; the HD95 pass on the same scratch
            raw["lesionwise"], raw["lesionwise_hd95"] = self.lesionwise_hd95_launch(mask, y)
        elif "lesionwise" in on:
            raw["lesionwise"] = self.lesionwise_launch(mask, y)
        if "lesionwise_nsd" in on:       # directly behind the lesion-wise passes, same stream and mask: it reads their scratch
            raw["lesionwise_nsd"] = self.lesionwise_nsd_launch(mask)
        if "surface_dice" in on:         # on the final mask, like the surface distances
            raw["surface_dice"] = self.surface_dice_launch(mask, y)
        job: Dict[str, Any] = {"counts": counts, "shape": tuple(y.shape[2:]), "mask": mask, "raw": raw,
                               "penalty": self.lesionwise_hd95_penalty_mm(y.shape[2:])}
        if self.report_loss:
            job["loss"] = self.loss_fn.launch(logits, y, channels_last=channels_last)
        if "surface" in on:
            raw["surface"] = self.surface_launch(mask, y)
        if "calibration" in on:
            raw["calibration"] = self.calibration_launch(logits, y, channels_last=channels_last)
        return job

    def table_rows(self, job: Dict[str, Any]) -> List[torch.Tensor]:
        """First host read of a queued job (with ``index`` and ``domain_id`` per volume added) -> the table rows of its
        volumes, the blocks in the order of ``BLOCKS``."""
        counts = job["counts"].cpu()
        dice, iou, valid = dice_iou_from_counts(counts)
        B = counts.shape[0]
        losses = [0.0] * B
        if "loss" in job:
            out, *dims = job["loss"]
            job["loss"] = (out.cpu(), *dims)         # one read serves the per-volume values and the batch's
            losses = self.loss_fn.values_per_volume(job["loss"])
        host = {k: v.cpu() for k, v in job["raw"].items() if torch.is_tensor(v)}
        if "surface" in job["raw"]:
            hd, asd = self.surface_fix(*job["raw"]["surface"], counts, job["shape"])
            host["surface"] = torch.cat([hd.double(), asd.double()], dim=1)
        blocks = [b for b in BLOCKS if b.name in self.layout().slices]
        rows = []
        for i in range(B):
            vol = dict({k: v[i] for k, v in host.items()}, penalty=job.get("penalty"))
            rows.append(torch.cat([torch.tensor([job["index"][i], job["domain_id"][i], losses[i]], dtype=torch.float64),
                                   dice[i].double(), iou[i].double(), valid[i].double()] + [b.columns(vol) for b in blocks]))
        return rows

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

    @torch.no_grad()
    def evaluate_epoch(self, model: torch.nn.Module, data_loader: Iterable, device) -> Dict[str, float]:
        """Single process: the reference's loop and aggregation (seg_eval.py:276-460), over the per-volume table rows; the
        reported loss is the batch's value times the batch size, as the reference forms it.  Under an initialised
        ``torch.distributed`` group with more than one rank ``data_loader`` is this rank's shard: the tables are merged
        (``merge_rank_tables``) and every rank reports the metrics of the WHOLE split - a rank never prints the metrics of
        its shard as if they were the test set."""
        import torch.distributed as dist

        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        model.eval()
        model.to(device)
        rows: List[torch.Tensor] = []
        domain_names: List[str] = []
        batch_losses: List[Tuple[float, int]] = []
        for batch in data_loader:
            x, y = self.check_batch(batch, device)
            job = self.queue_passes(model(x).float(), y)
            domains = as_list_str(batch.get("domain", None), batch_size=x.size(0))
            idx = batch.get("index", None)
            if idx is None and world > 1:
                raise KeyError("[seg_eval] a sharded evaluation needs batch['index'] (the volume's position in the whole split): "
                               "rank-local counters collide across ranks")
            domain_names += [d for d in dict.fromkeys(domains) if d not in domain_names]
            job.update(index=[int(idx[i]) if idx is not None else len(rows) + i for i in range(x.size(0))],
                       domain_id=[domain_names.index(d) for d in domains])
            rows += self.table_rows(job)
            if world == 1 and self.report_loss:
                batch_losses.append((self.loss_fn.value(job["loss"]), x.size(0)))
        table = torch.stack(rows) if rows else torch.empty((0, self._table_width()), dtype=torch.float64)
        if world == 1:
            return self._metrics_of(table, domain_names, batch_losses)
        table, domain_names = merge_rank_tables(table, domain_names, device)
        self.last_table = table
        return self._metrics_of(table, domain_names)

    def _table_width(self) -> int:
        return self.layout().width

    def _metrics_of(self, table: torch.Tensor, domain_names: Sequence[str],
                    batch_losses: Optional[List[Tuple[float, int]]] = None) -> Dict[str, float]:
        """Metrics of the whole split from its per-volume table (and ``last_reliability`` with calibration on); the loss from
        the rows, or from ``batch_losses`` = (value, batch size) per batch where given."""
        acc = RegionAccumulator(self.region_order, **self.switches())
        acc.add_table(table, domain_names, self.report_loss and batch_losses is None)
        for loss, n in batch_losses or []:
            acc.add_loss(loss, n)
        if self.enable_calibration:
            self.last_reliability = acc.reliability
        return acc.metrics(self.report_loss)


# ----------------------------------------------------------------------------- sharding
def shard_indices(n_items: int, rank: int, world: int) -> List[int]:
    """Round-robin, deterministic: volume i -> rank i mod W."""
    return list(range(rank, n_items, world))



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
        # the do-no-harm guard (guard.py): the table takes its block and ``_submit`` scores the reference prediction as well
        self.enable_guard = guard_enabled(self.config)
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
        res = self.plugins[lane].adapt_volume(xb)
        job = self.queue_passes(res["logits_cl"], yb, channels_last=True)
        if self.enable_guard:
            job["raw"]["guard"] = self.guard_launch(res, yb)
        job["keep"] = (xb, yb, res)
        return job

    def guard_launch(self, res: Dict[str, Any], y: torch.Tensor) -> torch.Tensor:
        """Queue the scoring of the guard's reference prediction on the current stream -> device int64 [B,R,7] = (fallback,
        s, a, i, then inter, pred, gt of the reference's mask).  That mask is thresholded like the returned one and, with the
        blocks on, filtered, filled and nested in place like it (its post-processing stats are discarded): the source Dice
        and ``<region>_dc`` describe masks that went through the same pipeline."""
        B, R = y.shape[0], y.shape[1]
        on = self.layout().slices
        counts = torch.empty((B, R, 3), dtype=torch.int64, device=y.device)
        mask = torch.empty(tuple(y.shape), dtype=torch.uint8, device=y.device) if "components" in on else None
        ops.mask_dice_counts(res["guard_reference_cl"], y, self.threshold, counts, mask, logits_channels_last=True)
        if "components" in on:
            counts, _ = self.postprocess_launch(mask, y)
        if "fill_nest" in on:
            counts, _ = self.fill_nest_launch(mask, y)
        return torch.cat([res["guard_fallback"].to(torch.int64).unsqueeze(-1), res["guard_counts"], counts], dim=-1)

    def _finish(self, job: Dict[str, Any]) -> List[torch.Tensor]:
        """First host read of a queued group -> the table rows of its volumes."""
        rows = self.table_rows(job)
        if self.gather_masks:
            mk = job["mask"].cpu()
            for b in range(len(rows)):
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
