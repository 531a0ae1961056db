"""Lesion-wise HD95, everything that needs no GPU: the config block, the score formed from the device's integers, the widened
per-volume table and its replay, and the argument checks of the C entry point."""
import ctypes

import pytest
import torch

from multimodal_tta_amd.evaluation import (RegionAccumulator, SegmentationEvaluationStrategy, lesionwise_columns,
                                           lesionwise_config, lesionwise_hd95_columns, lesionwise_hd95_config,
                                           metrics_from_table, table_width, volume_diagonal_mm)

Q1 = 1 << 30
Q20 = 1 << 20


def _cfg(lw=None, spacing=None, **hd):
    cfg = {"evaluation": {"lesionwise": dict(lw if lw is not None else {"enable": True})}}
    cfg["evaluation"]["lesionwise"]["hd95"] = dict(hd)
    if spacing is not None:
        cfg["evaluation"]["seg"] = {"spacing": list(spacing)}
    return cfg


# ----------------------------------------------------------------------------- config
def test_config_defaults_and_values():
    assert lesionwise_hd95_config({}) == (False, 95.0, "diagonal")
    assert lesionwise_hd95_config({"evaluation": {"lesionwise": {"enable": True}}}) == (False, 95.0, "diagonal")
    assert lesionwise_hd95_config(_cfg(enable=True)) == (True, 95.0, "diagonal")
    assert lesionwise_hd95_config(_cfg(enable=True, percentile=100, penalty=374)) == (True, 100.0, 374.0)
    assert lesionwise_hd95_config(_cfg(lw={"enable": False}, percentile=0.0, penalty=12.5)) == (False, 0.0, 12.5)
    assert lesionwise_config(_cfg(enable=True)) == (True, 3, 18, [0, 0, 0])          # still the 4-tuple, the sub-block is not its business
    off = SegmentationEvaluationStrategy({})
    assert not off.enable_lesionwise_hd95 and off.lesionwise_hd95_percentile == 95.0 and off.lesionwise_hd95_penalty == "diagonal"
    on = SegmentationEvaluationStrategy(_cfg(enable=True, penalty=374))
    assert on.enable_lesionwise and on.enable_lesionwise_hd95 and on.lesionwise_hd95_penalty == 374.0


@pytest.mark.parametrize("hd,key", [
    (dict(enable="on"), "evaluation.lesionwise.hd95.enable"),
    (dict(enable=1), "evaluation.lesionwise.hd95.enable"),
    (dict(percentile=-1), "evaluation.lesionwise.hd95.percentile"),
    (dict(percentile=100.5), "evaluation.lesionwise.hd95.percentile"),
    (dict(percentile="95"), "evaluation.lesionwise.hd95.percentile"),
    (dict(percentile=True), "evaluation.lesionwise.hd95.percentile"),
    (dict(percentile=float("nan")), "evaluation.lesionwise.hd95.percentile"),
    (dict(penalty="volume"), "evaluation.lesionwise.hd95.penalty"),
    (dict(penalty=0), "evaluation.lesionwise.hd95.penalty"),
    (dict(penalty=-374), "evaluation.lesionwise.hd95.penalty"),
    (dict(penalty=True), "evaluation.lesionwise.hd95.penalty"),
    (dict(penalty=float("inf")), "evaluation.lesionwise.hd95.penalty"),
    (dict(penalty=[374]), "evaluation.lesionwise.hd95.penalty"),
])
@pytest.mark.parametrize("enabled", [True, False])
def test_config_bad_values_name_their_key(hd, key, enabled):
    lw = {"enable": enabled}
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + r"\b"):
        lesionwise_hd95_config(_cfg(lw=lw, **hd))
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + r"\b"):
        SegmentationEvaluationStrategy(_cfg(lw=lw, **hd))


def test_hd95_needs_the_lesionwise_block():
    for lw in ({"enable": False}, {}):
        with pytest.raises(ValueError, match=r"evaluation\.lesionwise\.hd95\.enable needs evaluation\.lesionwise\.enable"):
            lesionwise_hd95_config(_cfg(lw=lw, enable=True))
        with pytest.raises(ValueError, match=r"evaluation\.lesionwise\.enable"):
            SegmentationEvaluationStrategy(_cfg(lw=lw, enable=True))


def test_softmax_head_stays_refused():
    cfg = _cfg(enable=True)
    cfg["training"] = {"criterion": {"softmax": True}}
    with pytest.raises(NotImplementedError, match=r"evaluation\.lesionwise"):
        SegmentationEvaluationStrategy(cfg)


def test_shipped_configs_leave_the_block_off():
    from multimodal_tta_amd.config import compose
    for task in ("brats", "hecktor21"):
        cfg = compose(overrides=[f"task={task}", "model=unet"])
        assert lesionwise_hd95_config(cfg) == (False, 95.0, "diagonal")
        assert not SegmentationEvaluationStrategy(cfg).enable_lesionwise_hd95


def test_penalty_diagonal_is_the_surface_penalty():
    from oracle.surface import diag_mm
    for shape, spacing in (((128, 128, 128), (1.0, 1.0, 1.0)), ((9, 17, 40), (1.5, 0.8, 2.0)), ((1, 1, 1), (2.0, 2.0, 2.0))):
        strat = SegmentationEvaluationStrategy(_cfg(spacing=spacing, enable=True))
        assert strat.lesionwise_hd95_penalty_mm(shape) == diag_mm(*shape, spacing) == volume_diagonal_mm(shape, spacing)
        assert SegmentationEvaluationStrategy(_cfg(spacing=spacing, enable=True, penalty=374)).lesionwise_hd95_penalty_mm(shape) == 374.0
        # surface_fix applies the same figure
        hd, asd = strat.surface_fix(torch.tensor([[float("nan")]]), torch.tensor([[float("inf")]]), torch.tensor([[[0, 0, 5]]]), shape)
        assert hd.item() == asd.item() == torch.tensor(diag_mm(*shape, spacing), dtype=torch.float32).item()


# ----------------------------------------------------------------------------- the score of one volume
def test_columns_of_one_volume():
    pen = 374.0
    # lesions, kept, found, predicted, matched, dice_q, fp voxels
    stats = torch.tensor([[3, 3, 2, 4, 2, Q1, 9],              # 2 scored, 1 missed, 2 false positives
                          [0, 0, 0, 2, 0, 0, 5],               # GT-empty with false positives: the penalty
                          [0, 0, 0, 0, 0, 0, 0],               # nothing to find, nothing predicted: invalid
                          [1, 0, 0, 1, 1, 0, 0],               # the only lesion is below min_lesion_voxels, its component matched: invalid
                          [2, 2, 2, 2, 2, Q1, 0],              # everything found
                          [2, 2, 2, 1, 1, Q1, 0]],             # ... but the lists overflowed
                         dtype=torch.int64)
    hd_stats = torch.tensor([[3 * Q20 + Q20 // 2, 2, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [5 * Q20, 2, 0], [0, 0, 2]], dtype=torch.int64)
    c = lesionwise_hd95_columns(stats, hd_stats, pen).reshape(2, 6)
    assert c.dtype == torch.float64
    assert c[0].tolist() == [(3.5 + pen * (1 + 2)) / (3 + 2), pen, 0.0, 0.0, 2.5, 0.0]
    assert c[1].tolist() == [1.0, 1.0, 0.0, 0.0, 1.0, -1.0]
    # an unmatched lesion alone: exactly the penalty
    one = lesionwise_hd95_columns(torch.tensor([[1, 1, 0, 0, 0, 0, 0]]), torch.tensor([[0, 0, 0]]), 88.5)
    assert one.tolist() == [88.5, 1.0]
    # the integers reach the score whole
    big = lesionwise_hd95_columns(torch.tensor([[4000, 4000, 4000, 4000, 4000, 0, 0]]), torch.tensor([[4000 * 300 * Q20 + 1, 4000, 0]]), pen)
    assert big[0].item() == float(4000 * 300 * Q20 + 1) / float(Q20) / 4000.0


# ----------------------------------------------------------------------------- table layout and replay
def test_table_width_places_the_columns_behind_the_lesionwise_ones():
    R = 2
    for surface in (False, True):
        base = table_width(R, surface)
        assert base == 3 + (5 if surface else 3) * R
        assert table_width(R, surface, lesionwise_hd95=False) == base
        assert table_width(R, surface, lesionwise=True, lesionwise_hd95=False) == base + 7 * R
        assert table_width(R, surface, lesionwise=True, lesionwise_hd95=True) == base + 9 * R
        assert table_width(R, surface, 4, 1, components=True, fill_nest=True, lesionwise=True, lesionwise_hd95=True) == \
            table_width(R, surface, 4, 1, components=True, fill_nest=True, lesionwise=True) + 2 * R


PEN = 100.0
# three volumes, two regions (A, B), domains d0 / d1 / d0
STATS = [[[2, 2, 1, 3, 1, Q1 // 2, 7], [0, 0, 0, 0, 0, 0, 0]],          # A: (4 + 100 (1 + 2)) / 4 = 76; B: invalid
         [[1, 1, 1, 1, 1, Q1, 0], [0, 0, 0, 2, 0, 0, 11]],              # A: 1.5 / 1; B: GT-empty with 2 false positives: 100
         [[3, 3, 3, 1, 1, 0, 0], [1, 1, 1, 2, 2, Q1 // 4, 0]]]          # A: overflowed; B: 0.25 / 1
HD = [[[4 * Q20, 1, 0], [0, 0, 0]],
      [[Q20 + Q20 // 2, 1, 0], [0, 0, 0]],
      [[0, 0, 3], [Q20 // 4, 1, 0]]]
DOMS = [0, 1, 0]
WANT = {"a_lw_hd95": (76.0 + 1.5) / 2, "b_lw_hd95": (100.0 + 0.25) / 2, "a_lw_hd95_overflow": 1.0 / 3, "b_lw_hd95_overflow": 0.0,
        "dom/d0/a_lw_hd95": 76.0, "dom/d0/b_lw_hd95": 0.25, "dom/d0/a_lw_hd95_overflow": 0.5, "dom/d0/b_lw_hd95_overflow": 0.0,
        "dom/d1/a_lw_hd95": 1.5, "dom/d1/b_lw_hd95": 100.0, "dom/d1/a_lw_hd95_overflow": 0.0, "dom/d1/b_lw_hd95_overflow": 0.0}
WANT["avg_lw_hd95"] = (WANT["a_lw_hd95"] + WANT["b_lw_hd95"]) / 2
WANT["dom/d0/avg_lw_hd95"] = (76.0 + 0.25) / 2
WANT["dom/d1/avg_lw_hd95"] = (1.5 + 100.0) / 2


def _hand_rows(surface, bins, components):
    rows = []
    for i in range(3):
        row = [float(i), float(DOMS[i]), 0.25 * (i + 1), 0.5 + 0.1 * i, 0.7, 0.4, 0.5, 1.0, 1.0 if i != 1 else 0.0]
        if surface:
            row += [2.0 + i, 3.0, 1.0, 0.5 + i]
        if components:
            row += [3.0, 1.0, 1.0, 1.0, 40.0 * i, 0.0]
        st, hs = torch.tensor(STATS[i], dtype=torch.int64), torch.tensor(HD[i], dtype=torch.int64)
        row += lesionwise_columns(st).tolist()
        mark = len(row)
        row += lesionwise_hd95_columns(st, hs, PEN).tolist()
        if bins:
            for r in range(2):
                row += [0.0] * (3 * (bins - 1)) + [10.0, 9.0, 8.0 + r, 1.0, 2.0]
        rows.append(row)
    return torch.tensor(rows, dtype=torch.float64), mark


@pytest.mark.parametrize("components", [False, True])
@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("bins", [0, 4])
def test_metrics_from_table_reads_the_hd95_columns(surface, bins, components):
    regions = ["A", "B"]
    table, mark = _hand_rows(surface, bins, components)
    assert table.shape[1] == table_width(2, surface, bins, components=components, lesionwise=True, lesionwise_hd95=True)
    assert mark == table_width(2, surface, components=components, lesionwise=True)       # directly behind the lesion-wise columns
    m = metrics_from_table(table, regions, ["d0", "d1"], True, surface, bins, components=components, lesionwise=True,
                           lesionwise_hd95=True)
    for k, v in WANT.items():
        assert m[k] == v, (k, m[k], v)
    # the other keys are those of the same table without the HD95 columns
    plain = torch.cat([table[:, :mark], table[:, mark + 4:]], 1)
    base = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, bins, components=components, lesionwise=True)
    assert {k: m[k] for k in base} == base and set(m) == set(base) | set(WANT)
    # the accumulator fed row by row gives the same
    acc = RegionAccumulator(regions, lesionwise=True, lesionwise_hd95=True)
    assert acc.lesionwise_hd95
    for i in range(3):
        st, hs = torch.tensor(STATS[i], dtype=torch.int64), torch.tensor(HD[i], dtype=torch.int64)
        acc.add_row([0.5, 0.5], [0.4, 0.4], [True, True], f"d{DOMS[i]}", lesionwise=lesionwise_columns(st),
                    lesionwise_hd95=lesionwise_hd95_columns(st, hs, PEN))
    direct = acc.metrics(False)
    assert {k: direct[k] for k in WANT} == WANT


def test_invalid_everywhere_reads_zero():
    acc = RegionAccumulator(["A"], lesionwise=True, lesionwise_hd95=True)
    st, hs = torch.zeros((1, 7), dtype=torch.int64), torch.zeros((1, 3), dtype=torch.int64)
    acc.add_row([0.5], [0.4], [True], "d", lesionwise=lesionwise_columns(st), lesionwise_hd95=lesionwise_hd95_columns(st, hs, 374.0))
    m = acc.metrics(False)
    assert m["a_lw_hd95"] == 0.0 and m["avg_lw_hd95"] == 0.0 and m["a_lw_hd95_overflow"] == 0.0 and m["dom/d/a_lw_hd95"] == 0.0


def test_without_the_keyword_nothing_changes():
    regions = ["A", "B"]
    for surface in (False, True):
        table, mark = _hand_rows(surface, 0, False)
        plain = table[:, :mark]
        a = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, lesionwise=True)
        b = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, lesionwise=True, lesionwise_hd95=False)
        assert a == b and list(a) == list(b) and not any("lw_hd95" in k for k in a)
        assert not RegionAccumulator(regions, surface, lesionwise=True).lesionwise_hd95
    for cfg in ({}, {"evaluation": {"lesionwise": {"enable": True}}}, _cfg(enable=False, penalty=374)):
        strat = SegmentationEvaluationStrategy(cfg)
        assert strat._table_width() == table_width(3, lesionwise=strat.enable_lesionwise)


# ----------------------------------------------------------------------------- the C entry point, without a device
def test_abi_symbols_and_argument_validation_without_a_gpu():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    assert {"mmtta_lesionwise_hd95_scratch_bytes", "mmtta_lesionwise_hd95"} <= set(_lib.exported_names())

    def call(mask=1, label=True, n=1, r=1, d=4, h=4, w=4, spacing=(1.0, 1.0, 1.0), pct=95.0, lw=1, stats=1, scratch=1,
             min_voxels=None, has_min=True, dtype=None, shape=None):
        mv = (ctypes.c_int64 * 64)(*(min_voxels or [0] * 64))
        sp = (ctypes.c_double * 3)(*spacing) if spacing is not None else None
        ln, lr, ld, lh, lw_ = shape or (n, r, d, h, w)
        t = _lib.Tensor(4096, ln, lr, ld, lh, lw_, lr * ld * lh * lw_, ld * lh * lw_, lh * lw_, lw_, 1,
                        _lib.F32 if dtype is None else dtype, 0)
        return lib.mmtta_lesionwise_hd95(mask, ctypes.byref(t) if label else None, n, r, d, h, w, sp, pct, mv if has_min else None,
                                         lw, stats, None, scratch, None)

    # (the pointers here are never followed: every call is refused before anything is queued)
    for kw, word in ((dict(mask=None), b"mask"), (dict(label=False), b"label"), (dict(spacing=None), b"spacing"),
                     (dict(has_min=False), b"min_lesion_voxels"), (dict(lw=None), b"lesionwise_scratch"),
                     (dict(stats=None), b"hd_stats"), (dict(scratch=None), b"scratch")):
        assert call(**kw) == -1 and b"null" in lib.mmtta_last_error() and word in lib.mmtta_last_error(), kw
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        assert call(spacing=bad) == -1 and b"spacing" in lib.mmtta_last_error(), bad
    for bad in (-0.5, 100.25, float("nan")):
        assert call(pct=bad) == -1 and b"percentile" in lib.mmtta_last_error(), bad
    assert call(r=65) == -2 and b"65" in lib.mmtta_last_error()
    assert call(d=0) == -1 and b"extent" in lib.mmtta_last_error()
    assert call(w=1025) == -2 and b"1024" in lib.mmtta_last_error()
    assert call(n=65535, r=2, d=1, h=1, w=1) == -2 and b"limits" in lib.mmtta_last_error()
    assert call(min_voxels=[-5] + [0] * 63) == -1 and b"min_lesion_voxels" in lib.mmtta_last_error()
    assert call(dtype=_lib.BF16) == -2 and b"fp32" in lib.mmtta_last_error()
    assert call(shape=(1, 1, 4, 4, 5)) == -1 and b"label" in lib.mmtta_last_error() and b"shape" in lib.mmtta_last_error()


def test_scratch_bytes_depend_on_the_shape_alone():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    V = 128 ** 3
    nb = lib.mmtta_lesionwise_hd95_scratch_bytes(6, 128, 128, 128)
    # twelve words and one byte per voxel, the pool (2 V packed coordinates and 2 V distances per mask) and a word per
    # slot of the pair table (2 * 64^3 slots per mask)
    assert 6 * (V * (12 * 4 + 1 + 16) + 2 * 64 ** 3 * 4) <= nb < 6 * V * 68
    assert lib.mmtta_lesionwise_hd95_scratch_bytes(1, 1, 1, 5) > 0
    assert lib.mmtta_lesionwise_hd95_scratch_bytes(1, 1024, 8, 8) > 0
    assert lib.mmtta_lesionwise_hd95_scratch_bytes(1, 1025, 8, 8) < 0
    assert lib.mmtta_lesionwise_hd95_scratch_bytes(1, 8, 8, 1025) < 0
    assert lib.mmtta_lesionwise_hd95_scratch_bytes(0, 4, 4, 4) < 0
    assert lib.mmtta_lesionwise_hd95_scratch_bytes(1, 0, 4, 4) < 0
    assert lib.mmtta_lesionwise_hd95_scratch_bytes(65536, 4, 4, 4) < 0


def test_ops_wrapper_checks_before_the_library():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    m, lab = torch.zeros((1, 1, 2, 2, 2), dtype=torch.uint8), torch.zeros((1, 1, 2, 2, 2))
    assert ops.LESIONWISE_HD_Q_ONE == Q20 and ops.LESIONWISE_HD_COLUMNS == ("hd_q", "lesions_scored", "overflow")
    with pytest.raises(MmttaError, match="spacing"):
        ops.lesionwise_hd95(m, lab, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(MmttaError, match="percentile"):
        ops.lesionwise_hd95(m, lab, percentile=101.0)
    with pytest.raises(MmttaError, match="dense"):
        ops.lesionwise_hd95(m, lab)      # not on the device
