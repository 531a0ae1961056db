"""Calibration metrics (ECE / Brier / NLL), everything that needs no GPU: the config block, the host arithmetic on the
reliability table, the widened per-volume table and its replay, and the argument checks of the C entry point."""
import ctypes

import pytest
import torch

from multimodal_tta_amd.evaluation import (RegionAccumulator, SegmentationEvaluationStrategy, calibration_config,
                                           calibration_from_bins, gather_table, metrics_from_table, reliability_from_table,
                                           table_width)

REGIONS = ["ET", "TC", "WT"]


def _cfg(**cal):
    return {"evaluation": {"calibration": dict(cal)}}


# ----------------------------------------------------------------------------- config
def test_config_defaults_and_values():
    assert calibration_config({}) == (False, 15, "volume")
    assert calibration_config(_cfg(enable=True, bins=10, scope="union")) == (True, 10, "union")
    assert calibration_config(_cfg(bins=1)) == (False, 1, "volume")
    assert calibration_config(_cfg(bins=64)) == (False, 64, "volume")
    off = SegmentationEvaluationStrategy({})
    assert not off.enable_calibration and off.cal_bins == 0 and off.last_reliability is None
    on = SegmentationEvaluationStrategy(_cfg(enable=True, bins=7, scope="union"))
    assert on.enable_calibration and on.calibration_bins == 7 and on.calibration_scope == "union"
    assert on.calibration_regions == REGIONS and not on.calibration_softmax
    sm = SegmentationEvaluationStrategy({**_cfg(enable=True), "training": {"criterion": {"softmax": True}}})
    assert sm.calibration_softmax and sm.calibration_regions == ["all"]       # the head follows training.criterion.softmax


@pytest.mark.parametrize("cal,key", [
    (dict(enable="yes"), "evaluation.calibration.enable"), (dict(enable=1), "evaluation.calibration.enable"),
    (dict(bins=0), "evaluation.calibration.bins"), (dict(bins=65), "evaluation.calibration.bins"),
    (dict(bins=7.5), "evaluation.calibration.bins"), (dict(bins=True), "evaluation.calibration.bins"),
    (dict(scope="band"), "evaluation.calibration.scope"), (dict(enable=True, scope=0), "evaluation.calibration.scope"),
])
def test_config_bad_values_name_their_key(cal, key):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        calibration_config(_cfg(**cal))
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        SegmentationEvaluationStrategy(_cfg(**cal))


def test_shipped_configs_carry_the_block_disabled():
    from multimodal_tta_amd.config import compose
    for task in ("brats", "hecktor21"):
        cfg = compose(overrides=[f"task={task}", "model=unet"])
        assert dict(cfg["evaluation"]["calibration"]) == {"enable": False, "bins": 15, "scope": "volume"}
        assert calibration_config(cfg) == (False, 15, "volume")


# ----------------------------------------------------------------------------- host arithmetic
def _hand_table():
    """Two regions, four bins (edges 0.25, 0.5, 0.75, 1), rows = [count, sum conf, correct] x 4, Brier sum, NLL sum.

    Region 0, n = 10:
        bin 2: 4 elements, sum conf 2.6 (mean 0.65), 2 correct (accuracy 0.50): (4/10) |0.50 - 0.65| = 0.06
        bin 3: 6 elements, sum conf 5.4 (mean 0.90), 6 correct (accuracy 1.00): (6/10) |1.00 - 0.90| = 0.06
        ECE = 0.12; Brier = 1.5 / 10 = 0.15; NLL = 4.0 / 10 = 0.4
    Region 1, n = 8:
        bin 1: 2 elements, sum conf 0.9 (mean 0.45), 0 correct: (2/8) |0 - 0.45|      = 0.1125
        bin 3: 6 elements, sum conf 5.7 (mean 0.95), 3 correct: (6/8) |0.5 - 0.95|    = 0.3375
        ECE = 0.45; Brier = 2.0 / 8 = 0.25; NLL = 6.0 / 8 = 0.75
    A third row has no element at all (union scope, neither prediction nor ground truth has foreground): invalid."""
    r0 = [0, 0, 0, 0, 0, 0, 4, 2.6, 2, 6, 5.4, 6, 1.5, 4.0]
    r1 = [0, 0, 0, 2, 0.9, 0, 0, 0, 0, 6, 5.7, 3, 2.0, 6.0]
    r2 = [0.0] * 14
    return torch.tensor([r0, r1, r2], dtype=torch.float64)


def test_calibration_from_bins_hand_table():
    ece, brier, nll, valid = calibration_from_bins(_hand_table())
    assert ece.dtype == brier.dtype == nll.dtype == torch.float64
    assert valid.tolist() == [True, True, False]
    assert ece[:2].tolist() == pytest.approx([0.12, 0.45], abs=1e-15)
    assert brier[:2].tolist() == pytest.approx([0.15, 0.25], abs=1e-15)
    assert nll[:2].tolist() == pytest.approx([0.4, 0.75], abs=1e-15)
    assert ece[2] == 0 and brier[2] == 0 and nll[2] == 0
    # leading shapes pass through: [volume, region, cols]
    e2, _, _, v2 = calibration_from_bins(_hand_table().reshape(1, 3, 14).expand(2, 3, 14))
    assert e2.shape == (2, 3) and v2.shape == (2, 3) and torch.equal(e2[1], ece)
    with pytest.raises(ValueError):
        calibration_from_bins(torch.zeros(2, 13, dtype=torch.float64))


def test_invalid_entries_stay_out_of_the_means():
    """Region 2 of the hand table is empty in volume A and filled in volume B: its mean is B's value alone, and avg_* is
    the mean of the three region means."""
    acc = RegionAccumulator(REGIONS, False, 4)
    a = _hand_table()
    b = _hand_table()
    b[2] = a[0]
    one = [1.0, 1.0, 1.0]
    acc.add_row(one, one, [True] * 3, "d", None, None, a)
    acc.add_row(one, one, [True] * 3, "d", None, None, b.reshape(-1))        # flat, as a table row carries it
    m = acc.metrics(False)
    assert m["et_ece"] == pytest.approx(0.12) and m["tc_ece"] == pytest.approx(0.45) and m["wt_ece"] == pytest.approx(0.12)
    assert m["avg_ece"] == pytest.approx((0.12 + 0.45 + 0.12) / 3)
    assert m["wt_brier"] == pytest.approx(0.15) and m["wt_nll"] == pytest.approx(0.4)
    assert m["dom/d/avg_nll"] == m["avg_nll"] == pytest.approx((0.4 + 0.75 + 0.4) / 3)
    want = (a + b)[:, :12].reshape(3, 4, 3)
    assert torch.equal(acc.reliability, want)


# ----------------------------------------------------------------------------- table and keys
def test_table_width_old_and_new():
    for R in (1, 3):
        assert table_width(R) == 3 + 3 * R and table_width(R, True) == 3 + 5 * R
        assert table_width(R, False, 0) == table_width(R) and table_width(R, True, 0) == table_width(R, True)
        for bins in (1, 15, 64):
            for surface in (False, True):
                assert table_width(R, surface, bins) == table_width(R, surface) + R * (3 * bins + 2)
                assert table_width(R, surface, bins, 1) == table_width(R, surface) + (3 * bins + 2)      # softmax head


def _rows(n, bins, rout, seed=0):
    g = torch.Generator().manual_seed(seed)
    R = len(REGIONS)
    rows = []
    for i in range(n):
        cnt = torch.randint(0, 50, (rout, bins), generator=g).double()
        if i == 1:
            cnt[0] = 0                                     # an invalid (volume, region)
        conf = cnt * (0.5 + 0.5 * torch.rand((rout, bins), generator=g, dtype=torch.float64))
        cor = torch.floor(cnt * torch.rand((rout, bins), generator=g, dtype=torch.float64))
        raw = torch.cat([torch.stack([cnt, conf, cor], -1).reshape(rout, -1),
                         cnt.sum(-1, keepdim=True) * 0.1, cnt.sum(-1, keepdim=True) * 0.3], 1)
        dice = torch.rand(R, generator=g).double()
        rows.append(torch.cat([torch.tensor([i, i % 2, 0.5 + i], dtype=torch.float64), dice, dice / 2,
                               torch.ones(R, dtype=torch.float64), raw.reshape(-1)]))
    return torch.stack(rows)


CAL_KEYS = {f"{p}{r}_{k}" for p in ("", "dom/a/", "dom/b/") for r in ("et", "tc", "wt", "avg") for k in ("ece", "brier", "nll")}


@pytest.mark.parametrize("rout,names", [(3, None), (1, ["all"])])
def test_replay_of_shuffled_and_repeated_rows_equals_the_accumulator(rout, names):
    bins, n = 5, 6
    rows = _rows(n, bins, rout)
    assert rows.shape[1] == table_width(3, False, bins, rout)
    acc = RegionAccumulator(REGIONS, False, bins, names)
    R = len(REGIONS)
    for row in rows:
        acc.add_row(row[3:3 + R].float().tolist(), row[3 + R:3 + 2 * R].float().tolist(), [True] * R, ["a", "b"][int(row[1])],
                    None, None, row[3 + 3 * R:])
        acc.add_loss(float(row[2]), 1)
    want = acc.metrics(True)
    perm = torch.tensor([4, 0, 2, 2, 5, 1, 3, 0])          # shuffled, two volumes twice
    merged = gather_table(rows[perm], len(perm), 1)
    assert torch.equal(merged, rows)
    got = metrics_from_table(merged, REGIONS, ["a", "b"], True, False, bins, names)
    assert got == want
    assert torch.equal(reliability_from_table(merged, bins, rout), acc.reliability)
    assert acc.reliability.shape == (rout, bins, 3) and acc.reliability.dtype == torch.float64
    if names is None:
        assert CAL_KEYS <= set(want)
    else:
        assert {"all_ece", "avg_ece", "all_brier", "avg_nll", "dom/a/all_nll"} <= set(want) and "et_ece" not in want


def test_metric_keys_only_when_enabled():
    rows = _rows(4, 5, 3)
    on = metrics_from_table(rows, REGIONS, ["a", "b"], True, False, 5)
    off = metrics_from_table(rows[:, :table_width(3)], REGIONS, ["a", "b"], True)
    assert set(on) - set(off) == CAL_KEYS
    assert {k: on[k] for k in off} == off                 # the old keys keep their values
    assert not any(k.endswith(("_ece", "_brier", "_nll")) for k in off)
    assert set(RegionAccumulator(REGIONS).metrics(True)) == {"et_dc", "tc_dc", "wt_dc", "avg_dc", "miou", "jc", "loss"}


# ----------------------------------------------------------------------------- the C entry point, no device touched
def _tensor(_lib, n=1, c=3, d=4, h=4, w=4, ptr=0x1000):
    return _lib.Tensor(ptr, n, c, d, h, w, c * d * h * w, d * h * w, h * w, w, 1, _lib.F32, 0)


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every check comes before the first HIP call (the pattern of test_abi.test_argument_validation_without_a_gpu); the
    pointers are made up and never followed."""
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    assert lib.mmtta_abi_version() == 2
    INVALID, UNSUPPORTED = -1, -2
    z, y, out = _tensor(_lib), _tensor(_lib), ctypes.c_void_p(0x2000)
    call = lambda z_, y_, softmax, bins, scope, out_=out: lib.mmtta_calibration_bins(
        ctypes.byref(z_) if z_ is not None else None, ctypes.byref(y_) if y_ is not None else None, softmax, bins, scope, out_,
        None, None)
    assert call(None, y, 0, 15, 0) == INVALID and b"null" in lib.mmtta_last_error()
    assert call(z, None, 0, 15, 0) == INVALID
    assert call(z, y, 0, 15, 0, None) == INVALID
    assert call(_tensor(_lib, ptr=None), y, 0, 15, 0) == INVALID
    assert call(z, _tensor(_lib, ptr=None), 0, 15, 0) == INVALID
    for bins in (0, 65, -3):
        assert call(z, y, 0, bins, 0) == INVALID and b"bins" in lib.mmtta_last_error()
        assert lib.mmtta_calibration_scratch_bytes(ctypes.byref(z), bins) == -1
    assert call(z, y, 0, 15, 2) == INVALID and b"scope" in lib.mmtta_last_error()
    assert call(z, y, 0, 15, -1) == INVALID
    one = _tensor(_lib, c=1)
    assert call(one, one, 1, 15, 0) == INVALID and b"softmax" in lib.mmtta_last_error()
    big = _tensor(_lib, c=17)
    assert call(big, big, 1, 15, 0) == UNSUPPORTED and b"16" in lib.mmtta_last_error()
    huge = _tensor(_lib, c=257)
    assert call(huge, huge, 0, 15, 0) == UNSUPPORTED
    assert lib.mmtta_calibration_scratch_bytes(ctypes.byref(huge), 15) == -1
    for other in (_tensor(_lib, c=2), _tensor(_lib, n=2), _tensor(_lib, d=5), _tensor(_lib, h=5), _tensor(_lib, w=5)):
        assert call(z, other, 0, 15, 0) == INVALID and b"shape" in lib.mmtta_last_error()
    assert lib.mmtta_calibration_scratch_bytes(None, 15) == -1
    assert lib.mmtta_calibration_scratch_bytes(ctypes.byref(z), 15) >= 0
    assert lib.mmtta_calibration_scratch_bytes(ctypes.byref(z), 1) >= 0 and lib.mmtta_calibration_scratch_bytes(ctypes.byref(z), 64) >= 0


def test_binding_knows_the_new_symbols():
    from multimodal_tta_amd import _lib, ops
    assert {"mmtta_calibration_scratch_bytes", "mmtta_calibration_bins"} <= set(_lib.exported_names())
    assert ops.CALIBRATION_SCOPES == {"volume": 0, "union": 1}
