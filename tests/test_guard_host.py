"""The do-no-harm guard (``method.guard``): the host-side half, no GPU needed.

The integer rule (``guard.decide``) against exact rational arithmetic and at every boundary; the config (ranges, refusals,
defaults, the shipped yaml block); the evaluator's block - absent when off, and a hand-built table of three volumes in two
domains whose keys are worked out by hand below; the two C entries (declared, exported, typed, and refusing bad arguments
before anything reaches the device)."""
import ctypes
import glob
import os
import random
import re
from fractions import Fraction

import pytest
import torch

INVALID, UNSUPPORTED = -1, -2
FAKE = 4096          # 16-byte aligned addresses that are never dereferenced: the checks fail first
STEP = 1 << 28
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 1 << 16
BIG = (1 << 31) - 1


def _rule(agree=0.0, grow=0.0, shrink=0.0, m=0, scope="volume"):
    from multimodal_tta_amd.guard import GuardRule
    return GuardRule(int(round(agree * Q)), int(round(grow * Q)), int(round(shrink * Q)), m, scope)


def _fails_exactly(s, a, i, rule):
    """The issue's three clauses in rational arithmetic: thresholds A / Q, G / Q, H / Q."""
    A, G, H, m = Fraction(rule.A, Q), Fraction(rule.G, Q), Fraction(rule.H, Q), rule.m
    if rule.A > 0 and max(s, a) >= max(m, 1) and Fraction(2 * i) < A * (s + a):      # Dice = 2i / (s + a) < A
        return True
    if rule.G > 0 and Fraction(a) > G * max(s, m):
        return True
    return rule.H > 0 and Fraction(s) > H * max(a, m)


# ----------------------------------------------------------------------------- the integer rule
def test_decide_equals_rational_arithmetic_on_random_counts():
    from multimodal_tta_amd.guard import decide
    rng = random.Random(7)
    for _ in range(400):
        rule = _rule(rng.choice([0.0, 0.25, 0.5, 0.9, 1.0]), rng.choice([0.0, 1.0, 1.5, 4.0, 1024.0]),
                     rng.choice([0.0, 1.0, 2.0, 4.0]), rng.choice([0, 1, 64, 5000]), "region")
        top = rng.choice([8, 200, 70000, BIG])
        counts = []
        for _ in range(3):
            s, a = rng.randint(0, top), rng.randint(0, top)
            counts.append((s, a, rng.randint(0, min(s, a))))
        want = [1 if _fails_exactly(s, a, i, rule) else 0 for s, a, i in counts]
        assert decide([counts], rule) == [want], (counts, rule)
        assert decide(torch.tensor([counts], dtype=torch.int64), rule) == [want]


def test_every_boundary_passes_at_equality_and_fails_one_past_it():
    from multimodal_tta_amd.guard import region_fails
    agree = _rule(agree=0.5)
    assert not region_fails(10, 6, 4, agree)          # 2 * 4 / 16 = 0.5: equality passes
    assert region_fails(10, 6, 3, agree) and region_fails(10, 7, 4, agree)
    # min_voxels spares a pair of small masks: max(s, a) must reach max(m, 1)
    small = _rule(agree=0.5, m=11)
    assert not region_fails(10, 6, 0, small) and region_fails(11, 6, 0, small) and region_fails(6, 11, 0, small)
    grow = _rule(grow=4.0)
    assert not region_fails(5, 20, 5, grow) and region_fails(5, 21, 5, grow)
    grow_m = _rule(grow=4.0, m=10)          # against max(s, m) = 10
    assert not region_fails(5, 40, 5, grow_m) and region_fails(5, 41, 5, grow_m)
    assert not region_fails(0, 40, 0, grow_m) and region_fails(0, 41, 0, grow_m)
    shrink = _rule(shrink=4.0)
    assert not region_fails(20, 5, 5, shrink) and region_fails(21, 5, 5, shrink)
    shrink_m = _rule(shrink=4.0, m=10)
    assert not region_fails(40, 0, 0, shrink_m) and region_fails(41, 0, 0, shrink_m)
    # a fractional threshold, exactly representable in Q: 1.5
    assert not region_fails(2, 3, 2, _rule(grow=1.5)) and region_fails(2, 4, 2, _rule(grow=1.5))


def test_the_extremes_do_not_overflow_and_empty_masks_pass():
    from multimodal_tta_amd.guard import decide, region_fails
    top = _rule(agree=1.0, grow=1024.0, shrink=1024.0, m=0)
    assert top.A == Q and top.G == 1024 * Q
    assert not region_fails(BIG, BIG, BIG, top)              # identical masks of 2^31 - 1 voxels: Dice 1 = A
    assert region_fails(BIG, BIG, BIG - 1, top)              # one voxel apart under A = Q
    assert (BIG * 1024 * Q) < (1 << 64) and (2 * BIG * Q) < (1 << 64) and (Q * 2 * BIG) < (1 << 64)      # the kernel's products
    assert not region_fails((BIG // 1024), (BIG // 1024) * 1024, (BIG // 1024), _rule(grow=1024.0))
    assert region_fails((BIG // 1024), (BIG // 1024) * 1024 + 1, (BIG // 1024), _rule(grow=1024.0))
    assert region_fails(0, 1, 0, _rule(grow=1024.0)) and region_fails(1, 0, 0, _rule(shrink=1024.0))      # max(s, m) = 0
    for rule in (top, _rule(agree=1.0), _rule(grow=1.0), _rule(shrink=1.0), _rule(0.5, 4.0, 4.0, 64)):
        assert not region_fails(0, 0, 0, rule)               # s = a = 0: nothing to compare
    assert decide([[(0, 0, 0), (BIG, BIG, BIG)]], top) == [[0, 0]]


def test_each_clause_alone_and_the_monitor():
    from multimodal_tta_amd.guard import region_fails
    collapsed, exploded, moved = (100, 10, 10), (10, 100, 10), (50, 50, 10)
    only_agree, only_grow, only_shrink = _rule(agree=0.5), _rule(grow=4.0), _rule(shrink=4.0)
    assert region_fails(*moved, only_agree) and not region_fails(*moved, only_grow) and not region_fails(*moved, only_shrink)
    assert region_fails(*exploded, only_grow) and not region_fails(*exploded, only_shrink)
    assert region_fails(*collapsed, only_shrink) and not region_fails(*collapsed, only_grow)
    monitor = _rule()
    assert monitor.monitors_only and not only_agree.monitors_only
    for c in (collapsed, exploded, moved, (0, BIG, 0), (BIG, 0, 0)):
        assert not region_fails(*c, monitor)


def test_scope_volume_returns_every_channel_and_region_the_failing_one():
    from multimodal_tta_amd.guard import decide
    counts = [[(50, 50, 50), (50, 50, 10), (7, 7, 7)], [(5, 5, 5), (6, 6, 6), (0, 0, 0)], [(1, 100, 1), (3, 3, 3), (4, 4, 4)]]
    assert decide(counts, _rule(0.5, 4.0, 4.0, 0, "region")) == [[0, 1, 0], [0, 0, 0], [1, 0, 0]]
    assert decide(counts, _rule(0.5, 4.0, 4.0, 0, "volume")) == [[1, 1, 1], [0, 0, 0], [1, 1, 1]]


def test_rule_fields_outside_their_ranges_are_refused():
    from multimodal_tta_amd.guard import GuardRule
    for kw, key in ((dict(A=Q + 1), "A"), (dict(A=-1), "A"), (dict(G=Q - 1), "G"), (dict(G=1024 * Q + 1), "G"), (dict(H=1), "H"),
                    (dict(m=-1), "m"), (dict(m=1 << 31), "m"), (dict(scope="item"), "scope"), (dict(A=0.5), "A")):
        with pytest.raises(ValueError, match=rf"GuardRule\.{key}\b"):
            GuardRule(**kw)
    s = GuardRule(Q // 2, 4 * Q, 0, 64, "region").struct()
    assert (s.min_agreement_q16, s.max_growth_q16, s.max_shrink_q16, s.min_voxels, s.scope) == (Q // 2, 4 * Q, 0, 64, 1)


# ----------------------------------------------------------------------------- the config
def _cfg(*extra, method="tta_entmin"):
    from multimodal_tta_amd.config import compose
    return compose(overrides=["task=brats", "model=unet", f"method={method}", *extra])


def test_shipped_block_is_there_and_disabled():
    from multimodal_tta_amd.guard import DEFAULTS, parse_guard
    files = sorted(glob.glob(os.path.join(ROOT, "configs", "method", "tta_*.yaml")))
    assert len(files) >= 15
    for path in files:
        name = os.path.basename(path)[:-5]
        cfg = _cfg(method=name)
        assert cfg["method"]["guard"] == DEFAULTS, name
        spec = parse_guard(cfg)
        assert spec.enable is False and (spec.rule.A, spec.rule.G, spec.rule.H, spec.rule.m, spec.rule.scope) == \
            (Q // 2, 4 * Q, 4 * Q, 64, "volume")
    on = parse_guard(_cfg("method.guard.enable=true", "method.guard.scope=region", "method.guard.max_growth=0"))
    assert on.enable and on.rule.scope == "region" and on.rule.G == 0
    assert parse_guard({}).enable is False          # no block at all: off, with the same numbers
    assert parse_guard({}).rule == parse_guard(_cfg()).rule


def test_threshold_defaults_to_the_evaluators():
    from multimodal_tta_amd.guard import parse_guard
    assert parse_guard({}).threshold == 0.5
    assert parse_guard(_cfg("evaluation.seg.threshold=0.3")).threshold == pytest.approx(0.3, abs=0)
    assert parse_guard(_cfg("evaluation.seg.threshold=0.3", "method.guard.threshold=0.7")).threshold == 0.7


@pytest.mark.parametrize("key,value", [("enable", 1), ("enable", "yes"), ("min_agreement", -0.1), ("min_agreement", 1.5),
                                       ("min_agreement", True), ("min_agreement", float("nan")), ("max_growth", 0.5),
                                       ("max_growth", 1025), ("max_growth", -1), ("max_growth", float("inf")), ("max_shrink", 0.99),
                                       ("max_shrink", 2000.0), ("max_shrink", "4"), ("min_voxels", -1), ("min_voxels", 1 << 31),
                                       ("min_voxels", 2.5), ("min_voxels", True), ("scope", "item"), ("scope", 0),
                                       ("threshold", 0.0), ("threshold", 1.0), ("threshold", -3), ("threshold", float("nan"))])
def test_every_out_of_range_value_raises_and_names_its_key(key, value):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["method"]["guard"] = dict(dict(cfg["method"]["guard"], enable=True), **{key: value})
    with pytest.raises(ValueError, match=rf"method\.guard\.{key}\b"):
        get_plugin("entmin_tta")(cfg)
    cfg["method"]["guard"]["enable"] = False if key != "enable" else value
    with pytest.raises(ValueError, match=rf"method\.guard\.{key}\b"):          # a disabled block is validated all the same
        get_plugin("entmin_tta")(cfg)


def test_non_episodic_runs_and_region_scope_on_a_softmax_head_are_refused():
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg("method.guard.enable=true", "method.episodic=false")
    with pytest.raises(ValueError, match=r"method\.guard\.enable.*method\.episodic"):
        get_plugin("entmin_tta")(cfg)
    for name in ("tta_cotta", "tta_petal"):
        cfg = _cfg("method.guard.enable=true", "method.episodic=false", method=name)
        with pytest.raises(ValueError, match=r"method\.guard\.enable.*method\.episodic"):
            get_plugin(cfg["method"]["name"])(cfg)
    get_plugin("entmin_tta")(_cfg("method.episodic=false"))          # the guard off: as before
    cfg = _cfg("method.guard.enable=true", "method.guard.scope=region")
    cfg["training"]["criterion"]["softmax"] = True
    with pytest.raises(ValueError, match=r"method\.guard\.scope.*training\.criterion\.softmax"):
        get_plugin("entmin_tta")(cfg)
    cfg["method"]["guard"]["scope"] = "volume"
    assert get_plugin("entmin_tta")(cfg).guard.enable
    cfg["method"]["guard"].update(scope="region", enable=False)
    assert not get_plugin("entmin_tta")(cfg).guard.enable


def test_every_registered_plugin_reads_the_block():
    from multimodal_tta_amd.registry import get_plugin
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "method", "tta_*.yaml"))):
        extra = ["method.window.roi=[32,32,32]"] if path.endswith("tta_window.yaml") else []
        cfg = _cfg("method.guard.enable=true", "method.guard.min_voxels=7", *extra, method=os.path.basename(path)[:-5])
        if cfg["method"].get("episodic", True) is False:
            cfg["method"]["episodic"] = True
        plug = get_plugin(cfg["method"]["name"])(cfg)
        assert plug.guard.enable and plug.guard.rule.m == 7, path


# ----------------------------------------------------------------------------- the evaluator's block
R2 = ["ET", "WT"]
DOMAINS = ["siteA", "siteB"]
TODAY_KEYS = ["et_dc", "wt_dc", "avg_dc", "miou", "jc", "loss", "dom/siteA/et_dc", "dom/siteA/wt_dc", "dom/siteA/avg_dc",
              "dom/siteA/miou", "dom/siteB/et_dc", "dom/siteB/wt_dc", "dom/siteB/avg_dc", "dom/siteB/miou"]


def _row(index, dom, dice, valid, guard=None, iou=(0.5, 0.5)):
    head = [float(index), float(dom), 0.0, *dice, *iou, *[1.0 if v else 0.0 for v in valid]]
    return torch.tensor(head + (list(guard) if guard is not None else []), dtype=torch.float64)


def test_off_means_absent():
    from multimodal_tta_amd.evaluation import (ADD_ROW_POSITIONAL, BLOCKS, RegionAccumulator, SegmentationEvaluationStrategy,
                                               metrics_from_table, table_layout, table_width)
    assert [b.name for b in BLOCKS][-2:] == ["guard", "calibration"]
    for R in (1, 2, 3):
        assert table_width(R) == table_width(R, guard=False) == 3 + 3 * R
        assert table_width(R, surface=True, bins=10, components=True) == 3 + 3 * R + 2 * R + 3 * R + R * 32
        assert table_width(R, guard=True) == table_width(R) + 5 * R
        lay = table_layout(R, bins=10, guard=True)          # the guard's columns, then the calibration at the row's end
        assert lay.slices["guard"] == slice(3 + 3 * R, 3 + 8 * R) and lay.slices["calibration"] == slice(3 + 8 * R, lay.width)
    table = torch.stack([_row(0, 0, (0.5, 0.75), (1, 1)), _row(1, 1, (1.0, 0.25), (1, 0))])
    off = metrics_from_table(table, R2, DOMAINS, False)
    assert list(off) == TODAY_KEYS and off == metrics_from_table(table, R2, DOMAINS, False, guard=False)
    assert not any("guard" in k or "src_dc" in k or "harmed" in k or "dc_gain" in k for k in off)
    assert "guard" not in ADD_ROW_POSITIONAL and len(ADD_ROW_POSITIONAL) == 7
    acc = RegionAccumulator(R2, guard=True)
    with pytest.raises(TypeError, match="by position"):          # a new block is passed by name only
        acc.add_row([0.5, 0.5], [0.5, 0.5], [True, True], "siteA", None, None, *([None] * 7), [0.0] * 10)
    with pytest.raises(TypeError, match="no such block"):
        RegionAccumulator(R2).add_row([0.5, 0.5], [0.5, 0.5], [True, True], "siteA", guardian=[0.0] * 10)
    strat = SegmentationEvaluationStrategy({})
    assert strat.enable_guard is False and strat.switches()["guard"] is False and strat._table_width() == 12


def test_seg_tta_eval_switches_the_block_on_with_the_method():
    from multimodal_tta_amd.evaluation import TTASegmentationEvaluationStrategy
    assert TTASegmentationEvaluationStrategy(_cfg()).enable_guard is False
    on = TTASegmentationEvaluationStrategy(_cfg("method.guard.enable=true"))
    assert on.enable_guard is True and list(on.layout().slices) == ["guard"] and on._table_width() == 12 + 15
    both = TTASegmentationEvaluationStrategy(_cfg("method.guard.enable=true", "evaluation.calibration.enable=true"))
    assert list(both.layout().slices) == ["guard", "calibration"]


def test_guard_columns_form_the_source_dice_as_dice_is_formed():
    from multimodal_tta_amd.evaluation import dice_iou_from_counts, guard_columns
    raw = torch.tensor([[1, 10, 6, 4, 3, 10, 7], [0, 0, 0, 0, 0, 0, 0], [0, 5, 9, 5, 2, 5, 9]], dtype=torch.int64)
    cols = guard_columns(raw).reshape(5, 3)
    assert cols.dtype == torch.float64
    assert cols[0].tolist() == [1, 0, 0] and cols[1].tolist() == [8, 0, 4]
    assert cols[2].tolist() == [8, 0, 10] and cols[3].tolist() == [16, 0, 14]
    want = dice_iou_from_counts(raw[:, 4:7])[0]
    assert want.dtype == torch.float32 and torch.equal(cols[4], want.double())


def test_hand_built_table_of_three_volumes_in_two_domains():
    """Columns per region: fallback, flips, 2i, s + a, source Dice.  Every number is a short binary fraction, so the sums are
    exact and the expected values are written as the quotients they are.
      vol 0 (A)  dice .5 .75   valid 1 1   ET s,a,i = 10,6,4 fell back, src .25     WT 0,0,0 (no agreement), src .75
      vol 1 (A)  dice .5 .5    valid 0 1   ET 4,4,4, src .9 (ground truth empty)    WT 8,8,6, src .75
      vol 2 (B)  dice 1. .25   valid 1 1   ET 2,6,2 fell back, src .5               WT 4,4,2 fell back, src .5"""
    from multimodal_tta_amd.evaluation import metrics_from_table
    table = torch.stack([
        _row(0, 0, (0.5, 0.75), (1, 1), [1, 0, 8, 0, 8, 0, 16, 0, 0.25, 0.75]),
        _row(1, 0, (0.5, 0.5), (0, 1), [0, 0, 0, 4, 8, 12, 8, 16, 0.9, 0.75]),
        _row(2, 1, (1.0, 0.25), (1, 1), [1, 1, 4, 4, 4, 4, 8, 8, 0.5, 0.5])])
    got = metrics_from_table(table, R2, DOMAINS, False, guard=True)
    want = {
        "et_guard_fallback": 2.0 / 3.0, "wt_guard_fallback": 1.0 / 3.0, "avg_guard_fallback": (2.0 / 3.0 + 1.0 / 3.0) / 2,
        "et_guard_agreement": 2.0 / 3.0, "wt_guard_agreement": 0.625,          # (.5 + 1 + .5) / 3; (.75 + .5) / 2
        "et_guard_flips": 4.0, "wt_guard_flips": 8.0 / 3.0,
        "et_src_dc": 0.375, "wt_src_dc": 2.0 / 3.0, "avg_src_dc": (0.375 + 2.0 / 3.0) / 2,
        "et_dc_gain": 0.375, "wt_dc_gain": -0.5 / 3.0,                         # (.25 + .5) / 2; (0 - .25 - .25) / 3
        "et_harmed": 0.0, "wt_harmed": 2.0 / 3.0,
        "dom/siteA/et_guard_fallback": 0.5, "dom/siteA/wt_guard_fallback": 0.0, "dom/siteA/avg_guard_fallback": 0.25,
        "dom/siteA/et_guard_agreement": 0.75, "dom/siteA/wt_guard_agreement": 0.75,
        "dom/siteA/et_guard_flips": 4.0, "dom/siteA/wt_guard_flips": 2.0,
        "dom/siteA/et_src_dc": 0.25, "dom/siteA/wt_src_dc": 0.75, "dom/siteA/avg_src_dc": 0.5,
        "dom/siteA/et_dc_gain": 0.25, "dom/siteA/wt_dc_gain": -0.125,
        "dom/siteA/et_harmed": 0.0, "dom/siteA/wt_harmed": 0.5,
        "dom/siteB/et_guard_fallback": 1.0, "dom/siteB/wt_guard_fallback": 1.0, "dom/siteB/avg_guard_fallback": 1.0,
        "dom/siteB/et_guard_agreement": 0.5, "dom/siteB/wt_guard_agreement": 0.5,
        "dom/siteB/et_guard_flips": 4.0, "dom/siteB/wt_guard_flips": 4.0,
        "dom/siteB/et_src_dc": 0.5, "dom/siteB/wt_src_dc": 0.5, "dom/siteB/avg_src_dc": 0.5,
        "dom/siteB/et_dc_gain": 0.5, "dom/siteB/wt_dc_gain": -0.25,
        "dom/siteB/et_harmed": 0.0, "dom/siteB/wt_harmed": 1.0,
    }
    new = {k: v for k, v in got.items() if k not in TODAY_KEYS}
    assert set(new) == set(want)
    for k, v in want.items():
        assert new[k] == pytest.approx(v, rel=0, abs=1e-15), (k, new[k], v)
    off = metrics_from_table(table[:, :9], R2, DOMAINS, False)
    assert {k: got[k] for k in TODAY_KEYS} == off          # every existing key describes the returned prediction, as before
    assert off["et_dc"] == 0.75 and off["wt_dc"] == 0.5


# ----------------------------------------------------------------------------- the entry points
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def test_the_symbols_are_declared_exported_and_typed():
    _l, lib = _lib()
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_l.LIB_PATH)
    for name, nargs in (("mmtta_guard_counts", 5), ("mmtta_guard_select", 6)):
        assert re.search(rf"\bint\s+{name}\s*\(", code), f"include/mmtta.h does not declare {name}"
        assert name in _l.exported_names()
        assert getattr(raw, name) is not None          # AttributeError: not exported
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    assert "typedef struct mmtta_guard_rule" in code and ctypes.sizeof(_l.GuardRule) == 24
    assert lib.mmtta_abi_version() == 2          # additive: the version stays
    assert "guard.hip" in __import__("multimodal_tta_amd.build", fromlist=["SOURCES"]).SOURCES


def _tensor(_l, slot=0, n=2, c=3, d=4, h=5, w=6, ptr=True, dtype=None, ldc=4, sc=1):
    return _l.Tensor((FAKE + slot * STEP) if ptr is True else ptr, n, c, d, h, w, d * h * w * ldc, sc, h * w * ldc, w * ldc, ldc,
                     _l.F32 if dtype is None else dtype, _l.TENSOR_OWNS_PAD)


def test_the_entries_refuse_bad_arguments_before_anything_is_launched():
    """Every pointer below is fake: a call that got as far as a memset or a launch would fault, not return a status."""
    _l, lib = _lib()
    ref, ada = _tensor(_l, 0), _tensor(_l, 1)
    out = FAKE + 4 * STEP

    def counts(r=ref, a=ada, thr=0.5, c=out):
        return lib.mmtta_guard_counts(ctypes.byref(r) if r is not None else None, ctypes.byref(a) if a is not None else None, thr, c, None)

    def message():
        return lib.mmtta_last_error().decode()

    assert counts(r=None) == INVALID and "reference" in message()
    assert counts(a=None) == INVALID and "adapted" in message()
    assert counts(c=None) == INVALID and "counts" in message()
    assert counts(r=_tensor(_l, 0, ptr=None)) == INVALID
    assert counts(a=_tensor(_l, 1, w=7)) == INVALID and "shape mismatch" in message()
    assert counts(a=_tensor(_l, 1, c=2)) == INVALID and "shape mismatch" in message()
    assert counts(a=_tensor(_l, 1, ldc=8)) == INVALID and "row width" in message()
    for thr in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert counts(thr=thr) == INVALID and "threshold" in message()
    assert counts(r=_tensor(_l, 0, dtype=_l.BF16), a=_tensor(_l, 1, dtype=_l.BF16)) == UNSUPPORTED
    assert counts(r=_tensor(_l, 0, sc=120), a=_tensor(_l, 1, sc=120)) == UNSUPPORTED and "channels-last" in message()
    assert counts(r=_tensor(_l, 0, c=17, ldc=20), a=_tensor(_l, 1, c=17, ldc=20)) == UNSUPPORTED
    big = dict(d=2048, h=1024, w=1024)          # 2^31 voxels
    assert counts(r=_tensor(_l, 0, **big), a=_tensor(_l, 1, **big)) == UNSUPPORTED and "2^31" in message()

    def select(rule=None, c=out, r=ref, lg=ada, fb=out + STEP, **fields):
        rs = _l.GuardRule(Q // 2, 4 * Q, 4 * Q, 64, 0, 0) if rule is None else rule
        for k, v in fields.items():
            setattr(rs, k, v)
        return lib.mmtta_guard_select(c, ctypes.byref(rs), ctypes.byref(r) if r is not None else None,
                                      ctypes.byref(lg) if lg is not None else None, fb, None)

    assert select(c=None) == INVALID and "counts" in message()
    assert select(fb=None) == INVALID and "fallback" in message()
    assert select(r=None) == INVALID and select(lg=None) == INVALID
    assert lib.mmtta_guard_select(out, None, ctypes.byref(ref), ctypes.byref(ada), out + STEP, None) == INVALID and "rule" in message()
    assert select(lg=ref) == INVALID and "aliased" in message()
    assert select(lg=_tensor(_l, 0, ptr=FAKE + 64)) == INVALID and "aliased" in message()          # overlapping, not identical
    assert select(lg=_tensor(_l, 1, h=6)) == INVALID and "shape mismatch" in message()
    assert select(lg=_tensor(_l, 1, ldc=8)) == INVALID and "row width" in message()
    assert select(min_agreement_q16=Q + 1) == INVALID and "min_agreement_q16" in message()
    assert select(max_growth_q16=Q - 1) == INVALID and "max_growth_q16" in message()
    assert select(max_growth_q16=1024 * Q + 1) == INVALID and "max_growth_q16" in message()
    assert select(max_shrink_q16=1) == INVALID and "max_shrink_q16" in message()
    assert select(min_voxels=-1) == INVALID and "min_voxels" in message()
    assert select(scope=2) == INVALID and "scope" in message()
    assert select(r=_tensor(_l, 0, **big), lg=_tensor(_l, 1, **big)) == UNSUPPORTED
    assert select(r=_tensor(_l, 0, dtype=_l.BF16), lg=_tensor(_l, 1, dtype=_l.BF16)) == UNSUPPORTED
