"""Normalised surface Dice, everything that needs no GPU: the two config blocks, the window-radius loop, the scores formed from
the device's integer counts, the widened per-volume table and its replay, the key names and the argument checks of the two C
entry points."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from multimodal_tta_amd import ops
from multimodal_tta_amd.evaluation import (RegionAccumulator, SegmentationEvaluationStrategy, lesionwise_columns,
                                           lesionwise_nsd_columns, lesionwise_nsd_config, metrics_from_table, nsd_suffix,
                                           surface_dice_columns, surface_dice_config, table_width)

Q30 = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(sd=None, nsd=None, lw=None, spacing=None, softmax=False):
    cfg = {"evaluation": {}}
    if sd is not None:
        cfg["evaluation"]["surface_dice"] = dict(sd)
    if lw is not None or nsd is not None:
        cfg["evaluation"]["lesionwise"] = dict(lw if lw is not None else {"enable": True})
        if nsd is not None:
            cfg["evaluation"]["lesionwise"]["nsd"] = dict(nsd)
    if spacing is not None:
        cfg["evaluation"]["seg"] = {"spacing": list(spacing)}
    if softmax:
        cfg["training"] = {"criterion": {"softmax": True}}
    return cfg


# ----------------------------------------------------------------------------- config
def test_config_defaults_and_values():
    assert surface_dice_config({}) == (False, [1.0])
    assert lesionwise_nsd_config({}) == (False, [0.5, 1.0])
    assert surface_dice_config(_cfg(sd={"enable": True, "tolerances": [0.5, 2]})) == (True, [0.5, 2.0])
    assert lesionwise_nsd_config(_cfg(nsd={"enable": True})) == (True, [0.5, 1.0])
    assert lesionwise_nsd_config(_cfg(nsd={"tolerances": [0, 3.0]}, lw={"enable": False})) == (False, [0.0, 3.0])
    off = SegmentationEvaluationStrategy({})
    assert not off.enable_surface_dice and not off.enable_lesionwise_nsd
    assert off.sd_tolerances == [] and off.ln_tolerances == [] and off._table_width() == table_width(3)
    on = SegmentationEvaluationStrategy(_cfg(sd={"enable": True}, nsd={"enable": True}))
    assert on.enable_surface_dice and on.enable_lesionwise_nsd and on.enable_lesionwise
    assert on.sd_tolerances == [1.0] and on.ln_tolerances == [0.5, 1.0]
    assert on._table_width() == table_width(3, lesionwise=True, surface_dice=1, lesionwise_nsd=2) == table_width(3) + 7 * 3 + 9


BAD = [(dict(enable="on"), "enable"), (dict(enable=1), "enable"), (dict(tolerances=[]), "tolerances"),
       (dict(tolerances=[0.5, 1, 2, 3, 4]), "tolerances"), (dict(tolerances=1.0), "tolerances"),
       (dict(tolerances=[-0.5]), "tolerances"), (dict(tolerances=[float("inf")]), "tolerances"),
       (dict(tolerances=[float("nan")]), "tolerances"), (dict(tolerances=["1"]), "tolerances"),
       (dict(tolerances=[True]), "tolerances"), (dict(tolerances=[1.0, 1]), "tolerances")]


@pytest.mark.parametrize("block,leaf", BAD)
@pytest.mark.parametrize("enabled", [True, False])
def test_config_bad_values_name_their_key(block, leaf, enabled):
    block = dict(block)
    block.setdefault("enable", enabled)
    for key, cfg, fn in (("evaluation.surface_dice", _cfg(sd=block), surface_dice_config),
                         ("evaluation.lesionwise.nsd", _cfg(nsd=block), lesionwise_nsd_config)):
        pat = (key + "." + leaf).replace(".", r"\.") + r"\b"
        with pytest.raises(ValueError, match=pat):
            fn(cfg)
        with pytest.raises(ValueError, match=pat):
            SegmentationEvaluationStrategy(cfg)


def test_config_window_limit_points_at_the_surface_block():
    """The window cap depends on the spacing and belongs to an ENABLED block: a disabled one keeps whatever well-formed
    tolerances it holds."""
    assert surface_dice_config(_cfg(sd={"enable": True, "tolerances": [8.0]})) == (True, [8.0])
    assert surface_dice_config(_cfg(sd={"enable": True, "tolerances": [12.0]}, spacing=[2.0, 1.5, 1.5])) == (True, [12.0])
    for sd, nsd, spacing, fn, key in (({"tolerances": [1.0, 6.8]}, None, [2.0, 1.0, 0.75], surface_dice_config, "evaluation.surface_dice"),
                                      ({"tolerances": [9.0]}, None, None, surface_dice_config, "evaluation.surface_dice"),
                                      (None, {"tolerances": [9.0]}, None, lesionwise_nsd_config, "evaluation.lesionwise.nsd")):
        block = dict(sd if sd is not None else nsd)
        for enable in (True, False):
            block["enable"] = enable
            cfg = _cfg(sd=block if sd is not None else None, nsd=block if nsd is not None else None, spacing=spacing)
            if not enable:
                assert fn(cfg) == (False, [float(v) for v in block["tolerances"]])
                SegmentationEvaluationStrategy(cfg)
                continue
            for build in (fn, SegmentationEvaluationStrategy):
                with pytest.raises(ValueError, match=re.escape(key) + r"\.tolerances.*evaluation\.surface \(HD95 / ASD\)"):
                    build(cfg)


def test_lesionwise_nsd_needs_the_lesionwise_block_and_the_sigmoid_head():
    with pytest.raises(ValueError, match=r"evaluation\.lesionwise\.nsd\.enable needs evaluation\.lesionwise\.enable"):
        lesionwise_nsd_config(_cfg(nsd={"enable": True}, lw={"enable": False}))
    with pytest.raises(ValueError, match=r"evaluation\.lesionwise\.nsd\.enable"):
        lesionwise_nsd_config({"evaluation": {"lesionwise": {"nsd": {"enable": True}}}})
    with pytest.raises(NotImplementedError, match=r"evaluation\.surface_dice\.enable"):
        SegmentationEvaluationStrategy(_cfg(sd={"enable": True}, softmax=True))
    SegmentationEvaluationStrategy(_cfg(sd={"enable": False}, softmax=True))


def test_key_names_use_percent_g():
    assert [nsd_suffix(t) for t in (0, 0.5, 1.0, 2, 1.25, 0.1)] == ["0", "0.5", "1", "2", "1.25", "0.1"]
    acc = RegionAccumulator(["ET", "WT"], lesionwise=True, surface_dice=[0.5, 1.0], lesionwise_nsd=[1.0])
    st = torch.tensor([[1, 1, 1, 1, 1, Q30, 0], [1, 1, 1, 1, 1, Q30, 0]])
    acc.add_row([1.0, 1.0], [1.0, 1.0], [True, True], "d", lesionwise=lesionwise_columns(st),
                surface_dice=torch.tensor([0.25, 0.5, 0.75, 1.0]), lesionwise_nsd=torch.tensor([0.5, 0.125]))
    m = acc.metrics(False)
    new = {k for k in m if "nsd" in k}
    base = {"et_nsd_0.5", "wt_nsd_0.5", "avg_nsd_0.5", "et_nsd_1", "wt_nsd_1", "avg_nsd_1", "et_lw_nsd_1", "wt_lw_nsd_1", "avg_lw_nsd_1"}
    assert new == base | {"dom/d/" + k for k in base}
    assert (m["et_nsd_0.5"], m["wt_nsd_0.5"], m["et_nsd_1"], m["wt_nsd_1"]) == (0.25, 0.5, 0.75, 1.0)
    assert m["avg_nsd_1"] == 0.875 and m["et_lw_nsd_1"] == 0.5 and m["dom/d/wt_lw_nsd_1"] == 0.125
    plain = RegionAccumulator(["ET", "WT"], lesionwise=True)
    plain.add_row([1.0, 1.0], [1.0, 1.0], [True, True], "d", lesionwise=lesionwise_columns(st))
    assert set(plain.metrics(False)) == set(m) - new and all(m[k] == v for k, v in plain.metrics(False).items())


# ----------------------------------------------------------------------------- the window radius
@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (2.0, 1.0, 0.75), (1.5, 0.8, 2.0), (0.3, 0.3, 3.0), (1.0, 1.0 / 3.0, 0.7)])
def test_window_radius_against_brute_force(spacing):
    f32 = np.float32
    for tau in (0.0, 0.2, 0.5, 0.75, 1.0, 1.5, 2.0, 2.4, 3.0, float(f32(1.0 / 3.0)), float(np.nextafter(f32(1.5), f32(0)))):
        rad = ops.surface_dice_radius(spacing, tau)
        want = []
        for s in spacing:
            ok = [k for k in range(0, 12) if f32(np.sqrt(np.float64(k * s) * np.float64(k * s))) <= f32(tau)]
            want.append(min(max(ok), ops.SURFACE_DICE_MAX_RADIUS + 1))      # k = 0 always qualifies
        assert list(rad) == want, (spacing, tau, rad, want)
        if max(rad) > ops.SURFACE_DICE_MAX_RADIUS:
            continue
        # the window holds every offset that can be a hit: one step outside it on any axis is beyond tau
        for off in itertools.product(range(-rad[0] - 1, rad[0] + 2), range(-rad[1] - 1, rad[1] + 2), range(-rad[2] - 1, rad[2] + 2)):
            d2 = math.fma(off[0] * spacing[0], off[0] * spacing[0], math.fma(off[1] * spacing[1], off[1] * spacing[1],
                          (off[2] * spacing[2]) ** 2)) if hasattr(math, "fma") else sum((o * s) ** 2 for o, s in zip(off, spacing))
            if any(abs(o) > r for o, r in zip(off, rad)):
                assert not f32(np.sqrt(d2)) <= f32(tau), (spacing, tau, off)


# ----------------------------------------------------------------------------- counts -> scores
def test_surface_dice_columns_and_validity():
    # [R=3, T=2, 4]: a plain case, an empty prediction against a ground truth (scores 0), both empty (0, and invalid via Dice)
    counts = torch.tensor([[[3, 10, 5, 6], [10, 10, 6, 6]], [[0, 0, 0, 7], [0, 0, 0, 7]], [[0, 0, 0, 0], [0, 0, 0, 0]]])
    c = surface_dice_columns(counts).reshape(2, 3)
    assert c.dtype == torch.float64 and c.tolist() == [[0.5, 0.0, 0.0], [1.0, 0.0, 0.0]]
    big = surface_dice_columns(torch.tensor([[[2 ** 29, 2 ** 30, 2 ** 29 + 1, 2 ** 30]]]))
    assert big.tolist() == [(2 ** 30 + 1) / 2 ** 31]
    acc = RegionAccumulator(["A", "B", "C"], surface_dice=[0.5, 2.0])
    acc.add_row([0.5, 0.0, 0.0], [0.4, 0.0, 0.0], [True, True, False], "d0", surface_dice=surface_dice_columns(counts))
    acc.add_row([0.5, 0.0, 0.0], [0.4, 0.0, 0.0], [True, False, False], "d1", surface_dice=torch.tensor([1.0, 9.0, 9.0, 0.0, 9.0, 9.0]))
    m = acc.metrics(False)
    assert m["a_nsd_0.5"] == 0.75 and m["a_nsd_2"] == 0.5
    assert m["b_nsd_0.5"] == 0.0 and m["b_nsd_2"] == 0.0          # one valid volume, all misses
    assert m["c_nsd_0.5"] == 0.0 and m["avg_nsd_0.5"] == 0.375     # C never valid: out of the mean over regions
    assert m["dom/d0/a_nsd_0.5"] == 0.5 and m["dom/d1/a_nsd_0.5"] == 1.0 and m["dom/d1/avg_nsd_2"] == 0.0


def test_lesionwise_nsd_columns_and_validity():
    # columns of stats: lesions, kept, found, components, matched, dice_q, fp voxels
    stats = torch.tensor([[2, 2, 1, 3, 1, Q30 // 2, 9],      # kept 2, fp 2 -> den 4
                          [0, 0, 0, 2, 0, 0, 5],             # GT-empty with false positives: counts, with 0
                          [0, 0, 0, 0, 0, 0, 0],             # nothing to find, nothing predicted: undefined
                          [3, 1, 0, 0, 0, 0, 0]])            # one kept lesion, missed: 0
    nsd = torch.tensor([[Q30, 3 * Q30 // 2], [0, 0], [0, 0], [0, 0]])
    c = lesionwise_nsd_columns(stats, nsd).reshape(2, 4)
    assert c.tolist() == [[0.25, 0.0, 0.0, 0.0], [0.375, 0.0, 0.0, 0.0]]
    q = 4000 * Q30 - 1      # beyond 2^41: formed from the integers, not carried through a float sum
    assert lesionwise_nsd_columns(torch.tensor([[4000, 4000, 4000, 4000, 4000, 0, 0]]), torch.tensor([[q]])).tolist() == [q / Q30 / 4000]
    acc = RegionAccumulator(["A", "B", "C", "D"], lesionwise=True, lesionwise_nsd=[0.5, 1.0])
    acc.add_row([0.0] * 4, [0.0] * 4, [True] * 4, "d", lesionwise=lesionwise_columns(stats), lesionwise_nsd=c.reshape(-1))
    m = acc.metrics(False)
    assert (m["a_lw_nsd_0.5"], m["a_lw_nsd_1"], m["b_lw_nsd_1"], m["c_lw_nsd_1"], m["d_lw_nsd_1"]) == (0.25, 0.375, 0.0, 0.0, 0.0)
    assert m["avg_lw_nsd_1"] == 0.375 / 3 and m["avg_lw_nsd_0.5"] == 0.25 / 3      # C is undefined: out of the mean over regions


@pytest.mark.parametrize("surface,bins,hd95", [(False, 0, False), (True, 4, True)])
def test_table_replay_equals_the_accumulator(surface, bins, hd95):
    from multimodal_tta_amd.evaluation import lesionwise_hd95_columns
    regions, sd_t, ln_t = ["ET", "WT"], [0.5, 1.0, 2.0], [1.0]
    rng = np.random.default_rng(5)
    acc = RegionAccumulator(regions, surface, bins, None, False, True, False, hd95, sd_t, ln_t)
    rows = []
    for i in range(5):
        dice, iou = rng.random(2).astype(np.float32), rng.random(2).astype(np.float32)
        valid = [bool(i % 2), True]
        st = torch.tensor(rng.integers(0, 4, (2, 7)))
        st[:, 2] = torch.minimum(st[:, 2], st[:, 1]); st[:, 4] = torch.minimum(st[:, 4], st[:, 3])
        lw = lesionwise_columns(st)
        lh = lesionwise_hd95_columns(st, torch.tensor([[5 << 20, 1, 0], [0, 0, 0]]), 100.0) if hd95 else None
        sd = surface_dice_columns(torch.tensor(rng.integers(0, 50, (2, 3, 4))))
        ln = lesionwise_nsd_columns(st, torch.tensor(rng.integers(0, Q30, (2, 1))))
        hdv, asd = (rng.random(2).astype(np.float32), rng.random(2).astype(np.float32)) if surface else (None, None)
        cal = torch.tensor(rng.random(2 * (3 * bins + 2))) if bins else None
        acc.add_row(dice.tolist(), iou.tolist(), valid, f"d{i % 2}", hdv.tolist() if surface else None,
                    asd.tolist() if surface else None, cal, None, lw, None, lh, sd, ln)
        parts = [torch.tensor([i, i % 2, 0.0], dtype=torch.float64), torch.tensor(dice).double(), torch.tensor(iou).double(),
                 torch.tensor(valid).double()]
        if surface:
            parts += [torch.tensor(hdv).double(), torch.tensor(asd).double()]
        parts.append(lw)
        if hd95:
            parts.append(lh)
        parts += [ln, sd]
        if bins:
            parts.append(cal)
        rows.append(torch.cat(parts))
    table = torch.stack(rows)
    assert table.shape[1] == table_width(2, surface, bins, lesionwise=True, lesionwise_hd95=hd95, surface_dice=3, lesionwise_nsd=1)
    again = metrics_from_table(table, regions, ["d0", "d1"], False, surface, bins, lesionwise=True, lesionwise_hd95=hd95,
                               surface_dice=sd_t, lesionwise_nsd=ln_t)
    want = acc.metrics(False)
    assert again == want and list(again) == list(want)
    # and without the new columns the replay is what it was
    keep = [c for c in range(table.shape[1]) if not (table_width(2, surface, 0, lesionwise=True, lesionwise_hd95=hd95) <= c <
                                                     table_width(2, surface, 0, lesionwise=True, lesionwise_hd95=hd95) + 8)]
    old = metrics_from_table(table[:, keep], regions, ["d0", "d1"], False, surface, bins, lesionwise=True, lesionwise_hd95=hd95)
    assert old == {k: v for k, v in want.items() if "nsd" not in k}


# ----------------------------------------------------------------------------- the C entry points, without a device
NAMES = ["mmtta_surface_dice_scratch_bytes", "mmtta_surface_dice", "mmtta_lesionwise_nsd_scratch_bytes", "mmtta_lesionwise_nsd",
         "mmtta_lesionwise_nsd_list_slots"]


def test_abi_symbols_in_header_and_library():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    assert set(NAMES) <= set(_lib.exported_names())
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert getattr(lib, name) is not None
    assert "#define MMTTA_ABI_VERSION 2" in header and lib.mmtta_abi_version() == 2
    assert 1 <= ops.lesionwise_nsd_list_slots() <= 8


def _tensor(_lib, shape, dtype=None):
    n, r, d, h, w = shape
    return _lib.Tensor(4096, n, r, d, h, w, r * d * h * w, d * h * w, h * w, w, 1, _lib.F32 if dtype is None else dtype, 0)


def test_surface_dice_refusals_without_a_gpu():
    from multimodal_tta_amd import _lib
    lib = _lib.load()

    def call(mask=1, label=True, shape=(1, 1, 4, 4, 4), spacing=(1.0, 1.0, 1.0), tol=(1.0,), T=None, counts=1, scratch=1, dtype=None):
        sp = (ctypes.c_double * 3)(*spacing) if spacing is not None else None
        tl = (ctypes.c_double * max(1, len(tol)))(*tol) if tol is not None else None
        t = _tensor(_lib, shape, dtype)
        return lib.mmtta_surface_dice(mask, ctypes.byref(t) if label else None, sp, tl, len(tol) if T is None and tol is not None else (T or 0),
                                      counts, scratch, None)

    # (the pointers here are never followed: every call is refused before anything is queued)
    for kw, word in ((dict(mask=None), b"pred_mask"), (dict(label=False), b"label"), (dict(spacing=None), b"spacing"),
                     (dict(tol=None, T=1), b"tolerances"), (dict(counts=None), b"counts"), (dict(scratch=None), b"scratch")):
        assert call(**kw) == -1 and b"null" in lib.mmtta_last_error() and word in lib.mmtta_last_error(), kw
    for T in (0, 5, 6, -1):
        assert call(tol=(1.0,) * 6, T=T) == -1 and b"n_tolerances" in lib.mmtta_last_error(), T
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert call(tol=(1.0, bad)) == -1 and b"tolerances[1]" in lib.mmtta_last_error(), bad
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        assert call(spacing=bad) == -1 and b"spacing" in lib.mmtta_last_error(), bad
    assert call(tol=(9.0,)) == -2 and b"tolerances" in lib.mmtta_last_error() and b"mmtta_surface_distances" in lib.mmtta_last_error()
    assert call(tol=(6.8,), spacing=(2.0, 1.0, 0.75)) == -2 and b"window" in lib.mmtta_last_error()
    assert call(shape=(1, 1, 4, 4, 1025)) == -2 and b"1024" in lib.mmtta_last_error()
    assert call(shape=(1, 1, 0, 4, 4)) == -1 and b"extent" in lib.mmtta_last_error()
    assert call(shape=(65535, 2, 1, 1, 1)) == -2 and b"65535" in lib.mmtta_last_error()
    assert call(dtype=_lib.BF16) == -2 and b"fp32" in lib.mmtta_last_error()
    assert lib.mmtta_surface_dice_scratch_bytes(6, 128, 128, 128) == 2 * 6 * 128 * 128 * 2 * 8      # two bit planes
    assert lib.mmtta_surface_dice_scratch_bytes(1, 1, 1, 5) > 0 and lib.mmtta_surface_dice_scratch_bytes(1, 1024, 8, 8) > 0
    for bad in ((1, 1025, 8, 8), (1, 8, 8, 1025), (0, 4, 4, 4), (1, 0, 4, 4), (65536, 4, 4, 4)):
        assert lib.mmtta_surface_dice_scratch_bytes(*bad) < 0, bad


def test_lesionwise_nsd_refusals_without_a_gpu():
    from multimodal_tta_amd import _lib
    lib = _lib.load()

    def call(mask=1, n=1, r=1, d=4, h=4, w=4, spacing=(1.0, 1.0, 1.0), tol=(0.5, 1.0), T=None, lw=1, stats=1, scratch=1,
             min_voxels=None, has_min=True):
        mv = (ctypes.c_int64 * 64)(*(min_voxels or [0] * 64))
        sp = (ctypes.c_double * 3)(*spacing) if spacing is not None else None
        tl = (ctypes.c_double * max(1, len(tol)))(*tol) if tol is not None else None
        return lib.mmtta_lesionwise_nsd(mask, n, r, d, h, w, sp, tl, len(tol) if T is None and tol is not None else (T or 0),
                                        mv if has_min else None, lw, stats, None, scratch, None)

    for kw, word in ((dict(mask=None), b"mask"), (dict(spacing=None), b"spacing"), (dict(tol=None, T=1), b"tolerances"),
                     (dict(has_min=False), b"min_lesion_voxels"), (dict(lw=None), b"lesionwise_scratch"),
                     (dict(stats=None), b"nsd_stats"), (dict(scratch=None), b"scratch")):
        assert call(**kw) == -1 and b"null" in lib.mmtta_last_error() and word in lib.mmtta_last_error(), kw
    for T in (0, 5, 6):
        assert call(tol=(1.0,) * 6, T=T) == -1 and b"n_tolerances" in lib.mmtta_last_error(), T
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(tol=(bad,)) == -1 and b"tolerances[0]" in lib.mmtta_last_error(), bad
    assert call(spacing=(1.0, 0.0, 1.0)) == -1 and b"spacing" in lib.mmtta_last_error()
    assert call(tol=(9.0,)) == -2 and b"tolerances" in lib.mmtta_last_error()
    assert call(r=65) == -2 and b"65" in lib.mmtta_last_error()
    assert call(d=0) == -1 and b"extent" in lib.mmtta_last_error()
    assert call(n=65535, r=2, d=1, h=1, w=1) == -2 and b"limits" in lib.mmtta_last_error()
    assert call(min_voxels=[-5] + [0] * 63) == -1 and b"min_lesion_voxels" in lib.mmtta_last_error()
    V = 128 ** 3
    nb = lib.mmtta_lesionwise_nsd_scratch_bytes(6, 128, 128, 128)
    assert 6 * V * (6 * 4) + 3 * 6 * V // 8 <= nb < 6 * V * 25      # six words per voxel and three bit planes
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (65536, 4, 4, 4), (1, 2048, 2048, 1024)):
        assert lib.mmtta_lesionwise_nsd_scratch_bytes(*bad) < 0, bad


def test_default_tolerances_never_refuse_a_fine_spacing():
    """The window cap is a matter of an enabled block: with the blocks absent or off - with or without tolerances written
    out - the evaluators construct at any spacing, as they did before the blocks existed."""
    from multimodal_tta_amd.evaluation import TTASegmentationEvaluationStrategy
    fine = {"spacing": [1.0, 1.0, 0.1]}
    for extra in ({}, {"surface_dice": {"enable": False}, "lesionwise": {"enable": True, "nsd": {"enable": False}}},
                  {"surface_dice": {"enable": False, "tolerances": [1.0]},
                   "lesionwise": {"enable": True, "nsd": {"enable": False, "tolerances": [0.5, 1.0]}}}):
        cfg = {"evaluation": dict(extra, seg=dict(fine))}
        assert surface_dice_config(cfg) == (False, [1.0]) and lesionwise_nsd_config(cfg) == (False, [0.5, 1.0])
        for cls in (SegmentationEvaluationStrategy, TTASegmentationEvaluationStrategy):
            strat = cls(cfg)
            assert strat.spacing == (1.0, 1.0, 0.1) and not strat.enable_surface_dice and not strat.enable_lesionwise_nsd
    # enabled, the defaults are checked like any other value
    for cfg, key in (({"evaluation": {"seg": dict(fine), "surface_dice": {"enable": True}}}, "evaluation.surface_dice"),
                     ({"evaluation": {"seg": dict(fine), "lesionwise": {"enable": True, "nsd": {"enable": True}}}}, "evaluation.lesionwise.nsd")):
        with pytest.raises(ValueError, match=re.escape(key) + r"\.tolerances"):
            SegmentationEvaluationStrategy(cfg)
    ok = SegmentationEvaluationStrategy({"evaluation": {"seg": dict(fine), "surface_dice": {"enable": True, "tolerances": [0.5]}}})
    assert ok.sd_tolerances == [0.5]


@pytest.mark.parametrize("task", ["brats", "hecktor21"])
def test_shipped_configs_construct_at_a_fine_spacing_with_the_blocks_off(task):
    """The shipped configs carry `surface_dice: {enable: false, tolerances: [1.0]}` written out: composed as a user composes
    them, at a spacing whose window for 1 mm would be beyond the cap, both evaluators construct, with and without the
    lesion-wise scores, and nothing of NSD is on; switching a block on at that spacing is what raises."""
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.evaluation import TTASegmentationEvaluationStrategy
    for extra in ([], ["evaluation.lesionwise.enable=true"], ["evaluation.lesionwise.enable=true", "+evaluation.lesionwise.nsd.enable=false"]):
        cfg = compose(overrides=[f"task={task}", f"dataset={task}", "model=unet", "method=tta_entmin",
                                 "evaluation.seg.spacing=[1.0,1.0,0.1]"] + extra)
        assert cfg["evaluation"]["surface_dice"]["enable"] is False and list(cfg["evaluation"]["surface_dice"]["tolerances"]) == [1.0]
        for cls in (SegmentationEvaluationStrategy, TTASegmentationEvaluationStrategy):
            strat = cls(cfg)
            assert strat.spacing == (1.0, 1.0, 0.1) and not strat.enable_surface_dice and not strat.enable_lesionwise_nsd
            assert strat.sd_tolerances == [] and strat.ln_tolerances == []
    cfg = compose(overrides=[f"task={task}", f"dataset={task}", "model=unet", "method=tta_entmin",
                             "evaluation.seg.spacing=[1.0,1.0,0.1]", "evaluation.surface_dice.enable=true"])
    with pytest.raises(ValueError, match=r"evaluation\.surface_dice\.tolerances"):
        SegmentationEvaluationStrategy(cfg)


def test_nsd_kernels_have_no_scratch_and_no_spills():
    """Resource figures of the built code objects (scripts/kernel_resources.py).  The lesion-wise window kernels keep their
    window constants in vector registers on purpose (sd_vreg in surface_dice.hip); a compiler under which that no longer
    holds them clear of spills shows up here."""
    import sys
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    table = kernel_resources.figures(os.path.join(ROOT, "multimodal_tta_amd", "csrc", "libmmtta.so"))
    mine = {k: v for k, v in table.items() if "SdArgs" in k or "LnArgs" in k}
    assert len(mine) == 8, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["vgpr"] <= 128 and v["lds"] <= 64, (k, v)      # four 256-thread blocks per CU; LDS only for the block sums


def test_ops_wrappers_check_before_the_library():
    from multimodal_tta_amd._lib import MmttaError
    m, lab = torch.zeros((1, 1, 2, 2, 2), dtype=torch.uint8), torch.zeros((1, 1, 2, 2, 2))
    assert ops.SURFACE_DICE_COLUMNS == ("hits_pred", "edge_pred", "hits_gt", "edge_gt") and ops.LESIONWISE_NSD_Q_ONE == Q30
    for fn in (ops.surface_dice, ops.lesionwise_nsd):
        with pytest.raises(MmttaError, match="spacing"):
            fn(m, lab, spacing=(1.0, 0.0, 1.0))
        for bad in ((), (1.0,) * 5, (-1.0,), (float("nan"),), "1"):
            with pytest.raises(MmttaError, match="tolerances"):
                fn(m, lab, tolerances=bad)
        with pytest.raises(MmttaError, match="window.*surface_distances"):
            fn(m, lab, tolerances=(9.0,))
        with pytest.raises(MmttaError, match="dense"):
            fn(m, lab)      # not on the device
    for bad in (m, m.float(), torch.zeros((2, 2, 2), dtype=torch.uint8), torch.zeros((1, 1, 2, 2, 4), dtype=torch.uint8)[..., ::2]):
        with pytest.raises(MmttaError, match="dense CUDA uint8"):
            ops.lesionwise_nsd_after_scores(bad, 0, (1.0, 1.0, 1.0), (1.0,))
