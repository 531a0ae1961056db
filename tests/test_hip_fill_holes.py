"""Hole filling and region nesting (mmtta_mask_fill_nest) against scipy on the CPU, and the evaluators that run it behind
the component filter.

The oracle: `scipy.ndimage.binary_fill_holes` with `generate_binary_structure(3, 1 | 2 | 3)` for `fill_connectivity`
6 | 18 | 26; what it adds to the mask are the holes, `scipy.ndimage.label` (same structure) separates them and
`np.bincount` gives their sizes for the cap; the nesting is numpy.  Masks, counts and stats are integers and must be exactly
equal: there is no tolerance anywhere in this file.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REAL_SHAPES = [(17, 33, 70), (9, 20, 48), (40, 40, 40)]
SHAPES = REAL_SHAPES + [(1, 1, 5), (3, 1, 1)]
CONNECTIVITIES = (6, 18, 26)
N, R = 2, 3
BIG = (17, 33, 70)
_id = lambda s: "x".join(map(str, s))


# ----------------------------------------------------------------------------- the scipy / numpy oracle
def holes_of(mask, conn):
    """mask bool [D,H,W] -> (labels of its holes int [D,H,W], 0 elsewhere; sizes of the holes, label k at k - 1)."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
    holes = ndimage.binary_fill_holes(mask, structure=st) & ~mask
    # two holes are two background components: they do not touch at this connectivity, so `label` keeps them apart
    lab, n = ndimage.label(holes, structure=st)
    return lab, np.bincount(lab.ravel(), minlength=n + 1)[1:]


def oracle(mask, label, conn, fill, cap, chain=(), mode="clip"):
    """mask uint8 [N,R,D,H,W], label float or None -> final mask uint8, counts [N,R,3] (None without a label), stats [N,R,4]."""
    n_, r_ = mask.shape[:2]
    old = np.zeros(mask.shape, dtype=bool)
    stats = np.zeros((n_, r_, 4), dtype=np.int64)
    for n in range(n_):
        for r in range(r_):
            m = mask[n, r] != 0
            lab, sizes = holes_of(m, conn)
            ok = np.zeros(sizes.size + 1, dtype=bool)
            if fill[r]:
                ok[1:] = (sizes <= cap[r]) if cap[r] else True
            filled = ok[lab]
            old[n, r] = m | filled
            stats[n, r, :3] = (sizes.size, int(ok.sum()), int(filled.sum()))
    new = old.copy()
    chain = list(chain)
    for i, c in enumerate(chain):
        if mode == "clip":
            new[:, c] = np.logical_and.reduce([old[:, k] for k in chain[i:]])
        else:
            new[:, c] = np.logical_or.reduce([old[:, k] for k in chain[:i + 1]])
    stats[..., 3] = (new != old).reshape(n_, r_, -1).sum(-1)
    counts = None
    if label is not None:
        g = label > 0.5
        counts = np.stack([(new & g).reshape(n_, r_, -1).sum(-1), new.reshape(n_, r_, -1).sum(-1),
                           g.reshape(n_, r_, -1).sum(-1)], -1).astype(np.int64)
    return new.astype(np.uint8), counts, stats


def run(mask, label, conn, fill, cap=0, chain=(), mode="clip"):
    from multimodal_tta_amd import ops
    m = torch.from_numpy(mask.copy()).cuda()
    lab = torch.from_numpy(label.copy()).cuda() if label is not None else None
    keep = lab.clone() if lab is not None else None
    res = ops.fill_nest(m, lab, fill, conn, cap, chain, mode)
    torch.cuda.synchronize()
    assert res["mask"] is m, "the pass runs in place"
    if lab is not None:
        assert torch.equal(lab, keep), "the label was written"
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in res.items()}


def assert_equal(got, want, what):
    mask, counts, stats = want
    assert got["stats"].shape == stats.shape and np.array_equal(got["stats"], stats), f"{what}: stats\n{got['stats']}\n{stats}"
    assert got["mask"].dtype == np.uint8 and np.array_equal(got["mask"], mask), f"{what}: final mask"
    if counts is None:
        assert got["counts"] is None
    else:
        assert np.array_equal(got["counts"], counts), f"{what}: counts\n{got['counts']}\n{counts}"


@functools.lru_cache(maxsize=None)
def random_case(shape, density):
    rng = np.random.default_rng(7000 + int(round(100 * density)) + sum(shape))
    mask = (rng.random((N, R) + shape) < density).astype(np.uint8)
    label = (rng.random((N, R) + shape) < 0.4).astype(np.float32)
    mask.setflags(write=False)
    label.setflags(write=False)
    return mask, label


# ----------------------------------------------------------------------------- 1. random masks
@pytest.mark.parametrize("conn", CONNECTIVITIES)
@pytest.mark.parametrize("density", [0.30, 0.60, 0.85])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_random_masks_match_scipy(shape, density, conn):
    mask, label = random_case(shape, density)
    for fill in ([True, False, True], [False, True, True]):
        want = oracle(mask, label, conn, fill, [0, 0, 0])
        if density == 0.85 and shape in REAL_SHAPES:      # the case is worth something only if there is a hole to fill
            assert want[2][..., 0].min() >= 1, f"{shape} connectivity {conn}: the oracle found a mask without a hole"
            assert want[2][..., 2].sum() > 0
        assert_equal(run(mask, label, conn, fill), want, f"{shape} density {density} connectivity {conn} fill {fill}")


# ----------------------------------------------------------------------------- 2. structured masks
CAVITY = (slice(2, 14), slice(2, 30), slice(2, 68))      # z 2..13, y 2..29, x 2..67: whole 4 x 8 x 32 tiles lie inside it


def _box(m, z, y, x, v=1):
    m[:, :, z[0]:z[1] + 1, y[0]:y[1] + 1, x[0]:x[1] + 1] = v


def _structured(kind):
    """-> (mask uint8 [N,R,17,33,70], holes of one mask at connectivity 6 / 18 / 26)."""
    D, H, W = BIG
    m = np.zeros((N, R, D, H, W), dtype=np.uint8)
    if kind == "ones":
        m[:] = 1
        holes = (0, 0, 0)
    elif kind == "zeros":
        holes = (0, 0, 0)
    elif kind == "shell":
        _box(m, (1, 14), (1, 30), (1, 68))
        m[(slice(None), slice(None)) + CAVITY] = 0
        holes = (1, 1, 1)
    elif kind == "shell_on_face":            # the wall is the z = 0, y = 0 and x = 0 faces themselves: still closed
        _box(m, (0, 13), (0, 29), (0, 67))
        _box(m, (1, 12), (1, 28), (1, 66), 0)
        holes = (1, 1, 1)
    elif kind == "shell_open_on_face":       # the same without its wall on z = 0: the cavity reaches the face
        _box(m, (0, 13), (0, 29), (0, 67))
        _box(m, (0, 12), (1, 28), (1, 66), 0)
        holes = (0, 0, 0)
    elif kind == "tunnel":                   # a block with a tunnel right through it along x
        _box(m, (4, 12), (4, 28), (4, 60))
        _box(m, (8, 8), (16, 16), (4, 60), 0)
        holes = (0, 0, 0)
    elif kind in ("edge_gap", "corner_gap"):
        # a one-voxel cavity in a block, and a shaft from outside that ends diagonally next to it: over an edge (closed
        # at 6, open at 18 and 26) or over a corner (open at 26 only)
        _box(m, (2, 14), (2, 30), (2, 67))
        m[:, :, 8, 16, 30] = 0
        _box(m, (2, 7), (15, 15), (30, 30) if kind == "edge_gap" else (29, 29), 0)
        holes = (1, 0, 0) if kind == "edge_gap" else (1, 1, 0)
    elif kind == "shell_in_shell":
        _box(m, (1, 14), (1, 30), (1, 68))
        m[(slice(None), slice(None)) + CAVITY] = 0
        _box(m, (4, 11), (6, 25), (10, 50))
        _box(m, (5, 10), (7, 24), (11, 49), 0)
        holes = (2, 2, 2)
    elif kind == "partial_tiles":            # a closed cell in the corner tile that hangs over the volume on three sides
        _box(m, (13, 16), (29, 32), (64, 69))
        _box(m, (14, 15), (30, 31), (65, 68), 0)
        holes = (1, 1, 1)
    # the items and regions differ a little, so a mix-up of (n, r) shows
    m[1, 2] = m[1, 2][::-1, ::-1, ::-1]
    return m, holes


@pytest.mark.parametrize("kind", ["ones", "zeros", "shell", "shell_on_face", "shell_open_on_face", "tunnel", "edge_gap",
                                  "corner_gap", "shell_in_shell", "partial_tiles"])
def test_structured_masks_match_scipy(kind):
    mask, holes = _structured(kind)
    label = (mask > 0).astype(np.float32)
    label[0, 1] = 0
    for conn, nh in zip(CONNECTIVITIES, holes):
        for fill in ([True, True, True], [True, False, True]):
            got = run(mask, label, conn, fill)
            want = oracle(mask, label, conn, fill, [0, 0, 0])
            assert_equal(got, want, f"{kind} connectivity {conn} fill {fill}")
        assert (want[2][..., 0] == nh).all(), f"{kind} connectivity {conn}: holes {want[2][..., 0]}"
        assert got["stats"][0, 0].tolist()[:2] == [nh, nh] and got["stats"][0, 1].tolist()[:3] == [nh, 0, 0]
        if kind == "shell":
            assert got["stats"][0, 0, 2] == 12 * 28 * 66 and got["mask"][0, 0, 1:15, 1:31, 1:69].all()
        if kind == "shell_in_shell":
            assert got["mask"][0, 0, 1:15, 1:31, 1:69].all() and got["mask"][0, 0].sum() == 14 * 30 * 68


# ----------------------------------------------------------------------------- 3. the cap
def test_cap_fills_the_small_holes_only():
    mask = np.zeros((N, R) + BIG, dtype=np.uint8)
    _box(mask, (1, 15), (1, 31), (1, 68))
    mask[:, :, 4, 4, 4] = 0                                   # 1 voxel
    for dz, dy, dx in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        mask[:, :, 8 + dz, 16 + dy, 40 + dx] = 0              # 7 voxels: a cross
    _box(mask, (11, 12), (24, 25), (60, 61), 0)               # 8 voxels: a cube
    label = (mask == 0).astype(np.float32)
    for cap, filled, voxels in (7, 2, 8), (0, 3, 16), (8, 3, 16), (1, 1, 1):
        got = run(mask, label, 6, True, cap)
        assert_equal(got, oracle(mask, label, 6, [True] * R, [cap] * R), f"cap {cap}")
        assert got["stats"][0, 0].tolist() == [3, filled, voxels, 0]
    got = run(mask, label, 6, [True, True, False], [7, 0, 0])
    assert_equal(got, oracle(mask, label, 6, [True, True, False], [7, 0, 0]), "cap per region")
    assert got["stats"][1].tolist() == [[3, 2, 8, 0], [3, 3, 16, 0], [3, 0, 0, 0]]


# ----------------------------------------------------------------------------- 4. nesting
@pytest.mark.parametrize("mode", ["clip", "grow"])
@pytest.mark.parametrize("chain", [(0, 1, 2), (2, 0, 1), (0, 2)], ids=_id)
def test_nesting_matches_numpy(chain, mode):
    for shape in ((9, 20, 48), (1, 1, 5)):
        mask, label = random_case(shape, 0.60)
        for fill in (False, [True, False, True]):
            fl = [fill] * R if isinstance(fill, bool) else fill
            got = run(mask, label, 6, fill, 0, chain, mode)
            want = oracle(mask, label, 6, fl, [0] * R, chain, mode)
            assert_equal(got, want, f"{shape} chain {chain} {mode} fill {fill}")
            if shape != (1, 1, 5):
                assert want[2][..., 3].sum() > 0, "the chain changed nothing: the case shows nothing"
            if len(chain) == 2:          # the region outside the chain passes through (filled or not), nothing nested in it
                assert np.array_equal(got["mask"][:, 1], oracle(mask, None, 6, fl, [0] * R)[0][:, 1])
                assert (got["stats"][:, 1, 3] == 0).all()
            inner, outer = got["mask"][:, chain[0]], got["mask"][:, chain[-1]]
            assert (inner <= outer).all(), "the chain is not nested afterwards"


def test_nesting_sees_the_filled_masks():
    mask = np.zeros((N, R) + BIG, dtype=np.uint8)
    et, tc, wt = mask[:, 0], mask[:, 1], mask[:, 2]
    wt[:, 1:16, 1:32, 1:69] = 1
    tc[:, 3:12, 4:24, 8:50] = 1
    tc[:, 5:9, 8:16, 20:40] = 0              # a hole in TC ...
    et[:, 6:8, 10:14, 25:30] = 1             # ... that ET lies in without covering it
    et[:, 4:11, 5:22, 52:64] = 1             # ET with a hole of its own, outside TC
    et[:, 6:8, 8:12, 55:60] = 0
    label = (mask > 0).astype(np.float32)
    fill = [True, True, False]
    for mode in ("clip", "grow"):
        got = run(mask, label, 6, fill, 0, (0, 1, 2), mode)
        want = oracle(mask, label, 6, fill, [0] * R, (0, 1, 2), mode)
        assert_equal(got, want, f"fill then {mode}")
        assert got["stats"][0, :2, :3].tolist() == [[1, 1, 2 * 4 * 5], [1, 1, 4 * 8 * 20]]
    # clip: ET inside the filled TC hole stays (TC covers it now), ET outside TC goes, filled hole and all
    clip = run(mask, label, 6, fill, 0, (0, 1, 2), "clip")
    assert clip["mask"][0, 0, 6:8, 10:14, 25:30].all() and not clip["mask"][0, 0, :, :, 52:64].any()
    assert clip["stats"][0, 0, 3] == 7 * 17 * 12 and clip["stats"][0, 1, 3] == 0
    # without the filling ET in the TC hole would have been clipped away
    bare = run(mask, label, 6, False, 0, (0, 1, 2), "clip")
    assert not bare["mask"][0, 0].any()
    # grow: TC takes all of ET, its filled hole included
    grow = run(mask, label, 6, fill, 0, (0, 1, 2), "grow")
    assert grow["mask"][0, 1, 4:11, 5:22, 52:64].all() and grow["stats"][0, 1, 3] == 7 * 17 * 12


# ----------------------------------------------------------------------------- 5. batches, repeats, what is written
def test_batch_repeat_and_what_is_written():
    from multimodal_tta_amd import ops
    mask, label = random_case(BIG, 0.85)
    args = (18, [True, False, True], [0, 0, 5], (0, 1, 2), "clip")
    a, b = run(mask, label, *args), run(mask, label, *args)
    for k in ("mask", "counts", "stats"):
        assert np.array_equal(a[k], b[k]), f"two calls differ in {k}"
    assert_equal(a, oracle(mask, label, 18, *args[1:]), "batch")
    for n in range(N):
        one = run(mask[n:n + 1], label[n:n + 1].copy(), *args)
        for k in ("mask", "counts", "stats"):
            assert np.array_equal(a[k][n:n + 1], one[k]), f"item {n} alone differs in {k}"
    # counts = what mask_dice_counts reports for logits that threshold to the final mask
    logits = torch.from_numpy((a["mask"].astype(np.float32) * 2 - 1) * 4).cuda()
    counts = torch.empty((N, R, 3), dtype=torch.int64, device="cuda")
    ops.mask_dice_counts(logits, torch.from_numpy(label.copy()).cuda(), 0.5, counts, None, logits_channels_last=False)
    assert np.array_equal(counts.cpu().numpy(), a["counts"])
    # no label, no counts
    c = run(mask, None, *args)
    assert c["counts"] is None and np.array_equal(c["mask"], a["mask"]) and np.array_equal(c["stats"], a["stats"])
    # a mask whose foreground is not 1, a strided label view, a side stream
    wide = torch.zeros((N, R) + BIG[:2] + (BIG[2] + 3,), device="cuda")
    wide[..., :BIG[2]] = torch.from_numpy(label.copy()).cuda()
    m = torch.from_numpy(mask * 200).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = ops.fill_nest(m, wide[..., :BIG[2]], args[1], 18, args[2], args[3], args[4])
    s.synchronize()
    assert np.array_equal(res["counts"].cpu().numpy(), a["counts"]) and np.array_equal(m.cpu().numpy(), a["mask"])


def test_ops_rejects_bad_arguments():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    m = torch.zeros((1, 2, 4, 4, 4), dtype=torch.uint8, device="cuda")
    for kw, word in ((dict(fill_connectivity=8), "fill_connectivity"), (dict(fill_holes=[True] * 3), "fill_holes"),
                     (dict(max_hole_voxels=-1), "max_hole_voxels"), (dict(nesting=[0]), "nesting"),
                     (dict(nesting=[0, 0]), "nesting"), (dict(nesting=[0, 2]), "nesting"), (dict(nesting_mode="shrink"), "nesting_mode"),
                     (dict(label_ncdhw=torch.zeros((1, 2, 4, 4, 5), device="cuda")), "label")):
        with pytest.raises(MmttaError, match=word):
            ops.fill_nest(m, **kw)
    with pytest.raises(MmttaError, match="dense"):
        ops.fill_nest(m[:, :, :, :, ::2])


# ----------------------------------------------------------------------------- 6. evaluators
REGIONS = ["ET", "TC", "WT"]
PP = {"enable": True, "connectivity": 18, "min_voxels": [0, 4, 12], "keep_largest": [True, False, False]}
FILL = {"fill_holes": [True, False, True], "fill_connectivity": 6, "max_hole_voxels": [0, 0, 6], "nesting": ["ET", "TC", "WT"],
        "nesting_mode": "clip"}
DEFAULTS = {"fill_holes": False, "fill_connectivity": 6, "max_hole_voxels": 0, "nesting": [], "nesting_mode": "clip"}
NEW_KEYS = {f"{p}{r}_{k}" for p in ("", "dom/synth/") for r in ("et", "tc", "wt")
            for k in ("holes", "filled_holes", "filled_voxels", "nested_voxels")}


def _cfg(block, threshold, **method):
    from test_hip_components import _e2e_cfg
    cfg = _e2e_cfg(block, threshold, **method)
    cfg["evaluation"]["lesionwise"] = {"enable": True, "dilation": 1}
    return cfg


def _expected_metrics(strat, raw_masks, labels):
    """The host restatement: raw masks uint8 [V,R,D,H,W] -> filter (scipy) -> fill (scipy) -> nest (numpy) -> the final masks
    and, through the package's own accumulator, every key of the run.  HD95 / ASD and the lesion-wise scores are taken with
    the package's ops ON THE FINAL MASKS, which is what the evaluators must have handed them."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.evaluation import RegionAccumulator, dice_iou_from_counts, lesionwise_columns
    from test_hip_components import oracle as filter_oracle
    _, filt, _, cstats = filter_oracle(raw_masks, labels, PP["connectivity"], PP["min_voxels"], PP["keep_largest"])
    final, counts, fstats = oracle(filt, labels, FILL["fill_connectivity"], FILL["fill_holes"], FILL["max_hole_voxels"],
                                   [REGIONS.index(x) for x in FILL["nesting"]], FILL["nesting_mode"])
    counts = torch.from_numpy(counts)
    dice, iou, valid = dice_iou_from_counts(counts)
    fm, lab = torch.from_numpy(final).cuda(), torch.from_numpy(labels).cuda()
    hd, asd = ops.surface_distances(fm, lab, strat.spacing, 95.0, strat.asd_symmetric)
    hd, asd = strat.surface_fix(hd, asd, counts, raw_masks.shape[2:])
    lw = strat.lesionwise_launch(fm, lab).cpu()
    acc = RegionAccumulator(REGIONS, True, 0, None, True, True, True)
    for i in range(raw_masks.shape[0]):
        acc.add_row(dice[i].tolist(), iou[i].tolist(), valid[i].tolist(), "synth", hd[i].tolist(), asd[i].tolist(), None,
                    torch.from_numpy(cstats[i]).double().t().reshape(-1), lesionwise_columns(lw[i]),
                    torch.from_numpy(fstats[i]).double().t().reshape(-1))
    return final, acc.metrics(False), fstats


def _check(m_on, m_base, m_dflt, want, fstats):
    assert fstats[..., 2].sum() > 0 and fstats[..., 3].sum() > 0, "nothing filled or nothing nested: the case shows nothing"
    assert m_dflt == m_base and list(m_dflt) == list(m_base)          # the new keys at their defaults: today's run exactly
    assert not NEW_KEYS & set(m_base)
    assert set(m_on) == set(m_base) | NEW_KEYS
    want = dict(want, loss=m_base["loss"])                           # the reported loss stays on the logits
    assert m_on == want, {k: (m_on[k], want[k]) for k in want if m_on[k] != want[k]}
    V = fstats.shape[0]
    for r, name in enumerate(("et", "tc", "wt")):
        for col, key in enumerate(("holes", "filled_holes", "filled_voxels", "nested_voxels")):
            assert m_on[f"{name}_{key}"] == float(np.float64(fstats[:, r, col].sum()) / V)
    assert m_on["avg_dc"] != m_base["avg_dc"] and m_on["avg_hd95"] != m_base["avg_hd95"]


def test_seg_tta_eval_fills_and_nests_its_masks():
    from multimodal_tta_amd.evaluation import table_width
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_components import _speckle_threshold
    from test_hip_tta import SMALL, build_pair

    runs = {}
    thr = _speckle_threshold()
    for name, block in (("on", {**PP, **FILL}), ("base", PP), ("defaults", {**PP, **DEFAULTS}), ("off", {**PP, **FILL, "enable": False})):
        cfg = _cfg(block, thr, lanes=2, group=2)
        _, hip = build_pair(SMALL)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_tta_eval")(cfg)
        runs[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
    (m_on, s_on), (m_base, s_base), (m_dflt, s_dflt), (_, s_off) = (runs[k] for k in ("on", "base", "defaults", "off"))
    assert s_on.enable_fill_nest and not s_base.enable_fill_nest and not s_dflt.enable_fill_nest and not s_off.enable_fill_nest
    assert torch.equal(s_dflt.last_table, s_base.last_table)
    labels = np.concatenate([b["label"].numpy() for b in loader]).astype(np.float32)
    raw = np.stack([s_off.last_masks[i].numpy() for i in range(3)])      # post-processing off: the thresholded masks
    final, want, fstats = _expected_metrics(s_on, raw, labels)
    for i in range(3):
        assert np.array_equal(s_on.last_masks[i].numpy(), final[i]), f"volume {i}: gathered mask is not the final one"
    _check(m_on, m_base, m_dflt, want, fstats)
    # the table: the component columns, then holes[R], filled holes[R], filled voxels[R], nested voxels[R], then lesion-wise
    c0 = table_width(3, True, components=True)
    assert s_on.last_table.shape == (3, table_width(3, True, components=True, lesionwise=True, fill_nest=True))
    assert s_on.last_table.shape[1] == s_base.last_table.shape[1] + 12
    assert np.array_equal(s_on.last_table[:, c0:c0 + 12].numpy(), fstats.transpose(0, 2, 1).reshape(3, 12).astype(np.float64))


def test_seg_eval_fills_and_nests_its_masks():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_components import _speckle_threshold
    from test_hip_tta import SMALL, build_pair

    _, hip = build_pair(SMALL)
    res = {}
    thr = _speckle_threshold()
    for name, block in (("on", {**PP, **FILL}), ("base", PP), ("defaults", {**PP, **DEFAULTS})):
        cfg = _cfg(block, thr)
        cfg["training"]["eval_batch_size"] = 2
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_eval")(cfg)
        res[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
    (m_on, s_on), (m_base, _), (m_dflt, _) = res["on"], res["base"], res["defaults"]
    raw, labels = [], []
    with torch.no_grad():
        for batch in loader:
            y = batch["label"].cuda().float()
            mask = torch.empty(tuple(y.shape), dtype=torch.uint8, device="cuda")
            counts = torch.empty((y.shape[0], 3, 3), dtype=torch.int64, device="cuda")
            ops.mask_dice_counts(hip(batch["image"].cuda()).float(), y, s_on.threshold, counts, mask, logits_channels_last=False)
            raw.append(mask.cpu().numpy())
            labels.append(batch["label"].numpy().astype(np.float32))
    _, want, fstats = _expected_metrics(s_on, np.concatenate(raw), np.concatenate(labels))
    _check(m_on, m_base, m_dflt, want, fstats)
