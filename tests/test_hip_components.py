"""Connected-component filtering (mmtta_components_filter) against scipy.ndimage.label on the CPU, and the evaluators that
filter their masks with it.

The oracle: `scipy.ndimage.label` with `generate_binary_structure(3, 1 | 2 | 3)` for connectivity 6 | 18 | 26.  Canonical
label of a scipy component = 1 + the smallest linear index of its voxels; sizes from `np.bincount`; the largest component =
the first maximum in scan order (the smallest canonical label among equals).  Labels, masks, counts and stats are integers
and must be exactly equal: there is no tolerance anywhere in this file.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(17, 33, 70), (9, 20, 48), (1, 1, 5), (3, 1, 1), (40, 40, 40)]
CONNECTIVITIES = (6, 18, 26)
N, R = 2, 3
# min_voxels in {0, 1, 7} and keep_largest off / on, mixed per region, both ways round
SETTINGS = [([0, 1, 7], [False, True, False]), ([7, 0, 1], [True, False, True])]
_id = lambda s: "x".join(map(str, s))


# ----------------------------------------------------------------------------- the scipy oracle
def oracle_one(mask, conn):
    """mask bool [D,H,W] -> (canonical labels int32, ids of the components (ascending), sizes)."""
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]))
    flat = lab.ravel()
    canon = np.zeros(flat.shape, dtype=np.int32)
    if n == 0:
        return canon.reshape(mask.shape), np.zeros(0, np.int64), np.zeros(0, np.int64)
    ids, first = np.unique(flat, return_index=True)           # first voxel of every scipy label in scan order
    first = first[ids > 0]
    lut = np.zeros(n + 1, dtype=np.int64)
    lut[ids[ids > 0]] = first + 1
    canon = lut[flat].astype(np.int32)
    sizes = np.bincount(flat, minlength=n + 1)[1:]
    order = np.argsort(lut[1:])
    return canon.reshape(mask.shape), lut[1:][order], sizes[order]


def oracle(mask, label, conn, min_voxels, keep_largest):
    """mask uint8 [N,R,D,H,W], label float [N,R,D,H,W] or None -> labels, filtered mask, counts [N,R,3], stats [N,R,3]."""
    n_, r_ = mask.shape[:2]
    labels = np.zeros(mask.shape, dtype=np.int32)
    out = np.zeros(mask.shape, dtype=np.uint8)
    counts = np.zeros((n_, r_, 3), dtype=np.int64)
    stats = np.zeros((n_, r_, 3), dtype=np.int64)
    for n in range(n_):
        for r in range(r_):
            canon, ids, sizes = oracle_one(mask[n, r] != 0, conn)
            labels[n, r] = canon
            ok = sizes >= min_voxels[r]
            ids_ok, sizes_ok = ids[ok], sizes[ok]
            if keep_largest[r] and ids_ok.size:
                ids_ok = ids_ok[np.argmax(sizes_ok):][:1]      # first maximum in scan order
            keep = np.isin(canon, ids_ok) & (canon > 0)
            out[n, r] = keep
            stats[n, r] = (ids.size, ids_ok.size, int((canon > 0).sum() - keep.sum()))
            if label is not None:
                g = label[n, r] > 0.5
                counts[n, r] = ((keep & g).sum(), keep.sum(), g.sum())
    return labels, out, counts, stats


def run(mask, label, conn, min_voxels, keep_largest, in_place=False, want_labels=True):
    from multimodal_tta_amd import ops
    m = torch.from_numpy(mask).cuda()
    keep = m.clone()
    lab = torch.from_numpy(label).cuda() if label is not None else None
    res = ops.components_filter(m, lab, conn, min_voxels, keep_largest, out=m if in_place else None, want_labels=want_labels)
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(m, keep), "the input mask was written"
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in res.items()}


def assert_equal(got, want, what):
    labels, out, counts, stats = want
    assert np.array_equal(got["stats"], stats), f"{what}: stats\n{got['stats']}\n{stats}"
    if got["labels"] is not None:
        assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], labels), f"{what}: labels of the raw mask"
    assert got["mask"].dtype == np.uint8 and np.array_equal(got["mask"], out), f"{what}: filtered mask"
    if got["counts"] is not None:
        assert np.array_equal(got["counts"], counts), f"{what}: counts\n{got['counts']}\n{counts}"


@functools.lru_cache(maxsize=None)
def random_case(shape, density, seed=0):
    rng = np.random.default_rng(1000 * seed + int(density * 100) + sum(shape))
    mask = (rng.random((N, R) + shape) < density).astype(np.uint8)
    label = (rng.random((N, R) + shape) < 0.4).astype(np.float32)
    mask.setflags(write=False)
    label.setflags(write=False)
    return mask, label


# ----------------------------------------------------------------------------- random masks
@pytest.mark.parametrize("conn", CONNECTIVITIES)
@pytest.mark.parametrize("density", [0.05, 0.30, 0.60])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_random_masks_match_scipy(shape, density, conn):
    mask, label = random_case(shape, density)
    for mv, kl in SETTINGS:
        got = run(mask, label, conn, mv, kl)
        want = oracle(mask, label, conn, mv, kl)
        assert_equal(got, want, f"{shape} density {density} connectivity {conn} {mv} {kl}")


# ----------------------------------------------------------------------------- structured masks
def _structured(kind, shape):
    D, H, W = shape
    m = np.zeros((N, R, D, H, W), dtype=np.uint8)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    if kind == "ones":
        m[:] = 1
    elif kind == "zeros":
        pass
    elif kind == "checkerboard":
        m[:] = ((z + y + x) % 2 == 0)
    elif kind == "faces":              # x = 0 and x = W - 1 set, the middle empty: two components unless rows wrap
        m[..., 0] = 1
        m[..., W - 1] = 1
    elif kind == "serpentine":         # one voxel wide: along W, one step in y at the end, back; slices joined at the snake's end
        for zz in range(0, D, 2):
            last = (0, 0)
            for k, yy in enumerate(range(0, H, 2)):
                m[:, :, zz, yy, :] = 1
                end = W - 1 if k % 2 == 0 else 0
                last = (yy, end)
                if yy + 1 < H:
                    m[:, :, zz, yy + 1, end] = 1
                    last = (yy + 1, end)
            if zz + 1 < D:
                m[:, :, zz + 1, last[0], last[1]] = 1
    elif kind == "diagonals":          # pairs joined by an edge diagonal (18, 26) and by a corner diagonal (26 only)
        if D >= 2 and H >= 2 and W >= 8:
            m[:, :, 0, 0, 0] = 1
            m[:, :, 0, 1, 1] = 1       # edge diagonal in the plane
            m[:, :, 0, 0, 4] = 1
            m[:, :, 1, 1, 5] = 1       # corner diagonal
            m[:, :, D - 1, H - 1, W - 1] = 1
            m[:, :, D - 2, H - 1, W - 2] = 1      # edge diagonal across z
            m[:, :, D - 1, 0, W - 1] = 1
            m[:, :, D - 2, 1, W - 2] = 1          # corner diagonal at a forward-x / backward-z offset
        else:
            m[..., 0, 0, 0] = 1
    # the items and regions differ a little, so a mix-up of (n, r) shows
    m[1, 2] = m[1, 2][::-1, ::-1, ::-1]
    return m


@pytest.mark.parametrize("kind", ["ones", "zeros", "checkerboard", "faces", "serpentine", "diagonals"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_structured_masks_match_scipy(shape, kind):
    mask = _structured(kind, shape)
    D, H, W = shape
    V = D * H * W
    label = (mask > 0).astype(np.float32)
    label[0, 1] = 0
    for conn in CONNECTIVITIES:
        for mv, kl in ([0, 0, 0], [False, False, True]), ([2, 0, 1], [True, False, False]):
            got = run(mask, label, conn, mv, kl)
            want = oracle(mask, label, conn, mv, kl)
            assert_equal(got, want, f"{kind} {shape} connectivity {conn} {mv} {kl}")
        comps = want[3][0, 0, 0]
        if kind == "ones":
            assert comps == 1 and got["labels"].max() == 1
        elif kind == "zeros":
            assert comps == 0 and not got["mask"].any()
        elif kind == "checkerboard":
            flat = sum(e > 1 for e in shape) < 2               # along a single axis the cells never touch
            assert comps == ((V + 1) // 2 if conn == 6 or flat else 1)
        elif kind == "faces":
            assert comps == (2 if W >= 3 else 1)
        elif kind == "serpentine":
            assert comps == 1
        elif kind == "diagonals" and W >= 8:
            assert comps == {6: 8, 18: 6, 26: 4}[conn]


# ----------------------------------------------------------------------------- ties and empty results
def test_equal_sizes_go_to_the_smaller_first_voxel():
    shape = (9, 20, 48)
    mask = np.zeros((1, 3) + shape, dtype=np.uint8)
    for r in range(3):
        mask[0, r, 5:7, 10:12, 30:32] = 1      # 8 voxels, later in scan order
        mask[0, r, 0:2, 3:5, 40:42] = 1        # 8 voxels, first in scan order
        mask[0, r, 8, 19, 0:5] = 1             # 5 voxels
    first = 1 + (0 * 20 + 3) * 48 + 40
    got = run(mask, None, 26, [0, 6, 9], [True, True, True])
    want = oracle(mask, None, 26, [0, 6, 9], [True, True, True])
    assert_equal(got, want, "ties")
    assert got["counts"] is None
    for r in (0, 1):
        kept = np.unique(got["labels"][0, r][got["mask"][0, r] != 0])
        assert kept.tolist() == [first]
    assert got["stats"][0].tolist() == [[3, 1, 13], [3, 1, 13], [3, 0, 21]]      # the largest is below min_voxels: empty, kept 0
    assert not got["mask"][0, 2].any()


# ----------------------------------------------------------------------------- aliasing, batching, streams
def test_in_place_repeat_batch_and_counts():
    from multimodal_tta_amd import ops
    shape = (17, 33, 70)
    mask, label = random_case(shape, 0.30)
    mv, kl = SETTINGS[0]
    a = run(mask, label, 18, mv, kl)
    b = run(mask, label, 18, mv, kl)
    c = run(mask, label, 18, mv, kl, in_place=True)
    for k in ("mask", "counts", "stats", "labels"):
        assert np.array_equal(a[k], b[k]), f"two calls differ in {k}"
        assert np.array_equal(a[k], c[k]), f"in place differs in {k}"
    for n in range(N):
        one = run(mask[n:n + 1].copy(), label[n:n + 1].copy(), 18, mv, kl)
        for k in ("mask", "counts", "stats", "labels"):
            assert np.array_equal(a[k][n:n + 1], one[k]), f"item {n} alone differs in {k}"
    # counts = what mask_dice_counts reports for logits that threshold to the filtered mask
    logits = torch.from_numpy((a["mask"].astype(np.float32) * 2 - 1) * 4).cuda()
    counts = torch.empty((N, R, 3), dtype=torch.int64, device="cuda")
    ops.mask_dice_counts(logits, torch.from_numpy(label).cuda(), 0.5, counts, None, logits_channels_last=False)
    assert np.array_equal(counts.cpu().numpy(), a["counts"])
    # no label, no counts, no labels, no stats
    res = ops.components_filter(torch.from_numpy(mask).cuda(), None, 18, mv, kl, want_stats=False)
    assert res["counts"] is None and res["stats"] is None and res["labels"] is None
    assert np.array_equal(res["mask"].cpu().numpy(), a["mask"])
    # a strided label view
    wide = torch.zeros((N, R) + shape[:2] + (shape[2] + 3,), device="cuda")
    wide[..., :shape[2]] = torch.from_numpy(label).cuda()
    res = ops.components_filter(torch.from_numpy(mask).cuda(), wide[..., :shape[2]], 18, mv, kl)
    assert np.array_equal(res["counts"].cpu().numpy(), a["counts"])


def test_on_a_side_stream():
    from multimodal_tta_amd import ops
    mask, label = random_case((9, 20, 48), 0.30)
    mv, kl = SETTINGS[1]
    want = oracle(mask, label, 26, mv, kl)
    m, lab = torch.from_numpy(mask).cuda(), torch.from_numpy(label).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = ops.components_filter(m, lab, 26, mv, kl, want_labels=True)
    s.synchronize()
    assert_equal({k: v.cpu().numpy() for k, v in res.items()}, want, "side stream")


def test_ops_rejects_bad_arguments():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    m = torch.zeros((1, 2, 4, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(MmttaError, match="connectivity"):
        ops.components_filter(m, None, 8)
    with pytest.raises(MmttaError, match="min_voxels"):
        ops.components_filter(m, None, 26, [1, 2, 3])
    with pytest.raises(MmttaError, match="min_voxels"):
        ops.components_filter(m, None, 26, -1)
    with pytest.raises(MmttaError, match="dense"):
        ops.components_filter(m[:, :, :, :, ::2], None, 26)
    with pytest.raises(MmttaError, match="label"):
        ops.components_filter(m, torch.zeros((1, 2, 4, 4, 5), device="cuda"), 26)


# ----------------------------------------------------------------------------- evaluators
REGIONS = ["ET", "TC", "WT"]
PP = {"enable": True, "connectivity": 18, "min_voxels": [0, 4, 12], "keep_largest": [True, False, False]}
EPS = 1e-7


def _e2e_cfg(postprocess, threshold=0.5, **method):
    """The small model and loader of the calibration evaluator tests; `postprocess`: the block, or None for no block at all."""
    from test_hip_tta import SMALL, root_cfg
    cfg = root_cfg(SMALL, steps=2, lr=1e-3, tune_volumes=4, **method)
    cfg["dataset"]["synthetic"]["num_volumes"] = 3
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    cfg["evaluation"]["surface"] = {"enable": True, "asd_symmetric": False}
    cfg["evaluation"]["gather_masks"] = True
    cfg["evaluation"]["seg"]["threshold"] = float(threshold)
    cfg["evaluation"].pop("postprocess", None)
    if postprocess is not None:
        cfg["evaluation"]["postprocess"] = dict(postprocess)
    return cfg


def _mean_over_valid(vals, valid):
    """Per region: float64 mean of the fp32 per-volume values over the valid volumes (0 without one), and the mean of those."""
    means, used = [], []
    for r in range(vals.shape[1]):
        v = [float(vals[i, r]) for i in range(vals.shape[0]) if valid[i, r]]
        means.append(sum(v) / len(v) if v else 0.0)
        used.append(bool(v))
    ok = [m for m, u in zip(means, used) if u]
    return means, (sum(ok) / max(1, len(ok)))


def _expected_metrics(strat, raw_masks, labels):
    """raw masks uint8 [V,R,D,H,W] + labels -> filtered masks and every key the filter moves or adds, from scipy."""
    from multimodal_tta_amd import ops
    _, filt, counts, stats = oracle(raw_masks, labels, PP["connectivity"], PP["min_voxels"], PP["keep_largest"])
    c = torch.from_numpy(counts).to(torch.float32)
    inter, ps, gs = c[..., 0], c[..., 1], c[..., 2]
    valid = (gs > 0).numpy()
    dice = ((2.0 * inter + EPS) / (ps + gs + EPS)).numpy()
    iou = ((inter + EPS) / (ps + gs - inter + EPS)).numpy()
    want = {}
    md, avg = _mean_over_valid(dice, valid)
    want.update({f"{n.lower()}_dc": v for n, v in zip(REGIONS, md)}, avg_dc=avg)
    _, want["miou"] = _mean_over_valid(iou, valid)
    want["jc"] = want["miou"]
    hd, asd = ops.surface_distances(torch.from_numpy(filt).cuda(), torch.from_numpy(labels).cuda(), strat.spacing, 95.0,
                                    strat.asd_symmetric)
    hd, asd = strat.surface_fix(hd, asd, torch.from_numpy(counts), raw_masks.shape[2:])
    for key, val in (("hd95", hd.numpy()), ("asd", asd.numpy())):
        mm, avg = _mean_over_valid(val, valid)
        want.update({f"{n.lower()}_{key}": v for n, v in zip(REGIONS, mm)})
        want[f"avg_{key}"] = avg
    V = raw_masks.shape[0]
    for col, key in enumerate(("components", "kept_components", "removed_voxels")):
        means = [float(np.float64(stats[:, r, col].sum()) / V) for r in range(len(REGIONS))]
        want.update({f"{n.lower()}_{key}": v for n, v in zip(REGIONS, means)})
        if col == 0:
            want["avg_components"] = sum(means) / len(means)
    return filt, want, stats


def _speckle_threshold():
    """An untrained model puts a whole volume on one side of 0.5: one component, nothing to filter.  The median of its own
    probabilities as the threshold cuts through their noise instead, which gives masks of many components."""
    from multimodal_tta_amd.registry import get_dataset_builder
    from test_hip_tta import SMALL, build_pair
    _, hip = build_pair(SMALL)
    hip.eval().to("cuda")
    loader = get_dataset_builder("brats")(_e2e_cfg(None)).get_loader("test")
    with torch.no_grad():
        p = torch.cat([torch.sigmoid(hip(b["image"].cuda()).float()).cpu().reshape(-1) for b in loader])
    return float(p.median())


NEW_KEYS = {f"{p}{r}_{k}" for p in ("", "dom/synth/") for r in ("et", "tc", "wt")
            for k in ("components", "kept_components", "removed_voxels")} | {"avg_components", "dom/synth/avg_components"}


def _check(m_on, m_off, want):
    assert set(m_on) == set(m_off) | NEW_KEYS
    for k, v in want.items():
        assert m_on[k] == v, (k, m_on[k], v)
        assert k == "jc" or m_on[f"dom/synth/{k}"] == v, k            # one domain: the same figures under it
    assert m_on["loss"] == m_off["loss"]                              # the reported loss stays on the logits


def test_seg_tta_eval_filters_its_masks():
    from multimodal_tta_amd.evaluation import table_width
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair

    runs = {}
    thr = _speckle_threshold()
    for name, block in (("on", PP), ("off", {**PP, "enable": False}), ("absent", None)):
        cfg = _e2e_cfg(block, thr, lanes=2, group=2)
        _, hip = build_pair(SMALL)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_tta_eval")(cfg)
        runs[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
    (m_on, s_on), (m_off, s_off), (m_abs, s_abs) = runs["on"], runs["off"], runs["absent"]
    # disabled = no block at all: keys, values, table
    assert m_off == m_abs and list(m_off) == list(m_abs)
    assert torch.equal(s_off.last_table, s_abs.last_table) and s_off.last_table.shape == (3, table_width(3, True))
    assert all(torch.equal(s_off.last_masks[i], s_abs.last_masks[i]) for i in range(3))
    labels = np.concatenate([b["label"].numpy() for b in loader]).astype(np.float32)
    raw = np.stack([s_off.last_masks[i].numpy() for i in range(3)])
    filt, want, stats = _expected_metrics(s_on, raw, labels)
    assert stats[..., 2].sum() > 0, "the filter removed nothing: the case shows nothing"
    for i in range(3):
        assert np.array_equal(s_on.last_masks[i].numpy(), filt[i]), f"volume {i}: gathered mask is not the filtered one"
    _check(m_on, m_off, want)
    # the table: today's columns, then components[R], kept[R], removed[R]
    w0 = table_width(3, True)
    assert s_on.last_table.shape == (3, table_width(3, True, components=True)) and s_on.last_table.shape[1] == w0 + 9
    assert np.array_equal(s_on.last_table[:, w0:].numpy(), stats.transpose(0, 2, 1).reshape(3, 9).astype(np.float64))
    assert torch.equal(s_on.last_table[:, :3], s_off.last_table[:, :3])


def test_seg_eval_filters_its_masks():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair

    _, hip = build_pair(SMALL)
    res = {}
    thr = _speckle_threshold()
    for name, block in (("on", PP), ("off", {**PP, "enable": False}), ("absent", None)):
        cfg = _e2e_cfg(block, thr)
        cfg["training"]["eval_batch_size"] = 2
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_eval")(cfg)
        res[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
    (m_on, s_on), (m_off, _), (m_abs, _) = res["on"], res["off"], res["absent"]
    assert m_off == m_abs and list(m_off) == list(m_abs)
    raw, labels = [], []
    with torch.no_grad():
        for batch in loader:
            y = batch["label"].cuda().float()
            mask = torch.empty(tuple(y.shape), dtype=torch.uint8, device="cuda")
            counts = torch.empty((y.shape[0], 3, 3), dtype=torch.int64, device="cuda")
            ops.mask_dice_counts(hip(batch["image"].cuda()).float(), y, s_on.threshold, counts, mask, logits_channels_last=False)
            raw.append(mask.cpu().numpy())
            labels.append(batch["label"].numpy().astype(np.float32))
    _, want, stats = _expected_metrics(s_on, np.concatenate(raw), np.concatenate(labels))
    assert stats[..., 2].sum() > 0, "the filter removed nothing: the case shows nothing"
    _check(m_on, m_off, want)
