"""Lesion-wise scores (mmtta_lesionwise_scores) against a scipy restatement of their definition, and the evaluators that
report them.

The oracle, per (volume, region): Gd = scipy.ndimage.binary_dilation(G, generate_binary_structure(3, 1 | 2 | 3), iterations)
(Gd = G for 0 iterations); lesions = the 26-connected components of Gd, predicted components = those of P
(`scipy.ndimage.label` with `generate_binary_structure(3, 3)`); a component is matched to lesion g iff it has a voxel in
component g of Gd (`np.isin`); per kept lesion q_g = (2 inter 2^30 + den // 2) // den in Python integers.  The seven figures
and the lesion labels are integers and must be exactly equal: there is no tolerance anywhere in this file.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(17, 33, 70), (9, 20, 48), (1, 1, 5), (3, 1, 1), (40, 40, 40)]
SETTINGS = [(3, 18), (1, 6), (0, 18), (2, 26)]          # (iterations, dilation connectivity)
MIN_LESION = [0, 5, 1]
N, R = 2, 3
Q1 = 1 << 30
_id = lambda s: "x".join(map(str, s))
COLS = ("lesions", "lesions_kept", "lesions_found", "pred_components", "matched_components", "dice_q", "fp_voxels")


# ----------------------------------------------------------------------------- the scipy oracle
def _canonical(lab, n):
    """scipy labels -> 1 + the smallest linear index of the component (0 background)."""
    flat = lab.ravel()
    if n == 0:
        return np.zeros(lab.shape, dtype=np.int32)
    ids, first = np.unique(flat, return_index=True)
    lut = np.zeros(n + 1, dtype=np.int64)
    lut[ids[ids > 0]] = first[ids > 0] + 1
    return lut[flat].astype(np.int32).reshape(lab.shape)


def oracle_one(P, G, iterations, conn, min_voxels):
    """P, G bool [D,H,W] -> (the seven figures as Python ints, lesion labels int32 on the voxels of G)."""
    from scipy import ndimage
    s26 = ndimage.generate_binary_structure(3, 3)
    Gd = G.copy()
    if iterations > 0:      # (scipy reads iterations < 1 as "until nothing changes")
        Gd = ndimage.binary_dilation(G, ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]), iterations)
    lg, ng = ndimage.label(Gd, structure=s26)
    lp, npc = ndimage.label(P, structure=s26)
    sizes = np.bincount(lp.ravel(), minlength=npc + 1)
    labels = np.where(G, _canonical(lg, ng), 0).astype(np.int32)
    matched = np.zeros(npc + 1, dtype=bool)
    kept = found = dice_q = 0
    for g in range(1, ng + 1):
        comp = lg == g
        own = G & comp
        n_own = int(own.sum())
        ids = np.unique(lp[comp])
        ids = ids[ids > 0]
        matched[ids] = True
        if n_own < min_voxels:
            continue
        kept += 1
        if ids.size:
            found += 1
            Pg = np.isin(lp, ids)
            inter, den = int((Pg & own).sum()), int(Pg.sum()) + n_own
            dice_q += (2 * inter * Q1 + den // 2) // den
    fp_voxels = int(sizes[1:][~matched[1:]].sum())
    return [ng, kept, found, npc, int(matched[1:].sum()), dice_q, fp_voxels], labels


def oracle(mask, label, iterations, conn, min_voxels):
    """mask uint8 [N,R,D,H,W], label float32 -> stats int64 [N,R,7], labels int32 [N,R,D,H,W]."""
    n_, r_ = mask.shape[:2]
    stats = np.zeros((n_, r_, 7), dtype=np.int64)
    labels = np.zeros(mask.shape, dtype=np.int32)
    for n in range(n_):
        for r in range(r_):
            stats[n, r], labels[n, r] = oracle_one(mask[n, r] != 0, label[n, r] > 0.5, iterations, conn, min_voxels[r])
    return stats, labels


def run(mask, label, iterations, conn, min_voxels, want_labels=True):
    from multimodal_tta_amd import ops
    m = torch.from_numpy(mask).cuda()
    keep = m.clone()
    res = ops.lesionwise_scores(m, torch.from_numpy(label).cuda(), iterations, conn, min_voxels, want_labels=want_labels)
    torch.cuda.synchronize()
    assert torch.equal(m, keep), "the input mask was written"
    assert res["stats"].dtype == torch.int64 and tuple(res["stats"].shape) == mask.shape[:2] + (7,)
    return res["stats"].cpu().numpy(), (res["labels"].cpu().numpy() if res["labels"] is not None else None)


def check(mask, label, iterations, conn, min_voxels, what):
    stats, labels = run(mask, label, iterations, conn, min_voxels)
    want_stats, want_labels = oracle(mask, label, iterations, conn, min_voxels)
    print(what, iterations, conn, "got", stats.reshape(-1, 7).tolist(), "want", want_stats.reshape(-1, 7).tolist())
    assert np.array_equal(stats, want_stats), f"{what} ({iterations} x {conn}): stats {COLS}\n{stats}\n{want_stats}"
    assert labels.dtype == np.int32 and np.array_equal(labels, want_labels), f"{what} ({iterations} x {conn}): lesion labels"
    return want_stats


# ----------------------------------------------------------------------------- random blobs
def _balls(rng, shape, count, rmax):
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros(shape, dtype=bool)
    for _ in range(count):
        c = [rng.integers(0, e) for e in shape]
        rad = rng.uniform(0.5, rmax)
        out |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= rad * rad
    return out


@functools.lru_cache(maxsize=None)
def random_case(shape, seed=0):
    """G: about 8 balls of radius <= 3.5.  P: G thinned at 0.8, plus about 6 spurious balls, plus 0.3 % speckle."""
    rng = np.random.default_rng(77 * seed + sum(shape))
    mask = np.zeros((N, R) + shape, dtype=np.uint8)
    label = np.zeros((N, R) + shape, dtype=np.float32)
    for n in range(N):
        for r in range(R):
            G = _balls(rng, shape, 8, 3.5)
            P = (G & (rng.random(shape) < 0.8)) | _balls(rng, shape, 6, 3.5) | (rng.random(shape) < 0.003)
            mask[n, r], label[n, r] = P, G
    mask.setflags(write=False)
    label.setflags(write=False)
    return mask, label


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_random_blobs_match_scipy(shape, setting):
    mask, label = random_case(shape)
    want = check(mask, label, setting[0], setting[1], MIN_LESION, f"random {shape}")
    if shape == (17, 33, 70) and setting == (3, 18):
        assert want[..., 0].max() > 1 and want[..., 3].sum() > want[..., 4].sum()      # several lesions, unmatched components


# ----------------------------------------------------------------------------- structured cases
SSHAPE = (17, 33, 70)


def _structured():
    """name -> (P, G) bool [D,H,W] on SSHAPE."""
    D, H, W = SSHAPE
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    E = lambda: np.zeros(SSHAPE, dtype=bool)
    cases = {}
    # one predicted bar joining two blobs farther apart than twice any dilation: one component, counted for both lesions
    P, G = E(), E()
    G[7:10, 15:18, 8:11] = True
    G[7:10, 15:18, 55:58] = True
    P[8, 16, 9:57] = True
    cases["bar"] = (P, G)
    # two blobs with 2 it and 2 it + 1 empty voxels between them along x, for it = 1, 2, 3: merged / not merged
    for it in (1, 2, 3):
        for extra in (0, 1):
            P, G = E(), E()
            gap = 2 * it + extra
            G[8, 16, 20:22] = True
            G[8, 16, 22 + gap:24 + gap] = True
            P[8, 16, 21] = True
            cases[f"axis-gap-{gap}"] = (P, G)
    # ... and along the face and the space diagonal
    for k in (2, 3, 4, 5, 6, 7, 8):
        P, G = E(), E()
        G[4, 10, 20] = True
        G[4, 10 + k, 20 + k] = True
        G[12, 4, 40] = True
        if 12 + k < D:
            G[12 + k, 4 + k, 40 + k] = True
        else:
            G[12 - k, 4 + k, 40 + k] = True
        P[4, 10, 20] = True
        cases[f"diagonal-{k}"] = (P, G)
    # lesions in the corners of the volume
    P, G = E(), E()
    G[0, 0, 0] = True
    G[D - 2:, H - 2:, W - 2:] = True
    P[0:2, 0:2, 0:2] = True
    P[D - 1, H - 1, W - 1] = True
    cases["corners"] = (P, G)
    # a predicted voxel inside the dilated ring, outside G: matched, intersection 0
    P, G = E(), E()
    G[6:9, 14:17, 30:33] = True
    P[7, 15, 34] = True
    cases["ring"] = (P, G)
    ones = np.ones(SSHAPE, dtype=bool)
    cases["p-empty"] = (E(), G.copy())
    cases["g-empty"] = (G.copy(), E())
    cases["both-empty"] = (E(), E())
    cases["both-full"] = (ones, ones)
    # a checkerboard over one blob: many voxels of one component, one pair
    G = (z - 8) ** 2 + (y - 16) ** 2 + (x - 30) ** 2 <= 36
    P = ((z + y + x) % 2 == 0) & ((z - 8) ** 2 + (y - 16) ** 2 + (x - 30) ** 2 <= 64)
    cases["checkerboard"] = (P, G)
    # isolated predicted voxels at stride 3 over one large lesion: as many pairs as components
    G = E()
    G[1:16, 2:31, 3:66] = True
    P = (z % 3 == 0) & (y % 3 == 0) & (x % 3 == 0)
    cases["stride-3"] = (P, G)
    # ... at stride 2, the densest set of isolated voxels there is, over two lesions and the background
    G = E()
    G[:, :, :30] = True
    G[:, :, 45:] = True
    P = (z % 2 == 0) & (y % 2 == 0) & (x % 2 == 0)
    cases["stride-2"] = (P, G)
    return cases


@functools.lru_cache(maxsize=None)
def structured_batch():
    cases = _structured()
    names = list(cases)
    n_ = (len(names) + R - 1) // R
    mask = np.zeros((n_, R) + SSHAPE, dtype=np.uint8)
    label = np.zeros((n_, R) + SSHAPE, dtype=np.float32)
    for i, name in enumerate(names):
        mask[i // R, i % R], label[i // R, i % R] = cases[name]
    return names, mask, label


@pytest.mark.parametrize("setting", SETTINGS + [(3, 6), (3, 26), (1, 18), (8, 26)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_structured_cases_match_scipy(setting):
    names, mask, label = structured_batch()
    it, conn = setting
    want = check(mask, label, it, conn, [0, 0, 0], "structured")
    row = {name: want[i // R, i % R].tolist() for i, name in enumerate(names)}
    if it <= 3:
        assert row["bar"][:5] == [2, 2, 2, 1, 1]                        # one component, found for both lesions
    if 1 <= it <= 3:
        assert row[f"axis-gap-{2 * it}"][0] == 1 and row[f"axis-gap-{2 * it + 1}"][0] == 2      # merged / not merged
    if it >= 2:
        assert row["ring"] == [1, 1, 1, 1, 1, 0, 0]                     # matched with intersection 0: Dice 0, no false positive
    else:
        assert row["ring"] == [1, 1, 0, 1, 0, 0, 1]
    assert row["p-empty"] == [1, 1, 0, 0, 0, 0, 0]
    assert row["g-empty"] == [0, 0, 0, 1, 0, 0, 27]
    assert row["both-empty"] == [0] * 7
    assert row["both-full"] == [1, 1, 1, 1, 1, Q1, 0]
    assert row["checkerboard"][:5] == [1, 1, 1, 1, 1]
    assert row["stride-3"][0] == 1 and row["stride-3"][3] == 6 * 11 * 24 and row["stride-3"][4] > 500
    assert row["stride-2"][3] == 9 * 17 * 35


def test_diagonal_pairs_merge_and_split_for_every_connectivity():
    names, mask, label = structured_batch()
    for conn in (6, 18, 26):
        lesions = set()
        for it in (1, 2):
            want, _ = oracle(mask, label, it, conn, [0, 0, 0])
            lesions |= {int(want[i // R, i % R, 0]) for i, name in enumerate(names) if name.startswith("diagonal-")}
        assert {2, 4} <= lesions, (conn, lesions)      # both pairs merged somewhere, both apart somewhere


# ----------------------------------------------------------------------------- invariance
def test_batch_repeat_stream_and_min_voxels():
    from multimodal_tta_amd import ops
    shape = (17, 33, 70)
    mask, label = random_case(shape)
    a = run(mask, label, 3, 18, MIN_LESION)
    b = run(mask, label, 3, 18, MIN_LESION)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two calls differ"
    for n in range(N):
        one = run(mask[n:n + 1].copy(), label[n:n + 1].copy(), 3, 18, MIN_LESION)
        assert np.array_equal(a[0][n:n + 1], one[0]) and np.array_equal(a[1][n:n + 1], one[1]), f"item {n} alone differs"
    # without the labels; a scalar min_lesion_voxels; a strided label view
    stats, labels = run(mask, label, 3, 18, MIN_LESION, want_labels=False)
    assert labels is None and np.array_equal(stats, a[0])
    assert np.array_equal(run(mask, label, 3, 18, 5)[0], oracle(mask, label, 3, 18, [5, 5, 5])[0])
    wide = torch.zeros((N, R) + shape[:2] + (shape[2] + 3,), device="cuda")
    wide[..., :shape[2]] = torch.from_numpy(label).cuda()
    res = ops.lesionwise_scores(torch.from_numpy(mask).cuda(), wide[..., :shape[2]], 3, 18, MIN_LESION)
    assert np.array_equal(res["stats"].cpu().numpy(), a[0])
    # a side stream
    m, lab = torch.from_numpy(mask).cuda(), torch.from_numpy(label).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = ops.lesionwise_scores(m, lab, 3, 18, MIN_LESION, want_labels=True)
    s.synchronize()
    assert np.array_equal(res["stats"].cpu().numpy(), a[0]) and np.array_equal(res["labels"].cpu().numpy(), a[1])


def test_ops_rejects_bad_arguments():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    m = torch.zeros((1, 2, 4, 4, 4), dtype=torch.uint8, device="cuda")
    lab = torch.zeros((1, 2, 4, 4, 4), device="cuda")
    with pytest.raises(MmttaError, match="uint8"):
        ops.lesionwise_scores(m.float(), lab)
    with pytest.raises(MmttaError, match="label"):
        ops.lesionwise_scores(m, lab.double())
    with pytest.raises(MmttaError, match="iterations"):
        ops.lesionwise_scores(m, lab, 9)
    with pytest.raises(MmttaError, match="connectivity"):
        ops.lesionwise_scores(m, lab, 3, 7)
    with pytest.raises(MmttaError, match="min_lesion_voxels"):
        ops.lesionwise_scores(m, lab, 3, 18, -1)
    with pytest.raises(MmttaError, match="min_lesion_voxels"):
        ops.lesionwise_scores(m, lab, 3, 18, [1, 2, 3])
    with pytest.raises(MmttaError, match="regions"):
        ops.lesionwise_scores(torch.zeros((1, 65, 2, 2, 2), dtype=torch.uint8, device="cuda"), torch.zeros((1, 65, 2, 2, 2), device="cuda"))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- evaluators
REGIONS = ["ET", "TC", "WT"]
LW = {"enable": True, "dilation": 2, "dilation_connectivity": 18, "min_lesion_voxels": [0, 3, 1]}
PP = {"enable": True, "connectivity": 18, "min_voxels": [0, 4, 12], "keep_largest": [True, False, False]}


def _e2e_cfg(lesionwise, threshold, postprocess=None, **method):
    """The small model and loader of the component-filter evaluator tests; `lesionwise`: the block, or None for none."""
    from test_hip_tta import SMALL, root_cfg
    cfg = root_cfg(SMALL, steps=2, lr=1e-3, tune_volumes=4, **method)
    cfg["dataset"]["synthetic"]["num_volumes"] = 3
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    cfg["evaluation"]["gather_masks"] = True
    cfg["evaluation"]["seg"]["threshold"] = float(threshold)
    cfg["evaluation"].pop("postprocess", None)
    cfg["evaluation"].pop("lesionwise", None)
    if postprocess is not None:
        cfg["evaluation"]["postprocess"] = dict(postprocess)
    if lesionwise is not None:
        cfg["evaluation"]["lesionwise"] = dict(lesionwise)
    return cfg


def _speckle_threshold():
    """The median of the untrained model's probabilities: masks of many components (tests/test_hip_components.py)."""
    from multimodal_tta_amd.registry import get_dataset_builder
    from test_hip_tta import SMALL, build_pair
    _, hip = build_pair(SMALL)
    hip.eval().to("cuda")
    loader = get_dataset_builder("brats")(_e2e_cfg(None, 0.5)).get_loader("test")
    with torch.no_grad():
        p = torch.cat([torch.sigmoid(hip(b["image"].cuda()).float()).cpu().reshape(-1) for b in loader])
    return float(p.median())


def expected_keys(stats, domain="synth"):
    """stats int [V,R,7] of the scored masks -> the lesion-wise keys, overall and under dom/<domain>/ (one domain)."""
    V = stats.shape[0]
    want = {}
    means, used = [], []
    for r, name in enumerate(REGIONS):
        name = name.lower()
        vals = []
        for i in range(V):
            _, kept, found, pred, matched, dice_q, _ = (int(v) for v in stats[i, r])
            den = kept + (pred - matched)
            if den > 0:
                vals.append(float(dice_q) / float(Q1) / float(den))
        want[f"{name}_lw_dc"] = sum(vals) / len(vals) if vals else 0.0
        means.append(want[f"{name}_lw_dc"])
        used.append(bool(vals))
        kept, found = int(stats[:, r, 1].sum()), int(stats[:, r, 2].sum())
        pred, matched = int(stats[:, r, 3].sum()), int(stats[:, r, 4].sum())
        want[f"{name}_lesions"] = float(kept) / V
        want[f"{name}_lesions_found"] = float(found) / V
        want[f"{name}_fp_components"] = float(pred - matched) / V
        if kept:
            want[f"{name}_lesion_recall"] = float(found) / float(kept)
        if pred:
            want[f"{name}_lesion_precision"] = float(matched) / float(pred)
    ok = [m for m, u in zip(means, used) if u]
    want["avg_lw_dc"] = sum(ok) / max(1, len(ok))
    want.update({f"dom/{domain}/{k}": v for k, v in list(want.items())})
    return want


def _check_e2e(m_on, m_off, want):
    assert set(m_on) == set(m_off) | set(want), sorted(set(m_on) ^ (set(m_off) | set(want)))
    for k, v in want.items():
        assert m_on[k] == v, (k, m_on[k], v)
    for k, v in m_off.items():
        assert m_on[k] == v, f"pre-existing key {k} moved: {m_on[k]} vs {v}"


def test_seg_tta_eval_reports_lesionwise_scores():
    from multimodal_tta_amd.evaluation import table_width
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair

    thr = _speckle_threshold()
    runs = {}
    for name, lw, pp in (("on", LW, None), ("off", {**LW, "enable": False}, None), ("absent", None, None),
                         ("pp", LW, PP), ("pp_off", None, PP)):
        cfg = _e2e_cfg(lw, thr, pp, lanes=2, group=2)
        _, hip = build_pair(SMALL)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_tta_eval")(cfg)
        runs[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
    labels = np.concatenate([b["label"].numpy() for b in loader]).astype(np.float32)
    (m_on, s_on), (m_off, s_off), (m_abs, s_abs) = runs["on"], runs["off"], runs["absent"]
    assert m_off == m_abs and list(m_off) == list(m_abs) and torch.equal(s_off.last_table, s_abs.last_table)
    assert s_off.last_table.shape == (3, table_width(3))
    # the masks the evaluator scored: the gathered ones
    scored = np.stack([s_on.last_masks[i].numpy() for i in range(3)])
    assert np.array_equal(scored, np.stack([s_off.last_masks[i].numpy() for i in range(3)]))
    stats, _ = oracle(scored, labels, LW["dilation"], LW["dilation_connectivity"], LW["min_lesion_voxels"])
    assert stats[..., 3].sum() > stats[..., 4].sum() > 0, "no matched or no unmatched component: the case shows nothing"
    _check_e2e(m_on, m_off, expected_keys(stats))
    assert s_on.last_table.shape == (3, table_width(3, lesionwise=True))
    assert torch.equal(s_on.last_table[:, :table_width(3)], s_off.last_table)
    # with post-processing the figures describe the filtered mask
    (m_pp, s_pp), (m_ppoff, s_ppoff) = runs["pp"], runs["pp_off"]
    filt = np.stack([s_pp.last_masks[i].numpy() for i in range(3)])
    assert not np.array_equal(filt, scored)
    assert np.array_equal(filt, np.stack([s_ppoff.last_masks[i].numpy() for i in range(3)]))
    stats_pp, _ = oracle(filt, labels, LW["dilation"], LW["dilation_connectivity"], LW["min_lesion_voxels"])
    assert not np.array_equal(stats_pp, stats)
    _check_e2e(m_pp, m_ppoff, expected_keys(stats_pp))


def test_seg_eval_reports_lesionwise_scores():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair

    _, hip = build_pair(SMALL)
    thr = _speckle_threshold()
    res = {}
    for name, lw, pp in (("on", LW, None), ("off", {**LW, "enable": False}, None), ("absent", None, None),
                         ("pp", LW, PP), ("pp_off", None, PP)):
        cfg = _e2e_cfg(lw, thr, pp)
        cfg["training"]["eval_batch_size"] = 2
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_eval")(cfg)
        res[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
    (m_on, s_on), (m_off, _), (m_abs, _) = res["on"], res["off"], res["absent"]
    assert m_off == m_abs and list(m_off) == list(m_abs)
    raw, filt, labels = [], [], []
    with torch.no_grad():
        for batch in loader:
            y = batch["label"].cuda().float()
            mask = torch.empty(tuple(y.shape), dtype=torch.uint8, device="cuda")
            counts = torch.empty((y.shape[0], 3, 3), dtype=torch.int64, device="cuda")
            ops.mask_dice_counts(hip(batch["image"].cuda()).float(), y, s_on.threshold, counts, mask, logits_channels_last=False)
            raw.append(mask.cpu().numpy())
            filt.append(ops.components_filter(mask, y, PP["connectivity"], PP["min_voxels"], PP["keep_largest"])["mask"].cpu().numpy())
            labels.append(batch["label"].numpy().astype(np.float32))
    raw, filt, labels = np.concatenate(raw), np.concatenate(filt), np.concatenate(labels)
    stats, _ = oracle(raw, labels, LW["dilation"], LW["dilation_connectivity"], LW["min_lesion_voxels"])
    assert stats[..., 3].sum() > stats[..., 4].sum() > 0, "no matched or no unmatched component: the case shows nothing"
    _check_e2e(m_on, m_off, expected_keys(stats))
    stats_pp, _ = oracle(filt, labels, LW["dilation"], LW["dilation_connectivity"], LW["min_lesion_voxels"])
    assert not np.array_equal(stats_pp, stats)
    _check_e2e(res["pp"][0], res["pp_off"][0], expected_keys(stats_pp))


def test_softmax_head_is_refused():
    from multimodal_tta_amd.registry import get_evaluation_strategy
    cfg = _e2e_cfg(LW, 0.5)
    cfg["training"]["criterion"] = dict(cfg["training"].get("criterion", {}) or {}, softmax=True)
    with pytest.raises(NotImplementedError, match=r"evaluation\.lesionwise"):
        get_evaluation_strategy("seg_eval")(cfg)
