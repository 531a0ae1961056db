"""Lesion-wise HD95 (mmtta_lesionwise_hd95) against scipy, and the evaluators that report it.

The oracle restates lesions and matching as tests/test_hip_lesionwise.py does (binary_dilation, `ndimage.label` with the
26-neighbourhood, `np.isin`); then, per kept lesion with a match, hd_g = oracle.surface.hd_asd(P_g, A_g, spacing, percentile)[0]
with P_g the union of the whole matched components and A_g the lesion's own voxels.  The tolerance on a distance is the one
tests/test_hip_surface.py uses against that oracle, 1e-6 relative + 1e-7; hd_q is compared with sum round(hd_g 2^20) within
that tolerance summed over the lesions.  Counts are integers and must be equal.  The oracle also adds up, over the
(component, lesion) pairs, the component's edge voxels: every case but the overflow case stays within 2 V.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q20 = 1 << 20
RTOL, ATOL = 1e-6, 1e-7
SHAPES = [(9, 17, 40), (12, 20, 33), (5, 9, 70)]
# (iterations, dilation connectivity, spacing)
SETTINGS = [(0, 6, (1.0, 1.0, 1.0)), (1, 18, (1.5, 0.8, 2.0)), (3, 26, (1.5, 0.8, 2.0)), (3, 18, (1.0, 1.0, 1.0))]
N, R = 2, 3
MIN_LESION = [0, 5, 1]
_id = lambda s: "x".join(map(str, s))


# ----------------------------------------------------------------------------- the scipy oracle
def oracle_one(P, G, iterations, conn, min_voxels, spacing, percentile):
    """P, G bool [D,H,W] -> (kept, found, {root index of the lesion: hd_g}, sum over pairs of the component's edge voxels)."""
    from scipy import ndimage
    from oracle.surface import hd_asd, mask_edges
    s26 = ndimage.generate_binary_structure(3, 3)
    Gd = G.copy()
    if iterations > 0:
        Gd = ndimage.binary_dilation(G, ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]), iterations)
    lg, ng = ndimage.label(Gd, structure=s26)
    lp, _ = ndimage.label(P, structure=s26)
    kept = found = pool = 0
    hd = {}
    for g in range(1, ng + 1):
        comp = lg == g
        own = G & comp
        ids = np.unique(lp[comp])
        ids = ids[ids > 0]
        if int(own.sum()) < min_voxels:
            continue
        kept += 1
        if ids.size:
            found += 1
            Pg = np.isin(lp, ids)
            pool += int(mask_edges(Pg).sum())       # = the sum of the matched components' edge voxels
            hd[int(np.flatnonzero(comp)[0])] = hd_asd(Pg, own, spacing, percentile)[0]
    return kept, found, hd, pool


def run(mask, label, it, conn, minv, spacing, percentile=95.0, **kw):
    from multimodal_tta_amd import ops
    m = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    keep = m.clone()
    res = ops.lesionwise_hd95(m, torch.from_numpy(np.ascontiguousarray(label)).cuda(), it, conn, minv, spacing, percentile,
                              want_lesion_hd=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(m, keep), "the input mask was written"
    assert res["hd_stats"].dtype == torch.int64 and tuple(res["hd_stats"].shape) == mask.shape[:2] + (3,)
    assert res["lesion_hd"].dtype == torch.float32 and tuple(res["lesion_hd"].shape) == mask.shape
    return res


def check(mask, label, it, conn, minv, spacing, percentile=95.0, what=""):
    """Run, compare everything with the oracle; -> (res, per (n, r) the oracle's {root: hd})."""
    from multimodal_tta_amd import ops
    res = run(mask, label, it, conn, minv, spacing, percentile)
    alone = ops.lesionwise_scores(torch.from_numpy(mask).cuda(), torch.from_numpy(label).cuda(), it, conn, minv)["stats"]
    assert torch.equal(res["stats"], alone), f"{what}: stats differ from ops.lesionwise_scores"
    stats, hd_stats, lesion_hd = res["stats"].cpu().numpy(), res["hd_stats"].cpu().numpy(), res["lesion_hd"].cpu().numpy()
    mv = [minv] * mask.shape[1] if isinstance(minv, int) else list(minv)
    V = int(np.prod(mask.shape[2:]))
    wants = {}
    for n in range(mask.shape[0]):
        for r in range(mask.shape[1]):
            kept, found, hd, pool = oracle_one(mask[n, r] != 0, label[n, r] > 0.5, it, conn, mv[r], spacing, percentile)
            assert pool <= 2 * V, f"{what}: the case itself is beyond the pool ({pool} > 2 * {V})"
            wants[n, r] = hd
            got = lesion_hd[n, r].ravel()
            at = np.flatnonzero(~np.isnan(got))
            print(what, (n, r), "scored", hd_stats[n, r].tolist(), "got", {int(i): float(got[i]) for i in at}, "want", hd)
            assert stats[n, r, 1] == kept and stats[n, r, 2] == found
            assert hd_stats[n, r, 1] == found == len(hd) and hd_stats[n, r, 2] == 0, f"{what} {(n, r)}: {hd_stats[n, r]} vs {found}"
            assert sorted(at.tolist()) == sorted(hd), f"{what} {(n, r)}: scored lesions {at.tolist()} vs {sorted(hd)}"
            tol = 0.0
            for root, want in hd.items():
                assert np.isfinite(want)
                assert abs(float(got[root]) - want) <= RTOL * abs(want) + ATOL, f"{what} {(n, r)} lesion {root}: {got[root]} vs {want}"
                tol += RTOL * abs(want) + ATOL
            want_q = sum(int(round(v * Q20)) for v in hd.values())
            assert abs(int(hd_stats[n, r, 0]) - want_q) <= tol * Q20, f"{what} {(n, r)}: hd_q {hd_stats[n, r, 0]} vs {want_q}"
    return res, wants


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
def random_case(shape):
    """G: about 5 balls of radius <= 3.  P: G thinned at 0.8, plus about 3 spurious balls, plus 0.3 % speckle."""
    rng = np.random.default_rng(91 + sum(shape))
    mask = np.zeros((N, R) + shape, dtype=np.uint8)
    label = np.zeros((N, R) + shape, dtype=np.float32)
    for n in range(N):
        for r in range(R):
            G = _balls(rng, shape, 5, 3.0)
            P = (G & (rng.random(shape) < 0.8)) | _balls(rng, shape, 3, 3.0) | (rng.random(shape) < 0.003)
            mask[n, r], label[n, r] = P, G
    mask.setflags(write=False)
    label.setflags(write=False)
    return mask, label


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"{s[0]}x{s[1]}-{'iso' if s[2][0] == 1.0 else 'aniso'}")
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_random_blobs_match_scipy(shape, setting):
    mask, label = random_case(shape)
    it, conn, spacing = setting
    _, wants = check(mask, label, it, conn, MIN_LESION, spacing, what=f"random {shape}")
    assert sum(len(w) for w in wants.values()) >= 3, "hardly a lesion scored: the case shows nothing"


@pytest.mark.parametrize("percentile", [100.0, 0.0, 50.0])
def test_percentiles(percentile):
    mask, label = random_case(SHAPES[0])
    check(mask, label, 1, 18, MIN_LESION, (1.5, 0.8, 2.0), percentile, what=f"percentile {percentile}")


# ----------------------------------------------------------------------------- structured cases
SSHAPE = (20, 24, 48)
E = lambda: np.zeros(SSHAPE, dtype=bool)


def _grid():
    return np.meshgrid(np.arange(SSHAPE[0]), np.arange(SSHAPE[1]), np.arange(SSHAPE[2]), indexing="ij")


def _one(P, G):
    return P[None, None].astype(np.uint8), G[None, None].astype(np.float32)


def _hd_of(res):
    got = res["lesion_hd"].cpu().numpy().ravel()
    return {int(i): got[i] for i in np.flatnonzero(~np.isnan(got))}


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (1.5, 0.8, 2.0)], ids=["iso", "aniso"])
def test_one_lesion_one_component_is_the_region_hd(spacing):
    from multimodal_tta_amd import ops
    z, y, x = _grid()
    G = (z - 9) ** 2 + (y - 11) ** 2 + (x - 20) ** 2 <= 30
    P = (z - 10) ** 2 + (y - 13) ** 2 + (x - 24) ** 2 <= 22
    mask, label = _one(P, G)
    res, _ = check(mask, label, 3, 18, 0, spacing, what="touching")
    (hd_g,) = _hd_of(res).values()
    hd, _ = ops.surface_distances(torch.from_numpy(mask).cuda(), torch.from_numpy(label).cuda(), spacing, 95.0)
    hd = float(hd.cpu()[0, 0])
    print("one lesion, one component: lesion-wise", float(hd_g), "region", hd, "bit-equal", float(hd_g) == hd)
    assert abs(float(hd_g) - hd) <= RTOL * abs(hd) + ATOL


def test_component_bridging_two_lesions_counts_for_each():
    from oracle.surface import hd_asd
    P, G = E(), E()
    G[8:11, 10:13, 6:9] = True
    G[8:11, 10:13, 38:41] = True
    P[9, 11, 7:40] = True
    mask, label = _one(P, G)
    res, wants = check(mask, label, 2, 18, 0, (1.0, 1.0, 1.0), what="bridge")
    assert res["stats"].cpu()[0, 0, :5].tolist() == [2, 2, 2, 1, 1]
    hds = _hd_of(res)
    assert len(hds) == 2
    whole = hd_asd(P, G, (1.0, 1.0, 1.0), 95.0)[0]
    assert all(v > whole + 5.0 for v in hds.values()), (hds, whole)     # each lesion sees the whole bar, its far end too


def test_nearest_surface_of_an_unmatched_component_is_ignored():
    from oracle.surface import hd_asd
    P, G = E(), E()
    G[8:12, 8:12, 10:22] = True          # one long lesion
    P[8:12, 8:12, 10:13] = True          # matched at its left end
    P[8:12, 8:12, 26:29] = True          # beyond the dilated lesion at its right end: unmatched, a false positive
    mask, label = _one(P, G)
    res, wants = check(mask, label, 1, 18, 0, (1.0, 1.0, 1.0), what="unmatched neighbour")
    assert res["stats"].cpu()[0, 0, :5].tolist() == [1, 1, 1, 2, 1]
    (hd_g,) = _hd_of(res).values()
    whole = hd_asd(P, G, (1.0, 1.0, 1.0), 95.0)[0]
    assert float(hd_g) > whole + 1.0, (hd_g, whole)     # a distance transform of the whole mask would stop at the false positive


def test_small_unmatched_and_false_positive_are_not_scored():
    P, G = E(), E()
    G[3:6, 3:6, 3:6] = True              # scored
    P[4:7, 3:6, 3:6] = True
    G[15, 20, 40:42] = True              # 2 voxels: below min_lesion_voxels, though matched
    P[15, 20, 40:44] = True
    G[14:17, 4:7, 30:33] = True          # kept, no match
    P[3:5, 18:20, 20:22] = True          # false positive
    mask, label = _one(P, G)
    res, wants = check(mask, label, 1, 18, 3, (1.0, 1.0, 1.0), what="mixed")
    assert res["stats"].cpu()[0, 0, :5].tolist() == [3, 2, 1, 3, 2]
    assert res["hd_stats"].cpu()[0, 0].tolist()[1:] == [1, 0]
    assert len(_hd_of(res)) == 1


def test_single_voxels_are_exact():
    spacing = (1.5, 0.8, 2.0)
    P, G = E(), E()
    G[3, 4, 5] = True
    P[4, 6, 5] = True
    res = run(*_one(P, G), 3, 26, 0, spacing)
    want = np.float32(np.sqrt((1 * 1.5) ** 2 + (2 * 0.8) ** 2))
    (hd_g,) = _hd_of(res).values()
    assert hd_g == want, (hd_g, want)
    assert res["hd_stats"].cpu()[0, 0].tolist() == [int(round(float(want) * Q20)), 1, 0]


def test_identical_masks_give_zero():
    mask, label = random_case(SHAPES[1])
    same = (label > 0.5).astype(np.uint8)
    res, wants = check(same, label, 0, 6, 0, (1.5, 0.8, 2.0), what="identical")
    hs = res["hd_stats"].cpu()
    assert int(hs[..., 0].abs().sum()) == 0 and int(hs[..., 1].sum()) == int(res["stats"].cpu()[..., 0].sum()) > 0
    assert all(v == 0.0 for v in _hd_of(res).values())


# ----------------------------------------------------------------------------- invariance
def _bits(res):
    return res["hd_stats"].cpu(), res["lesion_hd"].cpu().view(torch.int32), res["stats"].cpu()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_batch_repeat_stream_and_strided_label():
    from multimodal_tta_amd import ops
    shape, spacing = SHAPES[0], (1.5, 0.8, 2.0)
    mask, label = random_case(shape)
    a = _bits(run(mask, label, 3, 18, MIN_LESION, spacing))
    assert _same(a, _bits(run(mask, label, 3, 18, MIN_LESION, spacing))), "two calls differ"
    for n in range(N):
        one = _bits(run(mask[n:n + 1], label[n:n + 1], 3, 18, MIN_LESION, spacing))
        assert _same([t[n:n + 1] for t in a], one), f"item {n} alone differs"
    m = torch.from_numpy(mask).cuda()
    wide = torch.zeros((N, R) + shape[:2] + (shape[2] + 3,), device="cuda")
    wide[..., :shape[2]] = torch.from_numpy(label).cuda()
    res = ops.lesionwise_hd95(m, wide[..., :shape[2]], 3, 18, MIN_LESION, spacing, want_lesion_hd=True)
    assert _same(a, _bits(res)), "a strided label differs"
    res = ops.lesionwise_hd95(m, torch.from_numpy(label).cuda(), 3, 18, MIN_LESION, spacing, want_labels=True)
    assert res["lesion_hd"] is None and torch.equal(res["hd_stats"].cpu(), a[0])
    assert torch.equal(res["labels"], ops.lesionwise_scores(m, torch.from_numpy(label).cuda(), 3, 18, MIN_LESION, want_labels=True)["labels"])
    lab = torch.from_numpy(label).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res = ops.lesionwise_hd95(m, lab, 3, 18, MIN_LESION, spacing, want_lesion_hd=True)
    s.synchronize()
    assert _same(a, _bits(res)), "a side stream differs"


def test_overflow_is_counted_and_leaves_the_batch_alone():
    shape, spacing = SHAPES[0], (1.0, 1.0, 1.0)
    D, H, W = shape
    V = D * H * W
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    board = (z + y + x) % 2 == 0          # one 26-connected component, every voxel an edge voxel
    G = np.zeros(shape, dtype=bool)
    spots = [(0, 0, 0), (4, 4, 4), (8, 16, 38), (2, 10, 20), (6, 2, 30), (4, 12, 12)]
    for s in spots:
        assert sum(s) % 2 == 0
        G[s] = True
    assert 6 * int(board.sum()) > 2 * V
    rmask, rlabel = random_case(shape)
    mask = np.stack([board.astype(np.uint8)[None], rmask[0, :1]])
    label = np.stack([G.astype(np.float32)[None], rlabel[0, :1]])
    res = run(mask, label, 0, 18, 0, spacing)
    hs = res["hd_stats"].cpu()
    print("overflow", hs.tolist(), res["stats"].cpu().tolist())
    assert res["stats"].cpu()[0, 0, :5].tolist() == [6, 6, 6, 1, 1]
    assert int(hs[0, 0, 2]) > 0 and hs[0, 0, :2].tolist() == [0, 0]
    assert bool(torch.isnan(res["lesion_hd"][0]).all())
    alone = run(mask[1:], label[1:], 0, 18, 0, spacing)
    assert _same([t[1:] for t in _bits(res)], _bits(alone)), "the ordinary mask beside the overflowing one differs from itself alone"
    assert int(alone["hd_stats"].cpu()[0, 0, 2]) == 0 and int(alone["hd_stats"].cpu()[0, 0, 1]) > 0


def test_ops_rejects_bad_arguments():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    m = torch.zeros((1, 2, 4, 4, 4), dtype=torch.uint8, device="cuda")
    lab = torch.zeros((1, 2, 4, 4, 4), device="cuda")
    with pytest.raises(MmttaError, match="uint8"):
        ops.lesionwise_hd95(m.float(), lab)
    with pytest.raises(MmttaError, match="label"):
        ops.lesionwise_hd95(m, lab.double())
    with pytest.raises(MmttaError, match="iterations"):
        ops.lesionwise_hd95(m, lab, 9)
    with pytest.raises(MmttaError, match="min_lesion_voxels"):
        ops.lesionwise_hd95(m, lab, 3, 18, -1)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, float("inf"), 1.0), (1.0, float("nan"), 1.0), "abc"):
        with pytest.raises(MmttaError, match="spacing"):
            ops.lesionwise_hd95(m, lab, spacing=bad)
    for bad in (-1.0, 100.5, float("nan"), "95", True):
        with pytest.raises(MmttaError, match="percentile"):
            ops.lesionwise_hd95(m, lab, percentile=bad)
    with pytest.raises(MmttaError, match="1024"):
        ops.lesionwise_hd95(torch.zeros((1, 1, 1, 1, 1025), dtype=torch.uint8, device="cuda"), torch.zeros((1, 1, 1, 1, 1025), device="cuda"))
    res = ops.lesionwise_hd95(m, lab)
    assert res["lesion_hd"] is None and res["labels"] is None and int(res["hd_stats"].abs().sum()) == 0
    assert ops.LESIONWISE_HD_Q_ONE == Q20
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- evaluators
REGIONS = ["ET", "TC", "WT"]
LW = {"enable": True, "dilation": 2, "dilation_connectivity": 18, "min_lesion_voxels": [0, 3, 1]}
SPACING = [1.5, 0.8, 2.0]


def _e2e_cfg(hd95, threshold, **method):
    from test_hip_lesionwise import _e2e_cfg as base
    cfg = base(LW, threshold, None, **method)
    cfg["evaluation"]["seg"]["spacing"] = list(SPACING)
    if hd95 is not None:
        cfg["evaluation"]["lesionwise"]["hd95"] = dict(hd95)
    return cfg


def expected_keys(masks, labels, penalty, domain="synth"):
    """The lesion-wise HD95 keys of the scored masks uint8 [V,R,D,H,W], overall and under dom/<domain>/ (one domain)."""
    from oracle.surface import diag_mm
    from test_hip_lesionwise import oracle as lw_oracle
    stats, _ = lw_oracle(masks, labels, LW["dilation"], LW["dilation_connectivity"], LW["min_lesion_voxels"])
    pen = diag_mm(*masks.shape[2:], SPACING) if penalty == "diagonal" else float(penalty)
    V = masks.shape[0]
    want, means, used = {}, [], []
    scored = 0
    for r, name in enumerate(REGIONS):
        vals, over = [], 0
        for i in range(V):
            kept, found, hd, pool = oracle_one(masks[i, r] != 0, labels[i, r] > 0.5, LW["dilation"], LW["dilation_connectivity"],
                                               LW["min_lesion_voxels"][r], SPACING, 95.0)
            fp = int(stats[i, r, 3] - stats[i, r, 4])
            if pool > 2 * masks[i, r].size:       # beyond the pool: left out of the mean and counted
                over += 1
                continue
            scored += len(hd)
            if kept + fp > 0:
                vals.append((sum(int(round(v * Q20)) for v in hd.values()) / Q20 + pen * ((kept - found) + fp)) / (kept + fp))
        want[f"{name.lower()}_lw_hd95"] = sum(vals) / len(vals) if vals else 0.0
        want[f"{name.lower()}_lw_hd95_overflow"] = over / V
        means.append(want[f"{name.lower()}_lw_hd95"])
        used.append(bool(vals))
    ok = [m for m, u in zip(means, used) if u]
    want["avg_lw_hd95"] = sum(ok) / max(1, len(ok))
    want.update({f"dom/{domain}/{k}": v for k, v in list(want.items())})
    assert scored > 0, "no lesion scored: the case shows nothing"
    return want


def _check_e2e(m_on, m_off, want):
    assert set(m_on) == set(m_off) | set(want), sorted(set(m_on) ^ (set(m_off) | set(want)))
    for k, v in want.items():
        assert m_on[k] == pytest.approx(v, rel=RTOL, abs=ATOL), (k, m_on[k], v)
    for k, v in m_off.items():
        assert m_on[k] == v, f"pre-existing key {k} moved: {m_on[k]} vs {v}"


def _count_calls(monkeypatch):
    from multimodal_tta_amd import ops
    calls = []
    real = ops.lesionwise_hd95
    monkeypatch.setattr(ops, "lesionwise_hd95", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_seg_tta_eval_reports_lesionwise_hd95(monkeypatch):
    from multimodal_tta_amd.evaluation import table_width
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_lesionwise import _speckle_threshold
    from test_hip_tta import SMALL, build_pair

    thr = _speckle_threshold()
    calls = _count_calls(monkeypatch)
    runs = {}
    for name, hd in (("absent", None), ("off", {"enable": False, "penalty": 374}), ("diagonal", {"enable": True}),
                     ("374", {"enable": True, "penalty": 374, "percentile": 95.0})):
        cfg = _e2e_cfg(hd, thr, lanes=2, group=2)
        _, hip = build_pair(SMALL)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_tta_eval")(cfg)
        runs[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
        if name == "off":
            assert not calls, "ops.lesionwise_hd95 ran with the block absent or off"
    assert calls
    labels = np.concatenate([b["label"].numpy() for b in loader]).astype(np.float32)
    (m_abs, s_abs), (m_off, s_off) = runs["absent"], runs["off"]
    assert m_off == m_abs and list(m_off) == list(m_abs) and torch.equal(s_off.last_table, s_abs.last_table)
    assert s_off.last_table.shape == (3, table_width(3, lesionwise=True))
    for name in ("diagonal", "374"):
        m_on, s_on = runs[name]
        scored = np.stack([s_on.last_masks[i].numpy() for i in range(3)])
        assert np.array_equal(scored, np.stack([s_off.last_masks[i].numpy() for i in range(3)]))
        _check_e2e(m_on, m_off, expected_keys(scored, labels, name if name == "diagonal" else 374))
        assert s_on.last_table.shape == (3, table_width(3, lesionwise=True, lesionwise_hd95=True))
        assert torch.equal(s_on.last_table[:, :table_width(3, lesionwise=True)], s_off.last_table)
    assert runs["diagonal"][0]["avg_lw_hd95"] != runs["374"][0]["avg_lw_hd95"]


def test_seg_eval_reports_lesionwise_hd95(monkeypatch):
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_lesionwise import _speckle_threshold
    from test_hip_tta import SMALL, build_pair

    _, hip = build_pair(SMALL)
    thr = _speckle_threshold()
    calls = _count_calls(monkeypatch)
    res = {}
    for name, hd in (("absent", None), ("off", {"enable": False}), ("diagonal", {"enable": True, "penalty": "diagonal"}),
                     ("374", {"enable": True, "penalty": 374})):
        cfg = _e2e_cfg(hd, thr)
        cfg["training"]["eval_batch_size"] = 2
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_eval")(cfg)
        res[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
        if name == "off":
            assert not calls, "ops.lesionwise_hd95 ran with the block absent or off"
    assert calls
    m_abs, m_off = res["absent"][0], res["off"][0]
    assert m_off == m_abs and list(m_off) == list(m_abs)
    raw, labels = [], []
    with torch.no_grad():
        for batch in loader:
            y = batch["label"].cuda().float()
            mask = torch.empty(tuple(y.shape), dtype=torch.uint8, device="cuda")
            counts = torch.empty((y.shape[0], 3, 3), dtype=torch.int64, device="cuda")
            ops.mask_dice_counts(hip(batch["image"].cuda()).float(), y, res["off"][1].threshold, counts, mask, logits_channels_last=False)
            raw.append(mask.cpu().numpy())
            labels.append(batch["label"].numpy().astype(np.float32))
    raw, labels = np.concatenate(raw), np.concatenate(labels)
    for name in ("diagonal", "374"):
        _check_e2e(res[name][0], m_off, expected_keys(raw, labels, name if name == "diagonal" else 374))
