"""Normalised surface Dice, region-wise (mmtta_surface_dice) and lesion-wise (mmtta_lesionwise_nsd), against scipy, and the
evaluators that report them.

The oracle: a voxel of edge(A) is a hit at tau iff ``oracle.surface.surface_distance(edge A, edge B, spacing) <= float32(tau)``
(scipy's exact distance transform, cast to float32), with ``oracle.surface.mask_edges`` for the edges.  The lesion-wise oracle
restates lesions and matching as tests/test_hip_lesionwise.py does (binary_dilation, ``ndimage.label`` with the 26-neighbourhood,
``np.isin``) and takes the edges of A_g and of P_g with ``mask_edges`` on those masks themselves.  Every count is an integer and
must be EQUAL.  The tolerances are chosen so that the oracle is unambiguous: ``check_tolerances`` enumerates the offsets a window
can hold and asserts that a tolerance is 0, or equals an exactly representable distance at unit spacing (d^2 an integer), or
keeps a relative gap >= 1e-4 to every achievable distance.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q30 = 1 << 30
SHAPES = [(5, 19, 70), (24, 24, 40)]
UNIT, ANISO = (1.0, 1.0, 1.0), (2.0, 1.0, 0.75)
# unit: r = (1, 1, 1); anisotropic: r = (1, 2, 2)
TOLERANCES = {UNIT: (0.0, 0.5, 1.0, 1.5), ANISO: (0.0, 0.8, 1.3, 2.1)}
N, R = 2, 3
MIN_LESION = [0, 5, 1]
_id = lambda s: "x".join(map(str, s))


def check_tolerances(spacing, tolerances):
    from multimodal_tta_amd import ops
    rad = ops.surface_dice_radius(spacing, max(tolerances))
    assert max(rad) <= ops.SURFACE_DICE_MAX_RADIUS
    dist = sorted({float(np.sqrt(sum((k * s) ** 2 for k, s in zip(off, spacing))))
                   for off in itertools.product(*(range(0, r + 2) for r in rad))})
    for tau in tolerances:
        if tau == 0.0:
            continue
        exact = tuple(spacing) == UNIT and float(tau * tau).is_integer()
        gap = min(abs(d - tau) / tau for d in dist)
        assert exact or gap >= 1e-4, f"tolerance {tau} at spacing {spacing} is within {gap:.2e} of an achievable distance"
    return rad


# ----------------------------------------------------------------------------- the scipy oracles
def hits(edge_a, edge_b, spacing, tolerances):
    """Voxels of edge_a within each tolerance of edge_b: one distance transform for all of them."""
    from oracle.surface import surface_distance
    if not edge_a.any():
        return [0] * len(tolerances)
    d = surface_distance(edge_a, edge_b, spacing)
    return [int((d <= np.float32(tau)).sum()) for tau in tolerances]


def region_oracle(P, G, spacing, tolerances):
    """P, G bool [D,H,W] -> int [T,4]: hits P->G, |edge P|, hits G->P, |edge G|."""
    from oracle.surface import mask_edges
    ep, eg = mask_edges(P), mask_edges(G)
    hp, hg = hits(ep, eg, spacing, tolerances), hits(eg, ep, spacing, tolerances)
    return np.array([[hp[t], int(ep.sum()), hg[t], int(eg.sum())] for t in range(len(tolerances))], dtype=np.int64)


def lesion_oracle(P, G, iterations, conn, min_voxels, spacing, tolerances):
    """P, G bool [D,H,W] -> (kept, found, {root index of the lesion: [(hits, den)] per tolerance})."""
    from scipy import ndimage
    from oracle.surface import mask_edges
    s26 = ndimage.generate_binary_structure(3, 3)
    Gd = G.copy()
    if iterations > 0:
        Gd = ndimage.binary_dilation(G, ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]), iterations)
    lg, ng = ndimage.label(Gd, structure=s26)
    lp, _ = ndimage.label(P, structure=s26)
    kept = found = 0
    out = {}
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
            ea, ep = mask_edges(own), mask_edges(np.isin(lp, ids))
            den = int(ea.sum() + ep.sum())
            ha, hp = hits(ea, ep, spacing, tolerances), hits(ep, ea, spacing, tolerances)
            out[int(np.flatnonzero(comp)[0])] = [(ha[t] + hp[t], den) for t in range(len(tolerances))]
    return kept, found, out


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()      # a writable, contiguous copy


def check_region(mask, label, spacing, tolerances, what=""):
    from multimodal_tta_amd import ops
    check_tolerances(spacing, tolerances)
    m = _cuda(mask)
    keep = m.clone()
    got = ops.surface_dice(m, _cuda(label), spacing, tolerances)
    torch.cuda.synchronize()
    assert torch.equal(m, keep), "the input mask was written"
    assert got.dtype == torch.int64 and tuple(got.shape) == mask.shape[:2] + (len(tolerances), 4)
    got = got.cpu().numpy()
    for n in range(mask.shape[0]):
        for r in range(mask.shape[1]):
            want = region_oracle(mask[n, r] != 0, label[n, r] > 0.5, spacing, tolerances)
            print(what, (n, r), "got", got[n, r].tolist(), "want", want.tolist())
            assert np.array_equal(got[n, r], want), f"{what} {(n, r)}: {got[n, r].tolist()} vs {want.tolist()}"
    return got


def check_lesion(mask, label, it, conn, minv, spacing, tolerances, what=""):
    from multimodal_tta_amd import ops
    check_tolerances(spacing, tolerances)
    m = _cuda(mask)
    keep = m.clone()
    res = ops.lesionwise_nsd(m, _cuda(label), it, conn, minv, spacing, tolerances, want_lesion_nsd=True)
    alone = ops.lesionwise_scores(_cuda(mask), _cuda(label), it, conn, minv)["stats"]
    torch.cuda.synchronize()
    assert torch.equal(m, keep), "the input mask was written"
    assert torch.equal(res["stats"], alone), f"{what}: stats differ from ops.lesionwise_scores"
    T = len(tolerances)
    assert res["nsd_stats"].dtype == torch.int64 and tuple(res["nsd_stats"].shape) == mask.shape[:2] + (T,)
    assert res["lesion_nsd"].dtype == torch.float32 and tuple(res["lesion_nsd"].shape) == mask.shape[:2] + (T,) + mask.shape[2:]
    stats, nsd_stats, lesion_nsd = res["stats"].cpu().numpy(), res["nsd_stats"].cpu().numpy(), res["lesion_nsd"].cpu().numpy()
    mv = [minv] * mask.shape[1] if isinstance(minv, int) else list(minv)
    scored = 0
    for n in range(mask.shape[0]):
        for r in range(mask.shape[1]):
            kept, found, want = lesion_oracle(mask[n, r] != 0, label[n, r] > 0.5, it, conn, mv[r], spacing, tolerances)
            assert stats[n, r, 1] == kept and stats[n, r, 2] == found
            scored += len(want)
            for t in range(T):
                got = lesion_nsd[n, r, t].ravel()
                at = np.flatnonzero(~np.isnan(got))
                assert sorted(at.tolist()) == sorted(want), f"{what} {(n, r)}: scored lesions {at.tolist()} vs {sorted(want)}"
                want_q = sum((num * Q30 + den // 2) // den for num, den in (v[t] for v in want.values()))
                print(what, (n, r), tolerances[t], "got", int(nsd_stats[n, r, t]), {int(i): float(got[i]) for i in at[:8]},
                      "want", want_q, {k: v[t] for k, v in list(want.items())[:8]})
                for root, v in want.items():
                    assert got[root] == np.float32(v[t][0] / v[t][1]), f"{what} {(n, r)} tau {tolerances[t]} lesion {root}: {got[root]} vs {v[t]}"
                assert int(nsd_stats[n, r, t]) == want_q, f"{what} {(n, r)} tau {tolerances[t]}: {nsd_stats[n, r, t]} vs {want_q}"
    return res, scored


# ----------------------------------------------------------------------------- cases
def _balls(rng, shape, count, rmax):
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros(shape, dtype=bool)
    for _ in range(count):
        c = [rng.integers(0, e) for e in shape]
        rad = rng.uniform(0.5, rmax)
        out |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= rad * rad
    return out


def _shift(a, dz=0, dy=0, dx=0):
    out = np.zeros_like(a)
    D, H, W = a.shape
    out[dz:, dy:, dx:] = a[:D - dz, :H - dy, :W - dx]
    return out


@functools.lru_cache(maxsize=None)
def region_cases(shape, which):
    """N = 2, R = 3 (prediction, ground truth) pairs in one call."""
    rng = np.random.default_rng(17 + sum(shape) + which)
    blob = lambda: _balls(rng, shape, 6, 4.0)
    full, none = np.ones(shape, dtype=bool), np.zeros(shape, dtype=bool)
    a, b = blob(), blob()
    if which == 0:
        pairs = [((a & (rng.random(shape) < 0.8)) | (rng.random(shape) < 0.004), a),      # random blobs, thinned, plus speckle
                 (none, b),                                                              # empty prediction
                 (a, none),                                                              # empty ground truth
                 (full, b),                                                              # full mask: its edges are the volume faces
                 (b, b),                                                                 # identical: NSD = 1 at tau = 0
                 (_shift(a, dx=1), a)]                                                   # shifted by one along W
    else:
        pairs = [(_shift(a, dz=2), a), (_shift(b, dx=2), b), (_shift(a, dy=1), a), (full, full),
                 (rng.random(shape) < 0.05, rng.random(shape) < 0.05), (b | blob(), b)]
    mask = np.stack([p for p, _ in pairs]).reshape((N, R) + shape).astype(np.uint8)
    label = np.stack([g for _, g in pairs]).reshape((N, R) + shape).astype(np.float32)
    mask.setflags(write=False)
    label.setflags(write=False)
    return mask, label


@pytest.mark.parametrize("spacing", [UNIT, ANISO], ids=["iso", "aniso"])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_region_counts_match_scipy(shape, which, spacing):
    mask, label = region_cases(shape, which)
    got = check_region(mask, label, spacing, TOLERANCES[spacing], f"{_id(shape)} set {which}")
    if which == 0:
        assert got[0, 1, :, :3].sum() == 0 and got[0, 1, 0, 3] > 0            # empty prediction: all misses
        assert got[0, 2, :, 3].sum() == 0 and got[0, 2, 0, 1] > 0             # empty ground truth
        D, H, W = shape
        assert got[1, 0, 0, 1] == D * H * W - max(D - 2, 0) * max(H - 2, 0) * max(W - 2, 0)      # the faces of the volume
        assert (got[1, 1, :, 0] == got[1, 1, :, 1]).all() and (got[1, 1, :, 2] == got[1, 1, :, 3]).all()      # identical at tau = 0 ... max
        assert (got[1, 2, 2:, 0] == got[1, 2, 2:, 1]).all() and got[1, 2, 0, 0] < got[1, 2, 0, 1]             # one voxel off: all within 1


def test_region_window_at_the_cap():
    shape = (24, 24, 40)
    mask, label = region_cases(shape, 1)
    rad = check_tolerances(UNIT, (2.0, 8.0))
    assert rad == (8, 8, 8)
    got = check_region(mask, label, UNIT, (2.0, 8.0), "cap")
    assert (got[:, :, 1, 0] >= got[:, :, 0, 0]).all()
    rad = check_tolerances((2.0, 1.0, 1.5), (3.3, 8.3))
    assert rad == (4, 8, 5)
    check_region(mask[:1], label[:1], (2.0, 1.0, 1.5), (3.3, 8.3), "cap aniso")


def test_region_strided_labels_batch_and_repeat():
    from multimodal_tta_amd import ops
    shape = SHAPES[0]
    mask, label = region_cases(shape, 0)
    tol = TOLERANCES[ANISO]
    m, lab = _cuda(mask), _cuda(label)
    ref = ops.surface_dice(m, lab, ANISO, tol)
    assert torch.equal(ops.surface_dice(m, lab, ANISO, tol), ref), "two calls differ"
    wide = torch.zeros((N, R) + shape[:2] + (shape[2] + 7,), device="cuda")
    wide[..., :shape[2]] = lab
    assert torch.equal(ops.surface_dice(m, wide[..., :shape[2]], ANISO, tol), ref), "a W-strided label differs"
    cl = lab.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)      # channels-last storage
    assert not cl.is_contiguous() and torch.equal(ops.surface_dice(m, cl, ANISO, tol), ref)
    same = lab[:1].expand(N, -1, -1, -1, -1)      # one label for the whole batch, stride 0 (evaluation.check_batch)
    both = ops.surface_dice(m, same, ANISO, tol)
    for n in range(N):
        for r in range(R):
            one = ops.surface_dice(m[n:n + 1, r:r + 1].contiguous(), lab[n:n + 1, r:r + 1].contiguous(), ANISO, tol)
            assert torch.equal(one[0, 0], ref[n, r]), f"item {(n, r)} alone differs from the batch"
            one = ops.surface_dice(m[n:n + 1, r:r + 1].contiguous(), lab[:1, r:r + 1].contiguous(), ANISO, tol)
            assert torch.equal(one[0, 0], both[n, r])
    with torch.cuda.stream(torch.cuda.Stream()):
        other = ops.surface_dice(m, lab, ANISO, tol)
    torch.cuda.synchronize()
    assert torch.equal(other, ref)
    for t, tau in enumerate(tol):      # a subset of the tolerances gives the same columns
        assert torch.equal(ops.surface_dice(m, lab, ANISO, (tau,))[:, :, 0], ref[:, :, t])


# ----------------------------------------------------------------------------- lesion-wise
@functools.lru_cache(maxsize=None)
def lesion_random_case(shape):
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


@pytest.mark.parametrize("setting", [(0, 6, UNIT), (3, 18, ANISO), (3, 18, UNIT), (1, 26, ANISO)],
                         ids=lambda s: f"{s[0]}x{s[1]}-{'iso' if s[2] == UNIT else 'aniso'}")
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_lesion_random_blobs_match_scipy(shape, setting):
    it, conn, spacing = setting
    mask, label = lesion_random_case(shape)
    _, scored = check_lesion(mask, label, it, conn, MIN_LESION, spacing, TOLERANCES[spacing], f"{_id(shape)} {setting}")
    assert scored > 0, "no lesion scored: the case shows nothing"


@functools.lru_cache(maxsize=None)
def lesion_structured_case():
    """N * R = 6 masks of 12 x 20 x 33 in one call."""
    shape = (12, 20, 33)
    P, G = np.zeros((6,) + shape, dtype=bool), np.zeros((6,) + shape, dtype=bool)
    # 0: two lesions and one component touching both
    G[0, 4:8, 4:8, 4:9] = True; G[0, 4:8, 4:8, 20:26] = True; P[0, 5:7, 5:7, 6:23] = True
    # 1: a matched component next to an unmatched one whose surface is nearer to part of the lesion
    G[1, 3:9, 6:12, 10:16] = True; P[1, 3:9, 6:12, 6:12] = True; P[1, 3:9, 6:12, 17:20] = True
    # 2: a kept lesion with no match, beside a matched one
    G[2, 2:5, 2:5, 2:5] = True; G[2, 6:10, 10:15, 20:28] = True; P[2, 6:10, 11:16, 21:29] = True
    # 3: a lesion below min_lesion_voxels (region 0 of the second item: threshold 0 -> use region index 1 via layout below)
    G[3, 5, 5, 5:7] = True; P[3, 4:7, 4:7, 4:8] = True; G[3, 2:6, 12:17, 20:26] = True; P[3, 3:7, 12:17, 21:27] = True
    # 4: false positives only
    P[4, 2:5, 2:5, 2:5] = True; P[4, 8, 15, 30] = True
    # 5: a component matched to one lesion and lying within tolerance of another it does not touch
    G[5, 4:8, 4:8, 4:8] = True; G[5, 4:8, 4:8, 11:15] = True; P[5, 4:8, 4:8, 5:10] = True
    # item 0 holds cases 0, 3, 1 and item 1 cases 2, 4, 5: case 3 sits at region 1, whose threshold is 5 voxels
    order = [0, 3, 1, 2, 4, 5]
    mask = P[order].reshape((N, R) + shape).astype(np.uint8)
    label = G[order].reshape((N, R) + shape).astype(np.float32)
    mask.setflags(write=False)
    label.setflags(write=False)
    return mask, label


@pytest.mark.parametrize("setting", [(0, 6, UNIT), (0, 6, ANISO), (3, 18, UNIT)], ids=["0x6-iso", "0x6-aniso", "3x18-iso"])
def test_lesion_structured_cases(setting):
    it, conn, spacing = setting
    mask, label = lesion_structured_case()
    res, _ = check_lesion(mask, label, it, conn, MIN_LESION, spacing, TOLERANCES[spacing], f"structured {setting}")
    stats, nsd = res["stats"].cpu().numpy(), res["nsd_stats"].cpu().numpy()
    if it == 0:
        assert stats[0, 0, 1:3].tolist() == [2, 2] and stats[0, 0, 4] == 1                 # one component, both lesions
        assert stats[0, 1, 0] == 2 and stats[0, 1, 1:3].tolist() == [1, 1]                 # the 2-voxel lesion is dropped
        assert stats[0, 2, 3:5].tolist() == [2, 1]                                         # the unmatched neighbour
        assert stats[1, 0, 1:3].tolist() == [2, 1]                                         # one kept lesion is missed
        assert stats[1, 1, 1] == 0 and stats[1, 1, 3:5].tolist() == [2, 0] and (nsd[1, 1] == 0).all()      # false positives only
    if setting == (0, 6, UNIT):
        # case 1 shows something: at tau = 1.5 the lesion's far face is within reach of the unmatched component (x = 15 against
        # x = 17 is 2 away, the corners of the gap are not; so use the region count at tau = 2 of a one-off call) but not of the
        # matched one, so a pass that took the nearest predicted surface would score the lesion higher
        P, G = mask[0, 2] != 0, label[0, 2] > 0.5
        region = region_oracle(P, G, UNIT, [2.0])[0]
        _, _, les = lesion_oracle(P, G, 0, 6, 1, UNIT, [2.0])
        (num, den), = list(les.values())[0]
        assert den < region[1] + region[3] and num < region[0] + region[2]
        check_lesion(mask[:1], label[:1], 0, 6, MIN_LESION, UNIT, (2.0,), "structured tau 2")


def test_lesion_many_lesions_in_one_window_take_the_fallback():
    """dilation 0: one predicted block over a lattice of one-voxel lesions, two voxels apart.  Every lesion is matched to the
    block, and an edge voxel of the block has several times as many of them within the largest tolerance as a thread's list
    holds (the library says how many that is), so the launch for marked voxels does the counting."""
    from multimodal_tta_amd import ops
    from oracle.surface import mask_edges
    shape = (9, 17, 40)
    P, G = np.zeros((6,) + shape, dtype=bool), np.zeros((6,) + shape, dtype=bool)
    for i in range(6):
        P[i, 1:8, 2:15, 3:3 + 3 * (i + 2)] = True
        G[i, 1:8:2, 2:15:2, 3:3 + 3 * (i + 2):2] = True
    P[:, 4, 7, 5] = False      # a pit inside the block: interior edge voxels with lesions all around
    G[3] = False               # one mask with false positives only
    G[4, 1:8:2, 2:15:2, 19:31:2] = True      # x = 19 lies in the block, the others are not reached: kept, not found
    mask, label = P.reshape((N, R) + shape).astype(np.uint8), G.reshape((N, R) + shape).astype(np.float32)
    tol = (0.0, 1.0, 2.0, 2.5)
    near = 0
    ep, eg = mask_edges(P[5]), mask_edges(G[5])
    zz, yy, xx = np.nonzero(eg)
    for z, y, x in np.argwhere(ep):
        near = max(near, int((((zz - z) ** 2 + (yy - y) ** 2 + (xx - x) ** 2) <= 2.5 ** 2).sum()))
    slots = ops.lesionwise_nsd_list_slots()
    print("lesions within reach of one edge voxel:", near, "list slots:", slots)
    assert near >= 4 * slots, f"{near} lesions in a window against {slots} list slots: the case may not overflow the list"
    res, scored = check_lesion(mask, label, 0, 6, 0, UNIT, tol, "lattice")
    assert scored > 100
    assert res["stats"][0, 0, 4] == 1 and res["stats"][0, 0, 2] == res["stats"][0, 0, 1] > 50
    check_lesion(mask[:1], label[:1], 0, 26, 1, (1.0, 1.0, 0.75), (0.0, 0.8, 1.3, 1.55), "lattice aniso")


def test_lesion_batch_repeat_and_neighbours_unchanged(monkeypatch):
    from multimodal_tta_amd import ops
    shape = SHAPES[0]
    mask, label = lesion_random_case(shape)
    tol, args = TOLERANCES[ANISO], (3, 18, MIN_LESION)
    m, lab = _cuda(mask), _cuda(label)
    hd_ref = ops.lesionwise_hd95(m, lab, *args, ANISO, want_lesion_hd=True)
    hd_ref = {k: v.clone() for k, v in hd_ref.items() if v is not None}
    ref = ops.lesionwise_nsd(m, lab, *args, ANISO, tol, want_lesion_nsd=True)
    ref = {k: v.clone() for k, v in ref.items() if v is not None}
    again = ops.lesionwise_nsd(m, lab, *args, ANISO, tol, want_lesion_nsd=True)
    for k in ref:
        assert torch.equal(again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k],
                           ref[k].view(torch.int32) if ref[k].dtype == torch.float32 else ref[k]), f"two calls differ in {k}"
    assert torch.equal(ref["stats"], hd_ref["stats"])
    # the NSD pass between the lesion-wise scores and the HD95 pass, and once more behind them
    real = ops.lesionwise_scores
    between = {}

    def scores_then_nsd(mk, *a, **k):
        out = real(mk, *a, **k)
        between.update(ops.lesionwise_nsd_after_scores(mk, MIN_LESION, ANISO, tol, want_lesion_nsd=True))
        return out

    monkeypatch.setattr(ops, "lesionwise_scores", scores_then_nsd)
    hd = ops.lesionwise_hd95(m, lab, *args, ANISO, want_lesion_hd=True)
    monkeypatch.setattr(ops, "lesionwise_scores", real)
    behind = ops.lesionwise_nsd_after_scores(m, MIN_LESION, ANISO, tol, want_lesion_nsd=True)
    torch.cuda.synchronize()
    for k in ("stats", "hd_stats"):
        assert torch.equal(hd[k], hd_ref[k]), f"{k} moved with the NSD pass in between"
    assert torch.equal(hd["lesion_hd"].view(torch.int32), hd_ref["lesion_hd"].view(torch.int32))
    for got in (between, behind):
        assert torch.equal(got["nsd_stats"], ref["nsd_stats"])
        assert torch.equal(got["lesion_nsd"].view(torch.int32), ref["lesion_nsd"].view(torch.int32))
    # a batch gives what its items give alone
    for n in range(N):
        one = ops.lesionwise_nsd(m[n:n + 1].contiguous(), lab[n:n + 1].contiguous(), *args, ANISO, tol)
        assert torch.equal(one["nsd_stats"][0], ref["nsd_stats"][n]) and torch.equal(one["stats"][0], ref["stats"][n])
    one = ops.lesionwise_nsd(m[1:, 1:2].contiguous(), lab[1:, 1:2].contiguous(), 3, 18, MIN_LESION[1], ANISO, tol[1:3])
    assert torch.equal(one["nsd_stats"][0, 0], ref["nsd_stats"][1, 1, 1:3])


def test_refusals_queue_nothing():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    m = torch.zeros((1, 2, 4, 5, 6), dtype=torch.uint8, device="cuda")
    lab = torch.zeros((1, 2, 4, 5, 6), device="cuda")
    for fn in (ops.surface_dice, ops.lesionwise_nsd):
        for bad in ((), (0.5,) * 5, (0.5,) * 6, (-1.0,), (float("nan"),), (float("inf"),)):
            with pytest.raises(MmttaError, match="tolerances"):
                fn(m, lab, tolerances=bad)
        with pytest.raises(MmttaError, match="window"):
            fn(m, lab, tolerances=(9.0,))
        with pytest.raises(MmttaError, match="window"):
            fn(m, lab, spacing=(2.0, 1.0, 0.75), tolerances=(6.8,))
        with pytest.raises(MmttaError):
            fn(m.float(), lab)
        with pytest.raises(MmttaError):
            fn(m, lab.double())
    with pytest.raises(MmttaError, match="extent"):
        ops.surface_dice(torch.zeros((1, 1, 1, 1, 1025), dtype=torch.uint8, device="cuda"), torch.zeros((1, 1, 1, 1, 1025), device="cuda"))
    assert ops.surface_dice(m, lab, tolerances=(8.0,)).sum() == 0      # the cap itself is fine


# ----------------------------------------------------------------------------- evaluators
REGIONS = ["ET", "TC", "WT"]
LW = {"enable": True, "dilation": 2, "dilation_connectivity": 18, "min_lesion_voxels": [0, 3, 1]}
SPACING = [1.5, 0.8, 2.0]
SD_TOL, LN_TOL = [1.0, 2.3], [0.5, 1.0, 1.8]


def _e2e_cfg(sd, nsd, threshold, **method):
    from test_hip_lesionwise import _e2e_cfg as base
    cfg = base(LW, threshold, None, **method)
    cfg["evaluation"]["seg"]["spacing"] = list(SPACING)
    if sd is not None:
        cfg["evaluation"]["surface_dice"] = dict(sd)
    if nsd is not None:
        cfg["evaluation"]["lesionwise"]["nsd"] = dict(nsd)
    return cfg


def expected_keys(masks, labels, domain="synth"):
    """The NSD keys of the scored masks uint8 [V,R,D,H,W], overall and under dom/<domain>/ (one domain)."""
    from test_hip_lesionwise import oracle as lw_oracle
    check_tolerances(SPACING, SD_TOL)
    check_tolerances(SPACING, LN_TOL)
    stats, _ = lw_oracle(masks, labels, LW["dilation"], LW["dilation_connectivity"], LW["min_lesion_voxels"])
    V = masks.shape[0]
    want = {}
    for stem, tols in (("nsd", SD_TOL), ("lw_nsd", LN_TOL)):
        for t, tau in enumerate(tols):
            means, used = [], []
            for r, name in enumerate(REGIONS):
                vals = []
                for i in range(V):
                    P, G = masks[i, r] != 0, labels[i, r] > 0.5
                    if stem == "nsd":
                        if G.any():
                            c = region_oracle(P, G, SPACING, [tau])[0]
                            vals.append((c[0] + c[2]) / (c[1] + c[3]))
                    else:
                        kept, found, les = lesion_oracle(P, G, LW["dilation"], LW["dilation_connectivity"],
                                                         LW["min_lesion_voxels"][r], SPACING, [tau])
                        den = kept + int(stats[i, r, 3] - stats[i, r, 4])
                        if den > 0:
                            vals.append(sum((num * Q30 + d // 2) // d for (num, d), in les.values()) / Q30 / den)
                key = f"{name.lower()}_{stem}_{'%g' % tau}"
                want[key] = sum(vals) / len(vals) if vals else 0.0
                means.append(want[key])
                used.append(bool(vals))
            ok = [m for m, u in zip(means, used) if u]
            want[f"avg_{stem}_{'%g' % tau}"] = sum(ok) / max(1, len(ok))
    want.update({f"dom/{domain}/{k}": v for k, v in list(want.items())})
    assert any(0.0 < v < 1.0 for v in want.values()), "every score is 0 or 1: the case shows nothing"
    return want


def _check_e2e(m_on, m_off, want):
    assert set(m_on) == set(m_off) | set(want), sorted(set(m_on) ^ (set(m_off) | set(want)))
    for k, v in want.items():
        assert m_on[k] == pytest.approx(v, rel=1e-12, abs=1e-15), (k, m_on[k], v)
    for k, v in m_off.items():
        assert m_on[k] == v, f"pre-existing key {k} moved: {m_on[k]} vs {v}"


def _count_calls(monkeypatch):
    from multimodal_tta_amd import ops
    calls = []
    for name in ("surface_dice", "lesionwise_nsd_after_scores"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
    return calls


def test_seg_tta_eval_reports_nsd(monkeypatch):
    from multimodal_tta_amd.evaluation import table_width
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_lesionwise import _speckle_threshold
    from test_hip_tta import SMALL, build_pair

    thr = _speckle_threshold()
    calls = _count_calls(monkeypatch)
    on_sd, on_ln = {"enable": True, "tolerances": SD_TOL}, {"enable": True, "tolerances": LN_TOL}
    runs = {}
    for name, sd, nsd, method in (("absent", None, None, dict(lanes=2, group=2)),
                                  ("off", {"enable": False, "tolerances": [2.0]}, {"enable": False}, dict(lanes=2, group=2)),
                                  ("grouped", on_sd, on_ln, dict(lanes=2, group=2)), ("single", on_sd, on_ln, dict(lanes=2, group=1))):
        cfg = _e2e_cfg(sd, nsd, thr, **method)
        _, hip = build_pair(SMALL)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_tta_eval")(cfg)
        runs[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
        if name == "off":
            assert not calls, "an NSD pass ran with the blocks absent or off"
    assert calls
    labels = np.concatenate([b["label"].numpy() for b in loader]).astype(np.float32)
    (m_abs, s_abs), (m_off, s_off) = runs["absent"], runs["off"]
    assert m_off == m_abs and list(m_off) == list(m_abs) and torch.equal(s_off.last_table, s_abs.last_table)
    m_on, s_on = runs["grouped"]
    scored = np.stack([s_on.last_masks[i].numpy() for i in range(3)])
    assert np.array_equal(scored, np.stack([s_off.last_masks[i].numpy() for i in range(3)]))
    _check_e2e(m_on, m_off, expected_keys(scored, labels))
    base = table_width(3, lesionwise=True)
    assert s_on.last_table.shape == (3, table_width(3, lesionwise=True, surface_dice=2, lesionwise_nsd=3)) == (3, base + 15)
    assert torch.equal(s_on.last_table[:, :base], s_off.last_table)
    m_one, s_one = runs["single"]      # grouped == one at a time, bit for bit
    assert m_one == m_on and torch.equal(s_one.last_table, s_on.last_table)


def test_seg_eval_reports_nsd(monkeypatch):
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_lesionwise import _speckle_threshold
    from test_hip_tta import SMALL, build_pair

    _, hip = build_pair(SMALL)
    thr = _speckle_threshold()
    calls = _count_calls(monkeypatch)
    res = {}
    for name, sd, nsd in (("absent", None, None), ("off", {"enable": False}, {"enable": False, "tolerances": [0.25]}),
                          ("on", {"enable": True, "tolerances": SD_TOL}, {"enable": True, "tolerances": LN_TOL})):
        cfg = _e2e_cfg(sd, nsd, thr)
        cfg["training"]["eval_batch_size"] = 2
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_eval")(cfg)
        res[name] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
        if name == "off":
            assert not calls, "an NSD pass ran with the blocks absent or off"
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
    _check_e2e(res["on"][0], m_off, expected_keys(np.concatenate(raw), np.concatenate(labels)))
