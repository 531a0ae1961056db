"""The calibration kernel (mmtta_calibration_bins) against a float64 restatement in numpy, and the evaluators that report
ECE / Brier / NLL from it.

Required agreement, from the arithmetic (n: elements of a (volume, region), n_b: of one of its bins):
  * count and correct count per bin: exactly equal;
  * sum of confidence per bin: within n_b * 2^-21 (an fp32 confidence is a few ulp of a value <= 1 off);
  * Brier sum: within n * 2^-21;
  * NLL sum: within 2^-20 * sum |term| + n * 2^-23.
Counts can only be compared exactly where no confidence sits on a bin edge, so the inputs are prepared on the CPU first: a
logit whose float64 confidence lies within 1e-5 of an INTERIOR edge k/B (0 < k < B) is moved by 1e-3, and the test asserts
that none remains.  The outer edges 0 and 1 are not edges in that sense: the index is clamped to [0, B-1], no confidence
exceeds 1, so the planted saturated logits (+-40, +-100: c = 1 in fp32) stay in.  Nothing is left out of the comparison.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EXTENTS = [(5, 7, 9), (16, 16, 16), (24, 40, 33)]
BINS = (1, 10, 15)
EDGE = 1e-5
N = 2


# ----------------------------------------------------------------------------- the float64 restatement
def _confidence(z, softmax):
    """z float64 [N,R,D,H,W] -> confidence [N,Rout,D,H,W]."""
    if softmax:
        return 1.0 / np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)
    return 1.0 / (1.0 + np.exp(-np.abs(z)))


def ref_elements(z32, lab32, softmax):
    """Per element: confidence, correct, foreground-of-either, Brier term, NLL term; float64 [N,Rout,D,H,W] each."""
    z = z32.astype(np.float64)
    if softmax:
        m = z.max(1, keepdims=True)
        ex = np.exp(z - m)
        se = ex.sum(1, keepdims=True)
        p = ex / se
        pred = z.argmax(1)[:, None]                      # lowest index on ties
        cls = lab32.argmax(1)[:, None]
        y = (np.arange(z.shape[1]).reshape(1, -1, 1, 1, 1) == cls).astype(np.float64)
        brier = ((p - y) ** 2).sum(1, keepdims=True)
        nll = (m + np.log(se)) - np.take_along_axis(z, cls, 1)
        return 1.0 / se, pred == cls, (pred != 0) | (cls != 0), brier, nll
    y = (lab32 > 0.5)
    e = np.exp(-np.abs(z))
    c = 1.0 / (1.0 + e)
    pred = z >= 0
    sig = np.where(pred, c, e / (1.0 + e))
    brier = (sig - y) ** 2
    nll = np.maximum(z, 0) - z * y + np.log1p(e)
    return c, pred == y, pred | y, brier, nll


def ref_table(z32, lab32, softmax, bins, scope):
    """-> table float64 [N,Rout,3*bins+2], and per (N,Rout): n and sum |NLL term| for the bounds."""
    c, correct, fg, brier, nll = ref_elements(z32, lab32, softmax)
    keep = np.ones_like(fg) if scope == "volume" else fg
    idx = np.minimum(bins - 1, np.maximum(0, np.ceil(c * bins).astype(np.int64) - 1))
    n_, r_ = c.shape[:2]
    out = np.zeros((n_, r_, 3 * bins + 2))
    for n in range(n_):
        for r in range(r_):
            k = keep[n, r].reshape(-1)
            i = idx[n, r].reshape(-1)[k]
            out[n, r, 0:3 * bins:3] = np.bincount(i, minlength=bins)
            out[n, r, 1:3 * bins:3] = np.bincount(i, weights=c[n, r].reshape(-1)[k], minlength=bins)
            out[n, r, 2:3 * bins:3] = np.bincount(i, weights=correct[n, r].reshape(-1)[k].astype(np.float64), minlength=bins)
            out[n, r, 3 * bins] = brier[n, r].reshape(-1)[k].sum()
            out[n, r, 3 * bins + 1] = nll[n, r].reshape(-1)[k].sum()
    n_el = keep.reshape(n_, r_, -1).sum(-1).astype(np.float64)
    abs_nll = (np.abs(nll) * keep).reshape(n_, r_, -1).sum(-1)
    return out, n_el, abs_nll


def assert_tables_agree(got, want, n_el, abs_nll, bins, what):
    cnt_g, cnt_w = got[..., 0:3 * bins:3], want[..., 0:3 * bins:3]
    assert np.array_equal(cnt_g, cnt_w), f"{what}: counts differ\n{cnt_g}\n{cnt_w}"
    assert np.array_equal(got[..., 2:3 * bins:3], want[..., 2:3 * bins:3]), f"{what}: correct counts differ"
    assert cnt_w.sum(-1).tolist() == n_el.tolist()
    d_conf = np.abs(got[..., 1:3 * bins:3] - want[..., 1:3 * bins:3])
    assert (d_conf <= cnt_w * 2.0 ** -21).all(), f"{what}: confidence sums off by {d_conf.max()} (bins of {cnt_w.max()})"
    d_brier = np.abs(got[..., 3 * bins] - want[..., 3 * bins])
    assert (d_brier <= n_el * 2.0 ** -21).all(), f"{what}: Brier sums off by {d_brier} for n = {n_el}"
    d_nll = np.abs(got[..., 3 * bins + 1] - want[..., 3 * bins + 1])
    assert (d_nll <= 2.0 ** -20 * abs_nll + n_el * 2.0 ** -23).all(), f"{what}: NLL sums off by {d_nll} for n = {n_el}"
    assert np.isfinite(got).all()


# ----------------------------------------------------------------------------- inputs
def _near_edge(z32, softmax, bins):
    c = _confidence(z32.astype(np.float64), softmax)
    near = np.zeros(c.shape, dtype=bool)
    for k in range(1, bins):
        near |= np.abs(c - k / bins) <= EDGE
    return near


@functools.lru_cache(maxsize=None)
def make_case(softmax, R, extent, bins, seed=0):
    """3*randn logits with planted +-40, +-100 (saturation, finite NLL) and exact zeros (c = 0.5 resp. 1/R, exact in fp32),
    moved off the interior bin edges of `bins`; labels {0,1} (one-hot or all-zero per voxel on the softmax head)."""
    rng = np.random.default_rng(seed + 1000 * R + extent[0])
    shape = (N, R) + tuple(extent)
    z = (3.0 * rng.standard_normal(shape)).astype(np.float32)
    flat = z.reshape(-1)
    planted = rng.choice(flat.size, size=min(flat.size // 4, 60), replace=False)
    flat[planted] = np.resize(np.array([40, -40, 100, -100, 0, 0], dtype=np.float32), planted.size)
    if softmax:
        z.reshape(N, R, -1)[:, :, :3] = 0.0              # whole voxels of zeros: argmax ties, c = 1/R
        cls = rng.integers(0, R, (N,) + tuple(extent))
        lab = (np.arange(R).reshape(1, R, 1, 1, 1) == cls[:, None]).astype(np.float32)
        lab[:, :, 0, 0, :2] = 0.0                        # label ties: class 0
    else:
        lab = (rng.random(shape) < 0.3).astype(np.float32)
        lab[1, R - 1] = 0.0                              # an empty ground truth
        z[1, R - 1] = -np.abs(z[1, R - 1]) - 0.01        # ... with an empty prediction: no element in union scope
    for _ in range(4):
        near = _near_edge(z, softmax, bins)
        if not near.any():
            break
        if softmax:                                      # move the voxel's winning logit
            top = z.argmax(1)[:, None]
            hit = near & (np.arange(R).reshape(1, R, 1, 1, 1) == top)
            z = np.where(hit, z + np.float32(1e-3), z).astype(np.float32)
        else:
            z = np.where(near, z + np.float32(1e-3), z).astype(np.float32)
    assert not _near_edge(z, softmax, bins).any()
    z.setflags(write=False)
    lab.setflags(write=False)
    return z, lab


@functools.lru_cache(maxsize=None)
def reference(softmax, R, extent, bins, scope):
    z, lab = make_case(softmax, R, extent, bins)
    return ref_table(z, lab, softmax, bins, scope)


def channels_last_with_nan_pad(z):
    """[N,R,D,H,W] -> the view [N,D,H,W,R] of a buffer with rows of ldc = multiple of 4 floats whose pad lanes hold NaN."""
    n, r, d, h, w = z.shape
    buf = torch.full((n, d, h, w, (r + 3) // 4 * 4), float("nan"), dtype=torch.float32, device="cuda")
    buf[..., :r] = z.permute(0, 2, 3, 4, 1)
    return buf[..., :r]


def run_kernel(z, lab, softmax, bins, scope, layout, strided_label=False):
    from multimodal_tta_amd import ops
    zg, lg = torch.from_numpy(np.array(z)).cuda(), torch.from_numpy(np.array(lab)).cuda()
    if strided_label:                                    # NCDHW view of channels-last storage with padded rows
        n, r, d, h, w = lg.shape
        store = torch.full((n, d, h, w + 3, r), 9.0, dtype=torch.float32, device="cuda")
        store[:, :, :, :w] = lg.permute(0, 2, 3, 4, 1)
        lg = store[:, :, :, :w].permute(0, 4, 1, 2, 3)
        assert not lg.is_contiguous()
    rout = 1 if softmax else z.shape[1]
    out = torch.full((z.shape[0], rout, 3 * bins + 2), -7.0, dtype=torch.float64, device="cuda")     # written whole by the call
    if layout == "cl":
        ops.calibration_bins(channels_last_with_nan_pad(zg), lg, bins, out, softmax=softmax, scope=scope, logits_channels_last=True)
    else:
        ops.calibration_bins(zg, lg, bins, out, softmax=softmax, scope=scope)
    return out


HEADS = [(False, 1), (False, 3), (True, 2), (True, 4)]


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("softmax,R", HEADS, ids=lambda v: str(v))
def test_kernel_matches_the_float64_restatement(softmax, R, extent):
    for bins in BINS:
        z, lab = make_case(softmax, R, extent, bins)
        for scope in ("volume", "union"):
            want, n_el, abs_nll = reference(softmax, R, extent, bins, scope)
            for layout in ("cl", "ncdhw"):
                strided = layout == "cl" and bins == 15
                got = run_kernel(z, lab, softmax, bins, scope, layout, strided).cpu().numpy()
                assert_tables_agree(got, want, n_el, abs_nll, bins, f"softmax={softmax} R={R} {extent} bins={bins} {scope} {layout}")
            if not softmax and scope == "union":
                assert n_el[1, R - 1] == 0 and not want[1, R - 1].any()
    if not softmax:                                      # the exact zeros reached the kernel: c = 0.5 sits in bin 7 of 15
        assert (make_case(softmax, R, extent, 15)[0] == 0).any()


@pytest.mark.parametrize("softmax,R", [(False, 6), (True, 16)], ids=lambda v: str(v))
def test_kernel_beyond_four_channels(softmax, R):
    """More regions than one lane carries (sigmoid head: a second chunk with a tail) and the 16-class softmax kernel."""
    extent, bins = (5, 7, 9), 15
    z, lab = make_case(softmax, R, extent, bins)
    for scope in ("volume", "union"):
        want, n_el, abs_nll = reference(softmax, R, extent, bins, scope)
        for layout in ("cl", "ncdhw"):
            got = run_kernel(z, lab, softmax, bins, scope, layout).cpu().numpy()
            assert_tables_agree(got, want, n_el, abs_nll, bins, f"softmax={softmax} R={R} {scope} {layout}")


@pytest.mark.parametrize("softmax,R", [(False, 3), (True, 4)], ids=lambda v: str(v))
def test_kernel_is_reproducible_and_items_do_not_leak(softmax, R):
    """A second call gives the same bits; the table of items [0, 1] is the tables of item 0 and item 1 computed alone."""
    extent, bins = (24, 40, 33), 15
    z, lab = make_case(softmax, R, extent, bins)
    for scope in ("volume", "union"):
        for layout in ("cl", "ncdhw"):
            both = run_kernel(z, lab, softmax, bins, scope, layout)
            assert torch.equal(run_kernel(z, lab, softmax, bins, scope, layout), both)
            for i in range(N):
                alone = run_kernel(z[i:i + 1], lab[i:i + 1], softmax, bins, scope, layout)
                assert torch.equal(alone[0], both[i]), f"item {i} {scope} {layout}"


def test_ops_rejects_a_wrong_output_and_scope():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    z = torch.zeros((1, 3, 4, 4, 4), device="cuda")
    with pytest.raises(MmttaError, match="scope"):
        ops.calibration_bins(z, z, 15, torch.empty((1, 3, 47), dtype=torch.float64, device="cuda"), scope="band")
    with pytest.raises(MmttaError, match="out"):
        ops.calibration_bins(z, z, 15, torch.empty((1, 3, 46), dtype=torch.float64, device="cuda"))
    with pytest.raises(MmttaError, match="bins"):
        ops.calibration_bins(z, z, 65, torch.empty((1, 3, 197), dtype=torch.float64, device="cuda"))


# ----------------------------------------------------------------------------- end to end
E2E_BINS = 15
REGIONS = ["ET", "TC", "WT"]
NEW_SUFFIXES = ("_ece", "_brier", "_nll")


def _metrics_from_tables(tables):
    """Per-volume tables [V,R,3*bins+2] (numpy) -> the evaluator's keys, the formulas of the issue written out."""
    V, R, _ = tables.shape
    B = E2E_BINS
    per = {k: np.zeros((V, R)) for k in ("ece", "brier", "nll")}
    for v in range(V):
        for r in range(R):
            cnt, conf, cor = tables[v, r, 0:3 * B:3], tables[v, r, 1:3 * B:3], tables[v, r, 2:3 * B:3]
            n = cnt.sum()
            assert n > 0
            nz = cnt > 0
            per["ece"][v, r] = ((cnt[nz] / n) * np.abs(cor[nz] / cnt[nz] - conf[nz] / cnt[nz])).sum()
            per["brier"][v, r] = tables[v, r, 3 * B] / n
            per["nll"][v, r] = tables[v, r, 3 * B + 1] / n
    out = {}
    for k, val in per.items():
        means = val.mean(0)
        for name, m in zip(REGIONS, means):
            out[f"{name.lower()}_{k}"] = float(m)
        out[f"avg_{k}"] = float(means.mean())
    return out


# An fp32 confidence is within 4 ulp (2.4e-7) of the float64 one and its product with B <= 64 rounds once more (6e-8 of the
# value): an element further than 1e-6 from every edge falls into the same bin in fp32 and in float64.
EDGE_E2E = 1e-6


def _edge_elements(logits, bins):
    """[V,R,bins+1]: how many elements of a (volume, region) have their float64 confidence within EDGE_E2E of the edge k/B.
    The end to end runs score a model's own logits, which cannot be moved off the edges as the kernel tests move theirs: such
    an element may fall on either side in fp32, on the GPU as in any other fp32 evaluation of the formula."""
    c = _confidence(logits.astype(np.float64), False)
    amb = np.zeros(c.shape[:2] + (bins + 1,))
    for k in range(1, bins):
        amb[..., k] = (np.abs(c - k / bins) <= EDGE_E2E).reshape(c.shape[0], c.shape[1], -1).sum(-1)
    return amb


def _assert_cumulative(got, want, amb, what):
    """Bins [..., B, 3] = (count, conf, correct) compared through their running sums up to every edge k/B: exactly equal
    counts (confidence within count * 2^-21) at every edge no element sits on - the bound of the kernel tests, which is what
    remains when `amb` is zero - and within the number of elements on the edge elsewhere (a confidence is at most 1)."""
    cg, cw = got.cumsum(-2), want.cumsum(-2)
    on_edge = amb[..., 1:]                                # running sum j ends at edge (j + 1) / B
    for col in (0, 2):
        assert (np.abs(cg[..., col] - cw[..., col]) <= on_edge).all(), f"{what}: column {col}\n{got[..., col]}\n{want[..., col]}"
    assert (np.abs(cg[..., 1] - cw[..., 1]) <= cw[..., 0] * 2.0 ** -21 + on_edge).all(), f"{what}: confidence sums"
    assert (on_edge[..., -1] == 0).all() and np.array_equal(cg[..., -1, 0], cw[..., -1, 0])      # every element counted once


def _check_reported(strat, metrics, tables_got, logits, labels):
    """Raw rows against the restatement on the plugins' own logits, then every reported key against the restatement.

    Bounds: those of the kernel tests.  Where A elements of a (volume, region) sit within EDGE_E2E of a bin edge, each may be
    counted in either neighbouring bin; that moves its |correct - confidence| <= 1 between two terms of the ECE sum, so the
    ECE of that entry may differ by 2 A / n on top.  Brier and NLL do not depend on the bins."""
    B = E2E_BINS
    want, n_el, abs_nll = ref_table(logits, labels, False, B, "volume")
    amb = _edge_elements(logits, B)
    print("elements on a bin edge per (volume, region):", amb.sum(-1).tolist())
    V = want.shape[0]
    _assert_cumulative(tables_got[..., :3 * B].reshape(V, 3, B, 3), want[..., :3 * B].reshape(V, 3, B, 3), amb, "per-volume rows")
    assert (np.abs(tables_got[..., 3 * B] - want[..., 3 * B]) <= n_el * 2.0 ** -21).all(), "Brier sums"
    assert (np.abs(tables_got[..., 3 * B + 1] - want[..., 3 * B + 1]) <= 2.0 ** -20 * abs_nll + n_el * 2.0 ** -23).all(), "NLL sums"
    ref = _metrics_from_tables(want)
    bound = {"ece": float(2.0 ** -21 + (2.0 * amb.sum(-1) / n_el).max()), "brier": 2.0 ** -21,
             "nll": float((2.0 ** -20 * abs_nll / n_el).max() + 2.0 ** -23)}
    for key, w in ref.items():
        tol = bound[key.rsplit("_", 1)[1]]
        assert abs(metrics[key] - w) <= tol, (key, metrics[key], w, tol)
        assert abs(metrics[f"dom/synth/{key}"] - w) <= tol, key                 # one domain: the same figures under it
    rel = strat.last_reliability
    assert rel.dtype == torch.float64 and not rel.is_cuda and tuple(rel.shape) == (3, B, 3)
    _assert_cumulative(rel.numpy(), want[..., :3 * B].reshape(V, 3, B, 3).sum(0), amb.sum(0), "pooled reliability")


def _e2e_cfg(enable, **method):
    from test_hip_tta import SMALL, root_cfg
    cfg = root_cfg(SMALL, steps=2, lr=1e-3, tune_volumes=4, **method)
    cfg["dataset"]["synthetic"]["num_volumes"] = 3
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    cfg["evaluation"]["surface"] = {"enable": False, "asd_symmetric": False}
    cfg["evaluation"]["calibration"] = {"enable": enable, "bins": E2E_BINS, "scope": "volume"}
    return cfg


def test_seg_tta_eval_reports_calibration_of_the_adapted_logits():
    from multimodal_tta_amd.evaluation import table_width
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy, get_plugin
    from test_hip_tta import SMALL, build_pair

    runs = {}
    for enable in (True, False):
        cfg = _e2e_cfg(enable, lanes=2, group=2)
        _, hip = build_pair(SMALL)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_tta_eval")(cfg)
        runs[enable] = (strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat)
        assert strat.lanes == 2 and strat.group == 2
    (m_on, s_on), (m_off, s_off) = runs[True], runs[False]
    # disabled: the keys of today and nothing else, no table columns, nothing kept
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "miou", "jc", "loss", "dom/synth/avg_dc"} <= set(m_off)
    assert not any(k.endswith(NEW_SUFFIXES) for k in m_off)
    assert s_off.last_reliability is None and s_off.last_table.shape == (3, table_width(3))
    new = {f"{p}{r}{s}" for p in ("", "dom/synth/") for r in ("et", "tc", "wt", "avg") for s in NEW_SUFFIXES}
    assert set(m_on) == set(m_off) | new
    assert {k: m_on[k] for k in m_off} == m_off          # Dice, IoU and the loss do not move
    assert s_on.last_table.shape == (3, table_width(3, False, E2E_BINS))
    assert torch.equal(s_on.last_table[:, :table_width(3)], s_off.last_table)

    # the logits the plugin itself returns, one volume at a time
    _, hip = build_pair(SMALL)
    plug = get_plugin("entmin_tta")(_e2e_cfg(True)).setup(hip, "cuda")
    logits, labels = [], []
    for batch in loader:
        for i in range(batch["image"].shape[0]):
            logits.append(plug.logits(plug.adapt_volume(batch["image"][i:i + 1].cuda())).cpu().numpy())
            labels.append(batch["label"][i:i + 1].numpy())
    got = s_on.last_table[:, table_width(3):].reshape(3, 3, 3 * E2E_BINS + 2).numpy()
    _check_reported(s_on, m_on, got, np.concatenate(logits), np.concatenate(labels))


def test_seg_eval_reports_calibration_of_the_model_logits():
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair

    cfg = _e2e_cfg(True)
    cfg["training"]["eval_batch_size"] = 2
    _, hip = build_pair(SMALL)
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy("seg_eval")(cfg)
    m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    logits, labels = [], []
    with torch.no_grad():
        for batch in loader:
            logits.append(hip(batch["image"].cuda()).float().cpu().numpy())
            labels.append(batch["label"].numpy())
    logits, labels = np.concatenate(logits), np.concatenate(labels)
    from multimodal_tta_amd import ops
    out = torch.empty((3, 3, 3 * E2E_BINS + 2), dtype=torch.float64, device="cuda")
    ops.calibration_bins(torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda(), E2E_BINS, out)
    _check_reported(strat, m, out.cpu().numpy(), logits, labels)
    cfg_off = _e2e_cfg(False)
    s_off = get_evaluation_strategy("seg_eval")(cfg_off)
    off = s_off.evaluate_epoch(hip, get_dataset_builder("brats")(cfg_off).get_loader("test"), torch.device("cuda"))
    assert not any(k.endswith(NEW_SUFFIXES) for k in off) and s_off.last_reliability is None
    assert set(m) - set(off) == {f"{p}{r}{s}" for p in ("", "dom/synth/") for r in ("et", "tc", "wt", "avg") for s in NEW_SUFFIXES}
