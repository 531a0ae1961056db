"""Every optional block of the evaluation tail queued in ONE launch sequence (``queue_passes``), against runs that queue one
block at a time: a pass that read another pass's leftovers, or a column that slid, shows as a difference.

Both evaluators, the 3-volume synthetic loader at the speckle threshold (masks of many components), anisotropic spacing,
component filter + hole filling + an ET < TC < WT chain in every run.  The integer-derived blocks must agree exactly; HD95 /
ASD and the calibration within the bounds of their own end-to-end tests (tests/test_hip_surface.py,
tests/test_hip_calibration.py): nobody has measured whether those two are bit-stable between runs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SPACING = [1.5, 0.8, 2.0]
SD_TOL, LN_TOL = [1.0, 2.3], [0.5, 1.0]
EXACT = ["components", "fill_nest", "lesionwise", "lesionwise_hd95", "lesionwise_nsd", "surface_dice"]
SINGLES = ["surface", "lesionwise", "lesionwise_hd95", "lesionwise_nsd", "surface_dice", "calibration"]
OPTIONAL_OPS = ("components_filter", "fill_nest", "lesionwise_scores", "lesionwise_hd95", "lesionwise_nsd_after_scores",
                "surface_dice", "surface_distances", "calibration_bins")


def _cfg(blocks, threshold, postprocess=True, **method):
    """`blocks`: the names to switch on beside the post-processing (which brings components and fill_nest)."""
    from test_hip_calibration import E2E_BINS
    from test_hip_fill_holes import FILL, PP
    from test_hip_lesionwise import LW, _e2e_cfg
    lw = None
    if any(b.startswith("lesionwise") for b in blocks):
        lw = dict(LW, hd95={"enable": "lesionwise_hd95" in blocks}, nsd={"enable": "lesionwise_nsd" in blocks, "tolerances": LN_TOL})
    cfg = _e2e_cfg(lw, threshold, {**PP, **FILL} if postprocess else None, **method)
    ev = cfg["evaluation"]
    ev["seg"]["spacing"] = list(SPACING)
    ev["surface"] = {"enable": "surface" in blocks, "asd_symmetric": False}
    ev["calibration"] = {"enable": "calibration" in blocks, "bins": E2E_BINS, "scope": "volume"}
    ev["surface_dice"] = {"enable": "surface_dice" in blocks, "tolerances": SD_TOL}
    return cfg


def _run(kind, blocks, threshold, postprocess=True):
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair
    cfg = _cfg(blocks, threshold, postprocess, **(dict(lanes=2, group=2) if kind == "seg_tta_eval" else {}))
    cfg["training"]["eval_batch_size"] = 2
    _, hip = build_pair(SMALL)
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy(kind)(cfg)
    return strat.evaluate_epoch(hip, loader, torch.device("cuda")), strat, loader


def _count_calls(monkeypatch):
    from multimodal_tta_amd import ops
    calls = []
    for name in OPTIONAL_OPS:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    return calls


def _scored_logits(kind, threshold, loader):
    """The logits the evaluator scores, numpy [V,R,D,H,W]: the model's, or the plugin's after adapting each volume."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair
    _, hip = build_pair(SMALL)
    out = []
    with torch.no_grad():
        if kind == "seg_eval":
            hip.eval().to("cuda")
            return np.concatenate([hip(b["image"].cuda()).float().cpu().numpy() for b in loader])
        plug = get_plugin("entmin_tta")(_cfg([], threshold)).setup(hip, "cuda")
        for batch in loader:
            for i in range(batch["image"].shape[0]):
                out.append(plug.logits(plug.adapt_volume(batch["image"][i:i + 1].cuda())).cpu().numpy())
    return np.concatenate(out)


def _close_surface(got, want, what):          # the bound of tests/test_hip_surface.py's evaluator test
    assert abs(got - want) <= 2e-6 * abs(want) + 1e-7, (what, got, want)


@pytest.mark.parametrize("kind", ["seg_tta_eval", "seg_eval"])
def test_every_block_on_equals_each_block_alone(kind, monkeypatch):
    from test_hip_calibration import E2E_BINS, _assert_cumulative, _edge_elements, ref_table
    from test_hip_lesionwise import _speckle_threshold
    B = E2E_BINS
    thr = _speckle_threshold()
    calls = _count_calls(monkeypatch)
    m_off, s_off, _ = _run(kind, [], thr, postprocess=False)
    assert not calls, f"optional passes ran with every block off: {calls}"
    assert s_off.layout().slices == {}
    m_all, s_all, loader = _run(kind, SINGLES, thr)
    assert set(calls) == set(OPTIONAL_OPS)
    assert list(s_all.layout().slices) == ["surface"] + EXACT + ["calibration"]
    m_base, s_base, _ = _run(kind, [], thr)
    assert set(m_off) < set(m_base)
    singles = {name: _run(kind, [name], thr)[:2] for name in SINGLES}

    labels = np.concatenate([b["label"].numpy() for b in loader])
    logits = _scored_logits(kind, thr, loader)
    want_cal, n_el, abs_nll = ref_table(logits, labels, False, B, "volume")
    amb = _edge_elements(logits, B)
    cal_bound = {"ece": float(2.0 ** -21 + (2.0 * amb.sum(-1) / n_el).max()), "brier": 2.0 ** -21,
                 "nll": float((2.0 ** -20 * abs_nll / n_el).max() + 2.0 ** -23)}

    # the metric keys: Dice / IoU / loss and the post-processing figures from the base run, every other block from its own run
    seen = set(m_base)
    for k, v in m_base.items():
        assert m_all[k] == v, (k, m_all[k], v)
    for name, (m_one, s_one) in singles.items():
        own = set(m_one) - seen if name == "lesionwise" else set(m_one) - set(m_base) - set(singles["lesionwise"][0])
        assert own, name
        for k in own:
            if name == "surface":
                _close_surface(m_all[k], m_one[k], k)
            elif name == "calibration":
                assert abs(m_all[k] - m_one[k]) <= cal_bound[k.rsplit("_", 1)[1]], (k, m_all[k], m_one[k])
            else:
                assert m_all[k] == m_one[k], (name, k, m_all[k], m_one[k])
        for k in set(m_one) - own:                 # what the single run shares with the base run does not move either
            assert m_all[k] == m_one[k], (name, k)
        seen |= own
    assert set(m_all) == seen
    if kind == "seg_eval":                        # keeps no table in one process
        return

    # the table, block by block
    t_all, sl_all = s_all.last_table, s_all.layout().slices
    assert t_all.shape == (3, s_all.layout().width) and torch.equal(t_all[:, :12], s_base.last_table[:, :12])
    for name in ("components", "fill_nest"):
        assert torch.equal(t_all[:, sl_all[name]], s_base.last_table[:, s_base.layout().slices[name]]), name
    for name, (m_one, s_one) in singles.items():
        t_one, sl_one = s_one.last_table, s_one.layout().slices
        assert torch.equal(t_one[:, :12], t_all[:, :12]), name
        for block in sl_one:
            a, b = t_all[:, sl_all[block]], t_one[:, sl_one[block]]
            if block == "surface":
                for x, y in zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()):
                    _close_surface(x, y, block)
            elif block == "calibration":
                a, b = a.reshape(3, 3, 3 * B + 2).numpy(), b.reshape(3, 3, 3 * B + 2).numpy()
                _assert_cumulative(a[..., :3 * B].reshape(3, 3, B, 3), b[..., :3 * B].reshape(3, 3, B, 3), amb, "all vs alone")
                assert (np.abs(a[..., 3 * B] - b[..., 3 * B]) <= n_el * 2.0 ** -21).all(), "Brier sums"
                assert (np.abs(a[..., 3 * B + 1] - b[..., 3 * B + 1]) <= 2.0 ** -20 * abs_nll + n_el * 2.0 ** -23).all(), "NLL sums"
            else:
                assert torch.equal(a, b), (name, block, a, b)
