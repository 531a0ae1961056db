"""The evaluation tail's block table (``evaluation.BLOCKS``) against values recorded before it existed.

``tests/golden/eval_blocks.json`` holds, for tables from a seeded generator and every switch combination below, the row width
and the metrics as ordered ``[key, value]`` pairs, as the commit named in the fixture computed them through the keyword API
that both commits share.  JSON round-trips doubles exactly, so every comparison here is ``==``.  The second half runs a
``seg_eval`` whose device passes are replaced by fixed host tensors, every block on, in one process and under two gloo
ranks.  (``python tests/test_eval_blocks_host.py OUT.json`` writes the table half of the fixture anew.)"""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from multimodal_tta_amd.evaluation import (SegmentationEvaluationStrategy, lesionwise_columns, lesionwise_hd95_columns,  # noqa: E402
                                           lesionwise_nsd_columns, metrics_from_table, surface_dice_columns, table_width)

GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_blocks.json")
REGIONS = {2: ["ET", "WT"], 3: ["ET", "TC", "WT"]}
DOMAINS = ["a", ""]          # the second one is reported as "unknown"
VOLUMES, BINS, PENALTY = 5, 4, 100.0
SD_T, LN_T = [0.5, 2.0], [1.0]
Q30, Q20 = 1 << 30, 1 << 20

ALL = dict(surface=True, bins=BINS, components=True, lesionwise=True, fill_nest=True, lesionwise_hd95=True, surface_dice=SD_T,
           lesionwise_nsd=LN_T)
COMBOS = {"off": {}, "surface": dict(surface=True), "components": dict(components=True), "fill_nest": dict(fill_nest=True),
          "lesionwise": dict(lesionwise=True), "lesionwise_hd95": dict(lesionwise=True, lesionwise_hd95=True),
          "lesionwise_nsd": dict(lesionwise=True, lesionwise_nsd=LN_T), "surface_dice": dict(surface_dice=SD_T),
          "calibration": dict(bins=BINS), "all": ALL, "all_softmax": dict(ALL, calibration_regions=["all"])}
# (combination, R, report_loss): nothing on and everything on at R = 2 and R = 3, a block alone at one of them in turn; with
# and without the loss.  (Every further case costs the fixture up to 10 KB.)
SINGLES = [name for name in COMBOS if name not in ("off", "all", "all_softmax")]
CASES = ([("off", R, loss) for R in (2, 3) for loss in (False, True)] +
         [(name, 2 + k % 2, k % 4 < 2) for k, name in enumerate(SINGLES)] +
         [("all", 2, True), ("all", 3, False), ("all_softmax", 2, False), ("all_softmax", 3, True)])


def _width(R, sw):
    kw = {k: v for k, v in sw.items() if k not in ("calibration_regions", "surface_dice", "lesionwise_nsd")}
    return table_width(R, rout=len(sw["calibration_regions"]) if "calibration_regions" in sw else None,
                       surface_dice=len(sw.get("surface_dice", ())), lesionwise_nsd=len(sw.get("lesionwise_nsd", ())), **kw)


def make_table(R, sw, seed):
    """VOLUMES rows in the documented column order: index, domain, loss, dice, iou, valid, then HD95 / ASD, components,
    fill / nest, lesion-wise, lesion-wise HD95, lesion-wise NSD, region-wise NSD, calibration - those that ``sw`` enables."""
    rng = np.random.default_rng(seed)
    ints = lambda hi, *shape: torch.from_numpy(rng.integers(0, hi, shape))
    f32 = lambda scale: torch.from_numpy((rng.random(R) * scale).astype(np.float32)).double()
    rout = len(sw.get("calibration_regions", REGIONS[R]))
    rows = []
    for i in range(VOLUMES):
        valid = ints(2, R).double()
        if i == 2:
            valid[R - 1] = 0.0
        if i == 0:
            valid[:] = 1.0
        parts = [torch.tensor([i, i % 2, rng.random()], dtype=torch.float64), f32(1.0), f32(1.0), valid]
        hd, asd = f32(40.0), f32(10.0)
        comp, fill = ints(9, R, 3), ints(50, R, 4)
        st = ints(5, R, 7)                        # lesions, kept, found, components, matched, dice_q, fp voxels
        st[:, 2] = torch.minimum(st[:, 2], st[:, 1])
        st[:, 4] = torch.minimum(st[:, 4], st[:, 3])
        st[:, 5] = torch.from_numpy(rng.integers(0, Q30, R)) * st[:, 2]
        if i == 3:
            st[0] = 0                             # nothing to find, nothing predicted: undefined
        hs = torch.stack([ints(60 * Q20, R), st[:, 2], torch.zeros(R, dtype=torch.int64)], dim=1)
        if i == 1:
            hs[0, 2] = 3                          # the region's surface lists overflowed: state -1
        ln = torch.from_numpy(rng.integers(0, Q30, (R, len(LN_T)))) * st[:, 2:3]
        edges = ints(40, R, len(SD_T), 2)
        hits = torch.minimum(ints(40, R, len(SD_T), 2), edges)
        sd = torch.stack([hits[..., 0], edges[..., 0], hits[..., 1], edges[..., 1]], dim=-1)
        cnt = ints(30, rout, BINS).double()
        if i == 4:
            cnt[0] = 0.0                          # an entry without elements
        conf = cnt * torch.from_numpy(rng.random((rout, BINS)))
        cor = torch.floor(cnt * torch.from_numpy(rng.random((rout, BINS))))
        n = cnt.sum(-1, keepdim=True)
        cal = torch.cat([torch.stack([cnt, conf, cor], -1).reshape(rout, -1), n * rng.random(), n * rng.random()], dim=1)
        if sw.get("surface"):
            parts += [hd, asd]
        if sw.get("components"):
            parts.append(SegmentationEvaluationStrategy.component_columns(comp))
        if sw.get("fill_nest"):
            parts.append(SegmentationEvaluationStrategy.fill_nest_columns(fill))
        if sw.get("lesionwise"):
            parts.append(lesionwise_columns(st))
        if sw.get("lesionwise_hd95"):
            parts.append(lesionwise_hd95_columns(st, hs, PENALTY))
        if sw.get("lesionwise_nsd"):
            parts.append(lesionwise_nsd_columns(st, ln))
        if sw.get("surface_dice"):
            parts.append(surface_dice_columns(sd))
        if sw.get("bins"):
            parts.append(cal.reshape(-1))
        rows.append(torch.cat(parts))
    return torch.stack(rows)


def compute_cases():
    out = {}
    for k, (name, R, loss) in enumerate(CASES):
        sw = COMBOS[name]
        table = make_table(R, sw, 100 + k)
        m = metrics_from_table(table, REGIONS[R], DOMAINS, loss, **sw)
        out[f"{name}/R{R}/{'loss' if loss else 'noloss'}"] = {"width": _width(R, sw), "rows": list(table.shape),
                                                              "metrics": [[key, v] for key, v in m.items()]}
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_generator_covers_the_edge_states():
    table = make_table(3, ALL, 7)
    w = _width(3, {}) + 6 + 9 + 12 + 21
    assert (table[:, w + 3:w + 6] == -1.0).any() and (table[:, w + 3:w + 6] == 0.0).any() and (table[:, w + 3:w + 6] == 1.0).any()
    assert set(table[:, 9:12].reshape(-1).tolist()) == {0.0, 1.0} and set(table[:, 1].tolist()) == {0.0, 1.0}
    assert (table[:, -3 * (3 * BINS + 2):] >= 0.0).all() and table.shape == (VOLUMES, _width(3, ALL))


def test_tables_give_the_recorded_metrics(golden):
    got = compute_cases()
    assert list(got) == list(golden["cases"]) and len(got) == len(CASES) == len(set(CASES))
    for case, want in golden["cases"].items():
        assert got[case]["width"] == want["width"] and got[case]["rows"] == want["rows"] == [VOLUMES, want["width"]], case
        keys = [k for k, _ in got[case]["metrics"]]
        assert keys == [k for k, _ in want["metrics"]], case
        assert got[case]["metrics"] == want["metrics"], [(a, b) for a, b in zip(got[case]["metrics"], want["metrics"]) if a != b]
    on = dict(golden["cases"]["all/R3/noloss"]["metrics"])
    assert {"avg_hd95", "avg_components", "wt_nested_voxels", "avg_lw_dc", "avg_lw_hd95", "et_lw_hd95_overflow", "avg_lw_nsd_1",
            "avg_nsd_0.5", "avg_nsd_2", "avg_ece", "dom/unknown/avg_nll", "dom/a/et_dc"} <= set(on)
    assert "all_ece" in dict(golden["cases"]["all_softmax/R2/noloss"]["metrics"])
    assert dict(golden["cases"]["off/R3/loss"]["metrics"])["loss"] > 0.0


# ----------------------------------------------------------------------------- seg_eval, every block on, passes stubbed
EVAL_REGIONS = ["ET", "TC", "WT"]
EVAL_SD_T, EVAL_LN_T = [0.5, 1.0], [1.0]


def stub_outputs(strat, logits, y):
    """Fixed host tensors for every pass of one batch, a function of each volume alone (seeded by its label sum), so a
    volume gets the same figures in whatever batch or rank it is scored."""
    B, R = y.shape[0], y.shape[1]
    pred, gt = torch.sigmoid(logits) >= strat.threshold, y > 0.5
    out = {"counts": torch.stack([(pred & gt).flatten(2).sum(-1), pred.flatten(2).sum(-1), gt.flatten(2).sum(-1)], -1).to(torch.int64)}
    per = {k: [] for k in ("components", "fill_nest", "lesionwise", "lesionwise_hd95", "lesionwise_nsd", "surface_dice", "hd", "asd",
                           "calibration", "loss")}
    rout, bins = len(strat.calibration_regions), strat.calibration_bins
    for b in range(B):
        rng = np.random.default_rng(int(y[b].sum().item()))
        ints = lambda hi, *shape: torch.from_numpy(rng.integers(0, hi, shape))
        per["components"].append(ints(9, R, 3))
        per["fill_nest"].append(ints(50, R, 4))
        st = ints(5, R, 7)
        st[:, 2], st[:, 4] = torch.minimum(st[:, 2], st[:, 1]), torch.minimum(st[:, 4], st[:, 3])
        st[:, 5] = torch.from_numpy(rng.integers(0, Q30, R)) * st[:, 2]
        per["lesionwise"].append(st)
        per["lesionwise_hd95"].append(torch.stack([ints(60 * Q20, R), st[:, 2], (ints(4, R) == 0).to(torch.int64)], dim=1))
        per["lesionwise_nsd"].append(torch.from_numpy(rng.integers(0, Q30, (R, len(EVAL_LN_T)))) * st[:, 2:3])
        edges = ints(40, R, len(EVAL_SD_T), 2)
        hits = torch.minimum(ints(40, R, len(EVAL_SD_T), 2), edges)
        per["surface_dice"].append(torch.stack([hits[..., 0], edges[..., 0], hits[..., 1], edges[..., 1]], dim=-1))
        per["hd"].append(torch.from_numpy((rng.random(R) * 40).astype(np.float32)))
        per["asd"].append(torch.from_numpy((rng.random(R) * 10).astype(np.float32)))
        cnt = ints(30, rout, bins).double()
        n = cnt.sum(-1, keepdim=True)
        per["calibration"].append(torch.cat([torch.stack([cnt, cnt * torch.from_numpy(rng.random((rout, bins))),
                                                          torch.floor(cnt * 0.5)], -1).reshape(rout, -1), n * 0.2, n * 0.6], dim=1))
        p, t = torch.sigmoid(logits[b].double()).flatten(1), y[b].double().flatten(1)
        ce = torch.nn.functional.binary_cross_entropy_with_logits(logits[b].double(), y[b].double(), reduction="sum")
        per["loss"].append(torch.cat([torch.stack([(p * t).sum(-1), p.sum(-1), t.sum(-1)], -1).reshape(-1), ce.reshape(1)]))
    out.update({k: torch.stack(v) for k, v in per.items()})
    out["loss"] = (out["loss"].reshape(-1), B, R, y[0, 0].numel())
    return out


class _CpuAllBlocks:
    """The strategy's host logic is the product code; what the GPU passes would leave is ``stub_outputs``."""

    def queue_passes(self, logits, y, channels_last=False):
        o = stub_outputs(self, logits, y)
        raw = {k: o[k] for k in ("components", "fill_nest", "lesionwise", "lesionwise_hd95", "lesionwise_nsd", "surface_dice",
                                 "calibration")}
        raw["surface"] = (o["hd"], o["asd"])
        job = {"counts": o["counts"], "shape": tuple(y.shape[2:]), "raw": raw, "penalty": self.lesionwise_hd95_penalty_mm(y.shape[2:])}
        if self.report_loss:
            job["loss"] = o["loss"]
        return job


def eval_cfg(report_loss):
    return {"evaluation": {"seg": {"threshold": 0.5, "region_order": EVAL_REGIONS, "spacing": [1.0, 1.0, 1.0]},
                           "loss": {"report_loss": report_loss}, "surface": {"enable": True},
                           "calibration": {"enable": True, "bins": BINS},
                           "postprocess": {"enable": True, "fill_holes": True, "nesting": ["ET", "WT"]},
                           "lesionwise": {"enable": True, "hd95": {"enable": True, "penalty": 55.0},
                                          "nsd": {"enable": True, "tolerances": EVAL_LN_T}},
                           "surface_dice": {"enable": True, "tolerances": EVAL_SD_T}},
            "dataset": {"synthetic": {"enabled": True}}}


def _setup(report_loss=False):
    class Strat(_CpuAllBlocks, SegmentationEvaluationStrategy):
        pass

    torch.manual_seed(3)
    return Strat(eval_cfg(report_loss)), torch.nn.Conv3d(2, len(EVAL_REGIONS), 1)


def _worker(rank, world, port, n, out_dir, shards):
    import torch.distributed as dist
    from test_shard import _batches, _eval_volumes
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    strat, model = _setup()
    metrics = strat.evaluate_epoch(model, _batches(_eval_volumes(n), shards[rank], 2), "cpu")
    with open(os.path.join(out_dir, f"m{rank}.json"), "w") as fh:
        json.dump(metrics, fh)
    torch.save(strat.last_table, os.path.join(out_dir, f"tab{rank}.pt"))
    torch.save(strat.last_reliability, os.path.join(out_dir, f"rel{rank}.pt"))
    dist.destroy_process_group()


ALL_WIDTH = dict(surface=True, bins=BINS, components=True, lesionwise=True, fill_nest=True, lesionwise_hd95=True,
                 surface_dice=len(EVAL_SD_T), lesionwise_nsd=len(EVAL_LN_T))


@pytest.mark.parametrize("shards", [[[0, 2, 4], [1, 3]], [[0, 1, 2, 3, 4], []]])
def test_sharded_seg_eval_with_every_block_equals_one_process(tmp_path, shards):
    import socket

    import torch.multiprocessing as mp
    from test_shard import _batches, _eval_volumes
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    n, world, R = 5, 2, len(EVAL_REGIONS)
    strat, model = _setup()
    want = strat.evaluate_epoch(model, _batches(_eval_volumes(n), list(range(n)), 2), "cpu")
    assert {"avg_hd95", "avg_components", "et_holes", "avg_lw_dc", "avg_lw_hd95", "avg_lw_nsd_1", "avg_nsd_0.5", "avg_ece",
            "dom/siteC/wt_nsd_1"} <= set(want)
    assert sum(want[f"{r.lower()}_lw_hd95_overflow"] for r in EVAL_REGIONS) > 0.0
    mp.spawn(_worker, args=(world, port, n, str(tmp_path), shards), nprocs=world, join=True)
    tabs = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), f"m{r}.json")) as fh:
            got = json.load(fh)
        assert got == want and list(got) == list(want), f"rank {r}: {got} vs {want}"
        tabs.append(torch.load(os.path.join(str(tmp_path), f"tab{r}.pt"), weights_only=True))
        assert torch.equal(torch.load(os.path.join(str(tmp_path), f"rel{r}.pt"), weights_only=True), strat.last_reliability)
    assert torch.equal(tabs[0], tabs[1]) and tabs[0].shape == (n, table_width(R, **ALL_WIDTH)) and strat._table_width() == tabs[0].shape[1]
    again = metrics_from_table(tabs[0], EVAL_REGIONS, ["siteA", "siteB", "siteC"], False, **dict(ALL_WIDTH, surface_dice=EVAL_SD_T,
                                                                                                lesionwise_nsd=EVAL_LN_T))
    assert again == want and list(again) == list(want)


def test_single_process_loss_is_the_batch_value_times_the_batch_size(golden):
    """Batch size 2 over 5 volumes: the reported loss is sum(batch value * batch size) / 5, what the recorded commit gives,
    and every other key is what the run without the loss gives."""
    from test_shard import _batches, _eval_volumes
    strat, model = _setup(report_loss=True)
    got = strat.evaluate_epoch(model, _batches(_eval_volumes(5), list(range(5)), 2), "cpu")
    assert got["loss"] == golden["seg_eval_loss"] and got["loss"] > 0.0
    plain, model = _setup()
    base = plain.evaluate_epoch(model, _batches(_eval_volumes(5), list(range(5)), 2), "cpu")
    assert dict(got, loss=0.0) == base and list(got) == list(base)


if __name__ == "__main__":
    with open(sys.argv[1], "w") as fh:
        json.dump({"cases": compute_cases()}, fh, separators=(",", ":"))
