"""Lesion-wise scores, everything that needs no GPU: the config block, the widened per-volume table and its replay, the
argument checks of the C entry point and a sharded run over gloo."""
import ctypes

import pytest
import torch

from multimodal_tta_amd.evaluation import (RegionAccumulator, SegmentationEvaluationStrategy, lesionwise_columns,
                                           lesionwise_config, metrics_from_table, table_width)

REGIONS = ["ET", "TC", "WT"]
Q1 = 1 << 30


def _cfg(regions=None, **lw):
    cfg = {"evaluation": {"lesionwise": dict(lw)}}
    if regions is not None:
        cfg["evaluation"]["seg"] = {"region_order": list(regions)}
    return cfg


# ----------------------------------------------------------------------------- config
def test_config_defaults_and_per_region_lists():
    assert lesionwise_config({}) == (False, 3, 18, [0, 0, 0])
    assert lesionwise_config(_cfg(regions=["gtvt"])) == (False, 3, 18, [0])
    assert lesionwise_config(_cfg(enable=True, dilation=0, dilation_connectivity=6, min_lesion_voxels=7)) == (True, 0, 6, [7, 7, 7])
    assert lesionwise_config(_cfg(dilation=8, dilation_connectivity=26, min_lesion_voxels=[0, 5, 50])) == (False, 8, 26, [0, 5, 50])
    off = SegmentationEvaluationStrategy({})
    assert not off.enable_lesionwise and off.lesionwise_dilation == 3 and off.lesionwise_connectivity == 18
    on = SegmentationEvaluationStrategy(_cfg(enable=True, min_lesion_voxels=[1, 2, 3]))
    assert on.enable_lesionwise and on.lesionwise_min_voxels == [1, 2, 3]


@pytest.mark.parametrize("lw,key", [
    (dict(enable="on"), "evaluation.lesionwise.enable"),
    (dict(dilation=9), "evaluation.lesionwise.dilation"),
    (dict(dilation=-1), "evaluation.lesionwise.dilation"),
    (dict(dilation=True), "evaluation.lesionwise.dilation"),
    (dict(dilation=1.5), "evaluation.lesionwise.dilation"),
    (dict(dilation_connectivity=7), "evaluation.lesionwise.dilation_connectivity"),
    (dict(dilation_connectivity=True), "evaluation.lesionwise.dilation_connectivity"),
    (dict(min_lesion_voxels=-1), "evaluation.lesionwise.min_lesion_voxels"),
    (dict(min_lesion_voxels=[1, 2]), "evaluation.lesionwise.min_lesion_voxels"),
    (dict(min_lesion_voxels=[0, -3, 0]), "evaluation.lesionwise.min_lesion_voxels"),
    (dict(min_lesion_voxels=2.5), "evaluation.lesionwise.min_lesion_voxels"),
    (dict(min_lesion_voxels="5"), "evaluation.lesionwise.min_lesion_voxels"),
])
def test_config_bad_values_name_their_key(lw, key):
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + r"\b"):
        lesionwise_config(_cfg(**lw))
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + r"\b"):
        SegmentationEvaluationStrategy(_cfg(**lw))


def test_softmax_head_is_refused_by_name():
    cfg = _cfg(enable=True)
    cfg["training"] = {"criterion": {"softmax": True}}
    with pytest.raises(NotImplementedError, match=r"evaluation\.lesionwise"):
        SegmentationEvaluationStrategy(cfg)
    cfg["evaluation"]["lesionwise"]["enable"] = False
    assert not SegmentationEvaluationStrategy(cfg).enable_lesionwise


def test_shipped_configs_carry_the_block_disabled():
    from multimodal_tta_amd.config import compose
    for task, R in (("brats", 3), ("hecktor21", 1)):
        cfg = compose(overrides=[f"task={task}", "model=unet"])
        assert dict(cfg["evaluation"]["lesionwise"]) == {"enable": False, "dilation": 3, "dilation_connectivity": 18,
                                                         "min_lesion_voxels": 0}
        assert lesionwise_config(cfg) == (False, 3, 18, [0] * R)


# ----------------------------------------------------------------------------- table layout and replay
def test_table_width_places_the_lesionwise_columns():
    R = 2
    for surface in (False, True):
        base = table_width(R, surface)
        assert base == 3 + (5 if surface else 3) * R                          # today's layout
        assert table_width(R, surface, lesionwise=False) == base
        assert table_width(R, surface, lesionwise=True) == base + 7 * R
        assert table_width(R, surface, components=True) == base + 3 * R
        assert table_width(R, surface, components=True, lesionwise=True) == base + 10 * R
        assert table_width(R, surface, 4, lesionwise=True) == table_width(R, surface, 4) + 7 * R
        assert table_width(R, surface, 4, 1, components=True, lesionwise=True) == table_width(R, surface, 4, 1) + 10 * R


def test_columns_of_one_volume():
    # lesions, kept, found, predicted, matched, dice_q, fp voxels
    stats = torch.tensor([[3, 2, 1, 4, 1, Q1 // 2, 9],        # 2 kept + 3 false positives: 0.5 / 5
                          [0, 0, 0, 2, 0, 0, 5],               # GT-empty with false positives: valid, 0
                          [0, 0, 0, 0, 0, 0, 0],               # nothing to find, nothing predicted: invalid
                          [1, 0, 0, 1, 1, 0, 0]],              # the only lesion is below min_lesion_voxels, its component matched: invalid
                         dtype=torch.int64)
    c = lesionwise_columns(stats).reshape(7, 4)
    assert c.dtype == torch.float64
    assert c[0].tolist() == [0.5 / 5, 0.0, 0.0, 0.0] and c[1].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert c[2].tolist() == [2.0, 0.0, 0.0, 0.0] and c[3].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert c[4].tolist() == [3.0, 2.0, 0.0, 0.0] and c[5].tolist() == [1.0, 0.0, 0.0, 1.0] and c[6].tolist() == [4.0, 2.0, 0.0, 1.0]
    # a dice_q beyond 2^53 / volumes never reaches the table raw: the score is formed from the integers
    big = torch.tensor([[5000, 5000, 5000, 5000, 5000, 5000 * Q1 - 1, 0]], dtype=torch.int64)
    assert lesionwise_columns(big)[0].item() == float(5000 * Q1 - 1) / float(Q1) / 5000.0


def _hand_rows(surface, bins, components):
    """Three volumes, two regions (A, B), domains d0 / d1 / d0.  Per (volume, region) the seven integers of the kernel."""
    stats = [[[2, 2, 1, 3, 1, Q1 // 2, 7], [0, 0, 0, 0, 0, 0, 0]],        # A: 0.5 / (2 + 2); B: invalid
             [[1, 1, 1, 1, 1, Q1, 0], [0, 0, 0, 2, 0, 0, 11]],            # A: 1 / 1; B: GT-empty with 2 false positives: 0, counts
             [[3, 1, 0, 0, 0, 0, 0], [1, 1, 1, 2, 2, Q1 // 4, 0]]]        # A: 0 / 1 (missed); B: 0.25 / 1
    doms = [0, 1, 0]
    rows = []
    for i in range(3):
        row = [float(i), float(doms[i]), 0.25 * (i + 1), 0.5 + 0.1 * i, 0.7, 0.4, 0.5, 1.0, 1.0 if i != 1 else 0.0]
        if surface:
            row += [2.0 + i, 3.0, 1.0, 0.5 + i]
        if components:
            row += [3.0, 1.0, 1.0, 1.0, 40.0 * i, 0.0]
        mark = len(row)
        row += lesionwise_columns(torch.tensor(stats[i], dtype=torch.int64)).tolist()
        if bins:
            for r in range(2):
                row += [0.0] * (3 * (bins - 1)) + [10.0, 9.0, 8.0 + r, 1.0, 2.0]
        rows.append(row)
    return torch.tensor(rows, dtype=torch.float64), mark


WANT = {"a_lw_dc": (0.125 + 1.0 + 0.0) / 3, "b_lw_dc": (0.0 + 0.25) / 2,
        "a_lesions": 4.0 / 3, "b_lesions": 1.0 / 3, "a_lesions_found": 2.0 / 3, "b_lesions_found": 1.0 / 3,
        "a_fp_components": 2.0 / 3, "b_fp_components": 2.0 / 3,
        "a_lesion_recall": 2.0 / 4.0, "b_lesion_recall": 1.0, "a_lesion_precision": 2.0 / 4.0, "b_lesion_precision": 2.0 / 4.0,
        "dom/d0/a_lw_dc": (0.125 + 0.0) / 2, "dom/d0/b_lw_dc": 0.25, "dom/d0/a_lesions": 1.5, "dom/d0/b_lesions": 0.5,
        "dom/d0/a_lesions_found": 0.5, "dom/d0/b_lesions_found": 0.5, "dom/d0/a_fp_components": 1.0, "dom/d0/b_fp_components": 0.0,
        "dom/d0/a_lesion_recall": 1.0 / 3.0, "dom/d0/b_lesion_recall": 1.0, "dom/d0/a_lesion_precision": 1.0 / 3.0,
        "dom/d0/b_lesion_precision": 1.0,
        "dom/d1/a_lw_dc": 1.0, "dom/d1/b_lw_dc": 0.0, "dom/d1/a_lesions": 1.0, "dom/d1/b_lesions": 0.0,
        "dom/d1/a_lesions_found": 1.0, "dom/d1/b_lesions_found": 0.0, "dom/d1/a_fp_components": 0.0, "dom/d1/b_fp_components": 2.0,
        "dom/d1/a_lesion_recall": 1.0, "dom/d1/a_lesion_precision": 1.0, "dom/d1/b_lesion_precision": 0.0}
WANT["avg_lw_dc"] = (WANT["a_lw_dc"] + WANT["b_lw_dc"]) / 2
WANT["dom/d0/avg_lw_dc"] = (WANT["dom/d0/a_lw_dc"] + WANT["dom/d0/b_lw_dc"]) / 2
WANT["dom/d1/avg_lw_dc"] = (1.0 + 0.0) / 2          # B of d1 is GT-empty with false positives: it enters the mean with 0


@pytest.mark.parametrize("components", [False, True])
@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("bins", [0, 4])
def test_metrics_from_table_reads_the_lesionwise_columns(surface, bins, components):
    regions = ["A", "B"]
    table, mark = _hand_rows(surface, bins, components)
    assert table.shape[1] == table_width(2, surface, bins, components=components, lesionwise=True)
    assert mark == table_width(2, surface, components=components)             # behind the component columns ...
    assert table.shape[1] - (mark + 14) == table_width(2, False, bins) - table_width(2)      # ... before the calibration block
    m = metrics_from_table(table, regions, ["d0", "d1"], True, surface, bins, components=components, lesionwise=True)
    for k, v in WANT.items():
        assert m[k] == v, (k, m[k], v)
    assert "dom/d1/b_lesion_recall" not in m                                  # no kept lesion in d1's region B: absent
    # the other keys are those of the same table without the lesion-wise columns
    plain = torch.cat([table[:, :mark], table[:, mark + 14:]], 1)
    base = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, bins, components=components)
    assert {k: m[k] for k in base} == base and set(m) == set(base) | set(WANT)
    # the accumulator fed row by row gives the same
    acc = RegionAccumulator(regions, surface, bins, None, components, True)
    assert acc.lesionwise


def test_without_the_keyword_nothing_changes():
    regions = ["A", "B"]
    for surface in (False, True):
        table, mark = _hand_rows(surface, 0, False)
        plain = table[:, :mark]
        a = metrics_from_table(plain, regions, ["d0", "d1"], True, surface)
        b = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, lesionwise=False)
        assert a == b and list(a) == list(b) and not any("lw_dc" in k or "lesion" in k or "fp_components" in k for k in a)
        assert not RegionAccumulator(regions, surface).lesionwise


def test_zero_denominators_leave_keys_out():
    regions = ["A", "B"]
    acc = RegionAccumulator(regions, lesionwise=True)
    cols = lesionwise_columns(torch.tensor([[0, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0]], dtype=torch.int64))
    acc.add_row([0.5, 0.5], [0.4, 0.4], [True, True], "d", lesionwise=cols)
    m = acc.metrics(False)
    for k in ("a_lesion_recall", "a_lesion_precision", "b_lesion_recall", "b_lesion_precision"):
        assert k not in m and f"dom/d/{k}" not in m
    assert m["a_lw_dc"] == 0.0 and m["avg_lw_dc"] == 0.0 and m["a_lesions"] == 0.0 and m["b_fp_components"] == 0.0


# ----------------------------------------------------------------------------- the C entry point, without a device
def test_abi_symbols_and_argument_validation_without_a_gpu():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    assert {"mmtta_lesionwise_scratch_bytes", "mmtta_lesionwise_scores"} <= set(_lib.exported_names())
    assert lib.mmtta_abi_version() == 2

    def call(mask=1, label=True, n=1, r=1, d=4, h=4, w=4, it=3, conn=18, stats=1, scratch=1, min_voxels=None, dtype=None):
        mv = (ctypes.c_int64 * 64)(*(min_voxels or [0] * 64))
        t = _lib.Tensor(4096, n, r, d, h, w, r * d * h * w, d * h * w, h * w, w, 1, _lib.F32 if dtype is None else dtype, 0)
        return lib.mmtta_lesionwise_scores(mask, ctypes.byref(t) if label else None, n, r, d, h, w, it, conn, mv, stats, None,
                                           scratch, None)

    # (the pointers here are never followed: every call is refused before anything is queued)
    assert call(mask=None) == -1 and b"null" in lib.mmtta_last_error()
    assert call(label=False) == -1 and b"null" in lib.mmtta_last_error()
    assert call(stats=None) == -1 and call(scratch=None) == -1
    assert call(it=9) == -1 and b"iterations 9" in lib.mmtta_last_error()
    assert call(it=-1) == -1 and b"iterations" in lib.mmtta_last_error()
    assert call(conn=7) == -1 and b"connectivity 7" in lib.mmtta_last_error()
    assert call(r=65) == -2 and b"65" in lib.mmtta_last_error()
    assert call(d=0) == -1 and b"extent" in lib.mmtta_last_error()
    assert call(d=2048, h=2048, w=512) == -2 and b"2^31" in lib.mmtta_last_error()
    assert call(n=2, d=1, h=1, w=2 ** 31 - 2) == -2 and b"split the batch" in lib.mmtta_last_error()
    assert call(min_voxels=[-5] + [0] * 63) == -1 and b"min_lesion_voxels" in lib.mmtta_last_error()
    assert call(dtype=_lib.BF16) == -2 and b"fp32" in lib.mmtta_last_error()


def test_scratch_bytes():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    V = 128 ** 3
    nb = lib.mmtta_lesionwise_scratch_bytes(6, 128, 128, 128)
    # two label volumes, four per-root counters, two byte planes; the pair table adds 2 * 64^3 slots of 8 bytes per mask
    assert nb >= 6 * (V * 26 + 2 * 64 ** 3 * 8)
    assert nb < 6 * V * 32
    assert lib.mmtta_lesionwise_scratch_bytes(1, 1, 1, 5) > 0
    assert lib.mmtta_lesionwise_scratch_bytes(1, 2048, 2048, 512) < 0
    assert lib.mmtta_lesionwise_scratch_bytes(2, 1, 1, 2 ** 31 - 2) < 0
    assert lib.mmtta_lesionwise_scratch_bytes(0, 4, 4, 4) < 0
    assert lib.mmtta_lesionwise_scratch_bytes(1, 0, 4, 4) < 0
    assert lib.mmtta_lesionwise_scratch_bytes(1, 2 ** 40, 2 ** 40, 2 ** 40) < 0


def test_ops_wrapper_checks_before_the_library():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    with pytest.raises(MmttaError, match="uint8"):
        ops.lesionwise_scores(torch.zeros((1, 1, 2, 2, 2), dtype=torch.float32), torch.zeros((1, 1, 2, 2, 2)))
    with pytest.raises(MmttaError, match="dense"):
        ops.lesionwise_scores(torch.zeros((1, 1, 2, 2, 2), dtype=torch.uint8), torch.zeros((1, 1, 2, 2, 2)))      # not on the device


# ----------------------------------------------------------------------------- sharded seg_eval with the lesion-wise columns
class _CpuLesionwiseEval:
    """The strategy's host logic is the product code; the GPU-only calls behind ``queue_passes`` (mmtta_mask_dice_counts,
    mmtta_lesionwise_scores) are replaced by a scipy restatement."""

    def queue_passes(self, logits, y, channels_last=False):
        import numpy as np
        from scipy import ndimage
        pred = (torch.sigmoid(logits) >= self.threshold).numpy()
        gt = (y > 0.5).numpy()
        B, R_ = pred.shape[:2]
        s26 = ndimage.generate_binary_structure(3, 3)
        se = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[self.lesionwise_connectivity])
        counts = torch.zeros((B, R_, 3), dtype=torch.int64)
        stats = torch.zeros((B, R_, 7), dtype=torch.int64)
        for b in range(B):
            for r in range(R_):
                P, G = pred[b, r], gt[b, r]
                counts[b, r] = torch.tensor([int((P & G).sum()), int(P.sum()), int(G.sum())])
                Gd = ndimage.binary_dilation(G, se, self.lesionwise_dilation) if self.lesionwise_dilation else G
                lg, ng = ndimage.label(Gd, structure=s26)
                lp, npc = ndimage.label(P, structure=s26)
                sizes = np.bincount(lp.ravel(), minlength=npc + 1)
                matched = np.zeros(npc + 1, dtype=bool)
                kept = found = q = 0
                for g in range(1, ng + 1):
                    comp = lg == g
                    own = G & comp
                    ids = np.unique(lp[comp])
                    ids = ids[ids > 0]
                    matched[ids] = True
                    if own.sum() < self.lesionwise_min_voxels[r]:
                        continue
                    kept += 1
                    if ids.size:
                        found += 1
                        Pg = np.isin(lp, ids)
                        den = int(Pg.sum()) + int(own.sum())
                        q += (2 * int((Pg & own).sum()) * Q1 + den // 2) // den
                stats[b, r] = torch.tensor([ng, kept, found, npc, int(matched[1:].sum()), q, int(sizes[1:][~matched[1:]].sum())])
        return {"counts": counts, "shape": tuple(y.shape[2:]), "raw": {"lesionwise": stats}}


def _lw_setup():
    class Strat(_CpuLesionwiseEval, SegmentationEvaluationStrategy):
        pass

    cfg = {"evaluation": {"seg": {"threshold": 0.5, "region_order": REGIONS}, "loss": {"report_loss": False},
                          "lesionwise": {"enable": True, "dilation": 1, "dilation_connectivity": 6, "min_lesion_voxels": [0, 2, 1]}},
           "dataset": {"synthetic": {"enabled": True}}}
    torch.manual_seed(3)
    return Strat(cfg), torch.nn.Conv3d(2, len(REGIONS), 1)


def _lw_worker(rank, world, port, n, out_dir, shards):
    import json
    import os

    import torch.distributed as dist
    from test_shard import _batches, _eval_volumes
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    strat, model = _lw_setup()
    metrics = strat.evaluate_epoch(model, _batches(_eval_volumes(n), shards[rank], 2), "cpu")
    with open(os.path.join(out_dir, f"m{rank}.json"), "w") as fh:
        json.dump(metrics, fh)
    torch.save(strat.last_table, os.path.join(out_dir, f"tab{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("shards", [[[0, 2, 4], [1, 3]], [[0, 1, 2, 3, 4], []]])
def test_sharded_seg_eval_carries_the_lesionwise_columns(tmp_path, shards):
    """Two gloo ranks assemble rows with the lesion-wise columns, merge them and report what one process reports."""
    import json
    import os
    import socket

    import torch.multiprocessing as mp
    from test_shard import _batches, _eval_volumes
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    n, world, R = 5, 2, len(REGIONS)
    strat, model = _lw_setup()
    want = strat.evaluate_epoch(model, _batches(_eval_volumes(n), list(range(n)), 2), "cpu")
    assert "avg_lw_dc" in want and "dom/siteA/et_lw_dc" in want
    assert sum(want[f"{r.lower()}_fp_components"] + want[f"{r.lower()}_lesions"] for r in REGIONS) > 0.0
    mp.spawn(_lw_worker, args=(world, port, n, str(tmp_path), shards), nprocs=world, join=True)
    tabs = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), f"m{r}.json")) as fh:
            got = json.load(fh)
        assert got == want, f"rank {r}: {got} vs {want}"
        tabs.append(torch.load(os.path.join(str(tmp_path), f"tab{r}.pt"), weights_only=True))
    assert torch.equal(tabs[0], tabs[1]) and tabs[0].shape == (n, table_width(R, lesionwise=True))
    assert metrics_from_table(tabs[0], REGIONS, ["siteA", "siteB", "siteC"], False, lesionwise=True) == want
