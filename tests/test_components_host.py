"""Connected-component post-processing, everything that needs no GPU: the config block, the widened per-volume table and
its replay, and the argument checks of the C entry point."""
import ctypes

import pytest
import torch

from multimodal_tta_amd.evaluation import (RegionAccumulator, SegmentationEvaluationStrategy, metrics_from_table,
                                           postprocess_config, table_width)

REGIONS = ["ET", "TC", "WT"]


def _cfg(regions=None, **pp):
    cfg = {"evaluation": {"postprocess": dict(pp)}}
    if regions is not None:
        cfg["evaluation"]["seg"] = {"region_order": list(regions)}
    return cfg


# ----------------------------------------------------------------------------- config
def test_config_defaults():
    assert postprocess_config({}) == (False, 26, [0, 0, 0], [False, False, False])
    assert postprocess_config(_cfg(regions=["gtvt"])) == (False, 26, [0], [False])
    off = SegmentationEvaluationStrategy({})
    assert not off.enable_postprocess and off.postprocess_connectivity == 26


def test_config_scalars_broadcast_and_lists_are_per_region():
    assert postprocess_config(_cfg(enable=True, connectivity=6, min_voxels=7, keep_largest=True)) == \
        (True, 6, [7, 7, 7], [True, True, True])
    assert postprocess_config(_cfg(connectivity=18, min_voxels=[0, 1, 50], keep_largest=[True, False, False])) == \
        (False, 18, [0, 1, 50], [True, False, False])
    assert postprocess_config(_cfg(regions=["a", "b"], min_voxels=[3, 4], keep_largest=False)) == (False, 26, [3, 4], [False, False])
    on = SegmentationEvaluationStrategy(_cfg(enable=True, min_voxels=[1, 2, 3], keep_largest=[False, True, False]))
    assert on.enable_postprocess and on.postprocess_min_voxels == [1, 2, 3]
    assert on.postprocess_keep_largest == [False, True, False]


@pytest.mark.parametrize("pp,key", [
    (dict(min_voxels=[1, 2]), "evaluation.postprocess.min_voxels"),
    (dict(keep_largest=[True, False, True, False]), "evaluation.postprocess.keep_largest"),
    (dict(connectivity=8), "evaluation.postprocess.connectivity"),
    (dict(connectivity=True), "evaluation.postprocess.connectivity"),
    (dict(min_voxels=-1), "evaluation.postprocess.min_voxels"),
    (dict(min_voxels=[0, -3, 0]), "evaluation.postprocess.min_voxels"),
    (dict(min_voxels=2.5), "evaluation.postprocess.min_voxels"),
    (dict(keep_largest=1), "evaluation.postprocess.keep_largest"),
    (dict(keep_largest="yes"), "evaluation.postprocess.keep_largest"),
    (dict(enable="on"), "evaluation.postprocess.enable"),
])
def test_config_bad_values_name_their_key(pp, key):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        postprocess_config(_cfg(**pp))
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        SegmentationEvaluationStrategy(_cfg(**pp))


def test_shipped_configs_carry_the_block_disabled():
    from multimodal_tta_amd.config import compose
    for task, R in (("brats", 3), ("hecktor21", 1)):
        cfg = compose(overrides=[f"task={task}", "model=unet"])
        assert dict(cfg["evaluation"]["postprocess"]) == {"enable": False, "connectivity": 26, "min_voxels": 0,
                                                          "keep_largest": False}
        assert postprocess_config(cfg) == (False, 26, [0] * R, [False] * R)


# ----------------------------------------------------------------------------- table layout and replay
def test_table_width_places_the_component_columns():
    R = 2
    for surface in (False, True):
        base = table_width(R, surface)
        assert base == 3 + (5 if surface else 3) * R                          # today's layout
        assert table_width(R, surface, components=True) == base + 3 * R
        assert table_width(R, surface, 4, components=True) == table_width(R, surface, 4) + 3 * R
        assert table_width(R, surface, 4, 1, components=True) == table_width(R, surface, 4, 1) + 3 * R
        assert table_width(R, surface, components=False) == base


def _hand_rows(surface, bins):
    """Two volumes, two regions (A, B), domains d0 / d1.  Components per (volume, region): found 3, 1 / 5, 0; kept 1, 1 /
    2, 0; removed voxels 40, 0 / 10, 0."""
    R = 2
    comp = [[3, 1, 1, 1, 40, 0], [5, 0, 2, 0, 10, 0]]
    rows = []
    for i in range(2):
        row = [float(i), float(i), 0.25 * (i + 1), 0.5 + 0.1 * i, 0.7, 0.4, 0.5, 1.0, 1.0 - i]      # B of volume 1 is invalid
        if surface:
            row += [2.0 + i, 3.0, 1.0, 0.5 + i]
        mark = len(row)
        row += [float(v) for v in comp[i]]
        if bins:
            # one calibration row per region, 3*bins + 2 doubles: 10 elements in the last bin
            for r in range(R):
                row += [0.0] * (3 * (bins - 1)) + [10.0, 9.0, 8.0 + r, 1.0, 2.0]
        rows.append(row)
    return torch.tensor(rows, dtype=torch.float64), mark


@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("bins", [0, 4])
def test_metrics_from_table_reads_the_component_columns(surface, bins):
    regions = ["A", "B"]
    table, mark = _hand_rows(surface, bins)
    assert table.shape[1] == table_width(2, surface, bins, components=True)
    assert mark == table_width(2, surface)                                    # behind the surface columns ...
    assert table.shape[1] - (mark + 6) == table_width(2, False, bins) - table_width(2)      # ... before the calibration block
    m = metrics_from_table(table, regions, ["d0", "d1"], True, surface, bins, components=True)
    want = {"a_components": 4.0, "b_components": 0.5, "a_kept_components": 1.5, "b_kept_components": 0.5,
            "a_removed_voxels": 25.0, "b_removed_voxels": 0.0, "avg_components": 2.25,
            "dom/d0/a_components": 3.0, "dom/d0/b_components": 1.0, "dom/d0/a_kept_components": 1.0,
            "dom/d0/b_kept_components": 1.0, "dom/d0/a_removed_voxels": 40.0, "dom/d0/b_removed_voxels": 0.0,
            "dom/d0/avg_components": 2.0,
            "dom/d1/a_components": 5.0, "dom/d1/b_components": 0.0, "dom/d1/a_kept_components": 2.0,
            "dom/d1/b_kept_components": 0.0, "dom/d1/a_removed_voxels": 10.0, "dom/d1/b_removed_voxels": 0.0,
            "dom/d1/avg_components": 2.5}
    for k, v in want.items():
        assert m[k] == v, (k, m[k], v)
    # the other keys are those of the same table without the component columns
    plain = torch.cat([table[:, :mark], table[:, mark + 6:]], 1)
    base = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, bins)
    assert {k: m[k] for k in base} == base and set(m) == set(base) | set(want)
    if bins:
        assert "a_ece" in m and m["a_ece"] == base["a_ece"]


def test_without_the_keyword_nothing_changes():
    regions = ["A", "B"]
    for surface in (False, True):
        table, mark = _hand_rows(surface, 0)
        plain = table[:, :mark]
        a = metrics_from_table(plain, regions, ["d0", "d1"], True, surface)
        b = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, components=False)
        assert a == b and not any("components" in k or "removed_voxels" in k for k in a)
        acc = RegionAccumulator(regions, surface)
        assert not acc.components


# ----------------------------------------------------------------------------- the C entry point, without a device
def _call(lib, mask_in=1, mask_out=1, label=None, n=1, r=1, d=4, h=4, w=4, conn=26, counts=None, scratch=1, min_voxels=None):
    from multimodal_tta_amd import _lib
    mv = (ctypes.c_int64 * 64)(*(min_voxels or [0] * 64))
    kl = (ctypes.c_int32 * 64)()
    lab = None
    if label:
        t = _lib.Tensor(4096, n, r, d, h, w, r * d * h * w, d * h * w, h * w, w, 1, _lib.F32, 0)
        lab = ctypes.byref(t)
    return lib.mmtta_components_filter(mask_in, mask_out, lab, n, r, d, h, w, conn, mv, kl, counts, None, None, scratch, None)


def test_argument_validation_without_a_gpu():
    """Bad arguments are refused before anything touches the device (the pointers here are never followed)."""
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    assert _call(lib, mask_in=None) == -1 and b"null" in lib.mmtta_last_error()
    assert _call(lib, scratch=None) == -1 and b"null" in lib.mmtta_last_error()
    assert _call(lib, conn=8) == -1 and b"connectivity 8" in lib.mmtta_last_error()
    assert _call(lib, r=65) == -2 and b"65" in lib.mmtta_last_error()
    assert _call(lib, d=0) == -1 and b"extent" in lib.mmtta_last_error()
    assert _call(lib, d=2048, h=2048, w=512) == -2 and b"2^31" in lib.mmtta_last_error()      # 2^31 voxels: two too many
    assert _call(lib, d=65536, h=65536, w=65536) == -2 and b"2^31" in lib.mmtta_last_error()
    assert _call(lib, counts=1) == -1 and b"label" in lib.mmtta_last_error()
    assert _call(lib, n=2, d=1, h=1, w=2 ** 31 - 2) == -2 and b"split the batch" in lib.mmtta_last_error()
    assert _call(lib, label=True, min_voxels=[-5] + [0] * 63) == -1 and b"min_voxels" in lib.mmtta_last_error()


def test_scratch_bytes():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    nb = lib.mmtta_components_scratch_bytes(6, 128, 128, 128)
    assert nb >= 6 * 128 ** 3 * 4                                             # at least the int32 label volume
    assert nb < 6 * 128 ** 3 * 16
    assert lib.mmtta_components_scratch_bytes(1, 1, 1, 5) > 0
    assert lib.mmtta_components_scratch_bytes(1, 2048, 2048, 512) < 0         # 2^31 voxels
    assert lib.mmtta_components_scratch_bytes(1, 1, 1, 2 ** 31 - 2) > 0         # thin volumes too: the tile pass loops
    assert lib.mmtta_components_scratch_bytes(2, 1, 1, 2 ** 31 - 2) < 0         # 2^32 voxels in one call: split the batch
    assert lib.mmtta_components_scratch_bytes(3, 1024, 1024, 1024) > 0
    assert lib.mmtta_components_scratch_bytes(1, 1, 1, 2 ** 31 - 1) < 0
    assert lib.mmtta_components_scratch_bytes(1, 2 ** 40, 2 ** 40, 2 ** 40) < 0
    assert lib.mmtta_components_scratch_bytes(0, 4, 4, 4) < 0
    assert lib.mmtta_components_scratch_bytes(1, 0, 4, 4) < 0


def test_ops_wrapper_checks_before_the_library():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    with pytest.raises(MmttaError, match="uint8"):
        ops.components_filter(torch.zeros((1, 1, 2, 2, 2), dtype=torch.float32))
    with pytest.raises(MmttaError, match="dense"):
        ops.components_filter(torch.zeros((1, 1, 2, 2, 2), dtype=torch.uint8))           # not on the device


# ----------------------------------------------------------------------------- sharded seg_eval with the component columns
class _CpuFilteredEval:
    """The strategy's host logic is the product code; the two GPU-only calls behind ``queue_passes`` (mmtta_mask_dice_counts,
    mmtta_components_filter) are replaced by a scipy restatement: 6-connected components below 3 voxels are dropped."""

    def queue_passes(self, logits, y, channels_last=False):
        import numpy as np
        from scipy import ndimage
        pred = (torch.sigmoid(logits) >= self.threshold).numpy()
        gt = (y > 0.5).numpy()
        B, R_ = pred.shape[:2]
        counts = torch.zeros((B, R_, 3), dtype=torch.int64)
        stats = torch.zeros((B, R_, 3), dtype=torch.int64)
        for b in range(B):
            for r in range(R_):
                lab, n = ndimage.label(pred[b, r])
                sizes = np.bincount(lab.ravel(), minlength=n + 1)
                ok = np.flatnonzero(sizes[1:] >= self.postprocess_min_voxels[r]) + 1
                keep = np.isin(lab, ok)
                counts[b, r] = torch.tensor([int((keep & gt[b, r]).sum()), int(keep.sum()), int(gt[b, r].sum())])
                stats[b, r] = torch.tensor([n, len(ok), int(pred[b, r].sum() - keep.sum())])
        return {"counts": counts, "shape": tuple(y.shape[2:]), "raw": {"components": stats}}


def _pp_setup():
    class Strat(_CpuFilteredEval, SegmentationEvaluationStrategy):
        pass

    cfg = {"evaluation": {"seg": {"threshold": 0.5, "region_order": REGIONS}, "loss": {"report_loss": False},
                          "postprocess": {"enable": True, "connectivity": 6, "min_voxels": [3, 0, 2]}},
           "dataset": {"synthetic": {"enabled": True}}}
    torch.manual_seed(3)
    return Strat(cfg), torch.nn.Conv3d(2, len(REGIONS), 1)


def _pp_worker(rank, world, port, n, out_dir, shards):
    import json
    import os

    import torch.distributed as dist
    from test_shard import _batches, _eval_volumes
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    strat, model = _pp_setup()
    metrics = strat.evaluate_epoch(model, _batches(_eval_volumes(n), shards[rank], 2), "cpu")
    with open(os.path.join(out_dir, f"m{rank}.json"), "w") as fh:
        json.dump(metrics, fh)
    torch.save(strat.last_table, os.path.join(out_dir, f"tab{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("shards", [[[0, 2, 4], [1, 3]], [[0, 1, 2, 3, 4], []]])
def test_sharded_seg_eval_carries_the_component_columns(tmp_path, shards):
    """Two gloo ranks assemble rows with the component columns, merge them and report what one process reports."""
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
    strat, model = _pp_setup()
    want = strat.evaluate_epoch(model, _batches(_eval_volumes(n), list(range(n)), 2), "cpu")
    assert want["avg_components"] > 0.0 and "dom/siteA/et_removed_voxels" in want
    assert sum(want[f"{r.lower()}_removed_voxels"] for r in REGIONS) > 0.0
    mp.spawn(_pp_worker, args=(world, port, n, str(tmp_path), shards), nprocs=world, join=True)
    tabs = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), f"m{r}.json")) as fh:
            got = json.load(fh)
        assert got == want, f"rank {r}: {got} vs {want}"
        tabs.append(torch.load(os.path.join(str(tmp_path), f"tab{r}.pt"), weights_only=True))
    assert torch.equal(tabs[0], tabs[1]) and tabs[0].shape == (n, table_width(R, components=True))
    assert metrics_from_table(tabs[0], REGIONS, ["siteA", "siteB", "siteC"], False, components=True) == want
