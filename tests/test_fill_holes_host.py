"""Hole filling and region nesting, everything that needs no GPU: the new keys of the post-processing block, the widened
per-volume table and its replay, a sharded run against a single one, and the argument checks of the C entry point."""
import ctypes

import pytest
import torch

from multimodal_tta_amd.evaluation import (POSTPROCESS_FILL_DEFAULTS, RegionAccumulator, SegmentationEvaluationStrategy,
                                           fill_nest_config, metrics_from_table, postprocess_config, table_width)

REGIONS = ["ET", "TC", "WT"]


def _cfg(regions=None, **pp):
    cfg = {"evaluation": {"postprocess": dict(pp)}}
    if regions is not None:
        cfg["evaluation"]["seg"] = {"region_order": list(regions)}
    return cfg


# ----------------------------------------------------------------------------- config
def test_config_defaults():
    assert fill_nest_config({}) == ([False] * 3, 6, [0] * 3, [], "clip")
    assert fill_nest_config(_cfg(regions=["gtvt"])) == ([False], 6, [0], [], "clip")
    assert POSTPROCESS_FILL_DEFAULTS == {"fill_holes": False, "fill_connectivity": 6, "max_hole_voxels": 0, "nesting": [],
                                         "nesting_mode": "clip"}
    assert fill_nest_config(_cfg(**POSTPROCESS_FILL_DEFAULTS)) == fill_nest_config({})
    for cfg in ({}, _cfg(enable=True), _cfg(enable=True, **POSTPROCESS_FILL_DEFAULTS), _cfg(fill_holes=True, nesting=["ET", "WT"])):
        assert not SegmentationEvaluationStrategy(cfg).enable_fill_nest      # defaults, or the block itself off: no pass
    assert postprocess_config(_cfg(enable=True, fill_holes=True)) == (True, 26, [0, 0, 0], [False, False, False])


def test_config_values():
    assert fill_nest_config(_cfg(fill_holes=True, fill_connectivity=26, max_hole_voxels=9, nesting=["ET", "TC", "WT"],
                                 nesting_mode="grow")) == ([True] * 3, 26, [9] * 3, [0, 1, 2], "grow")
    assert fill_nest_config(_cfg(fill_holes=[False, True, False], max_hole_voxels=[0, 5, 0], nesting=("WT", "ET"))) == \
        ([False, True, False], 6, [0, 5, 0], [2, 0], "clip")
    assert fill_nest_config(_cfg(regions=["a", "b"], nesting=["b", "a"], fill_holes=[True, False])) == \
        ([True, False], 6, [0, 0], [1, 0], "clip")
    s = SegmentationEvaluationStrategy(_cfg(enable=True, fill_holes=[False, False, True]))
    assert s.enable_fill_nest and s.postprocess_fill_holes == [False, False, True] and s.postprocess_nesting == []
    s = SegmentationEvaluationStrategy(_cfg(enable=True, nesting=["TC", "WT"], nesting_mode="grow"))
    assert s.enable_fill_nest and s.postprocess_nesting == [1, 2] and s.postprocess_nesting_mode == "grow"


@pytest.mark.parametrize("pp,key", [
    (dict(fill_holes=[True, False]), "evaluation.postprocess.fill_holes"),
    (dict(fill_holes=1), "evaluation.postprocess.fill_holes"),
    (dict(fill_holes="yes"), "evaluation.postprocess.fill_holes"),
    (dict(fill_connectivity=8), "evaluation.postprocess.fill_connectivity"),
    (dict(fill_connectivity=True), "evaluation.postprocess.fill_connectivity"),
    (dict(max_hole_voxels=-1), "evaluation.postprocess.max_hole_voxels"),
    (dict(max_hole_voxels=[0, 1]), "evaluation.postprocess.max_hole_voxels"),
    (dict(max_hole_voxels=2.5), "evaluation.postprocess.max_hole_voxels"),
    (dict(max_hole_voxels=True), "evaluation.postprocess.max_hole_voxels"),
    (dict(nesting="ET"), "evaluation.postprocess.nesting"),
    (dict(nesting=["ET"]), "evaluation.postprocess.nesting"),
    (dict(nesting=["ET", "ET"]), "evaluation.postprocess.nesting"),
    (dict(nesting=["ET", "NCR"]), "evaluation.postprocess.nesting"),
    (dict(nesting=[0, 1]), "evaluation.postprocess.nesting"),
    (dict(nesting=3), "evaluation.postprocess.nesting"),
    (dict(nesting_mode="shrink"), "evaluation.postprocess.nesting_mode"),
    (dict(nesting_mode=True), "evaluation.postprocess.nesting_mode"),
])
def test_config_bad_values_name_their_key(pp, key):
    for block in (pp, dict(pp, enable=True)):
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + r"\b"):
            fill_nest_config(_cfg(**block))
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + r"\b"):
            SegmentationEvaluationStrategy(_cfg(**block))


def test_shipped_configs_leave_the_pass_out():
    from multimodal_tta_amd.config import compose
    for task, R in (("brats", 3), ("hecktor21", 1)):
        cfg = compose(overrides=[f"task={task}", "model=unet"])
        assert fill_nest_config(cfg) == ([False] * R, 6, [0] * R, [], "clip")
    cfg = compose(overrides=["task=brats", "model=unet", "evaluation.postprocess.enable=true",
                             "evaluation.postprocess.fill_holes=true", "evaluation.postprocess.nesting=[ET,TC,WT]"])
    assert fill_nest_config(cfg) == ([True] * 3, 6, [0] * 3, [0, 1, 2], "clip")
    assert SegmentationEvaluationStrategy(cfg).enable_fill_nest


# ----------------------------------------------------------------------------- table layout and replay
def test_table_width_places_the_columns():
    R = 2
    for surface in (False, True):
        for lw in (False, True):
            base = table_width(R, surface, components=True, lesionwise=lw)
            assert table_width(R, surface, components=True, lesionwise=lw, fill_nest=True) == base + 4 * R
            assert table_width(R, surface, 4, 1, components=True, lesionwise=lw, fill_nest=True) == \
                table_width(R, surface, 4, 1, components=True, lesionwise=lw) + 4 * R
            assert table_width(R, surface, components=True, lesionwise=lw, fill_nest=False) == base


@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("bins", [0, 4])
def test_metrics_from_table_reads_the_columns(surface, bins):
    from test_components_host import _hand_rows
    regions = ["A", "B"]
    plain, mark = _hand_rows(surface, bins)                  # ... surface | components (6) | calibration
    fill = torch.tensor([[4, 0, 2, 0, 30, 0, 7, 1], [2, 2, 0, 1, 0, 5, 0, 3]], dtype=torch.float64)
    table = torch.cat([plain[:, :mark + 6], fill, plain[:, mark + 6:]], 1)
    assert table.shape[1] == table_width(2, surface, bins, components=True, fill_nest=True)
    m = metrics_from_table(table, regions, ["d0", "d1"], True, surface, bins, components=True, fill_nest=True)
    want = {"a_holes": 3.0, "b_holes": 1.0, "a_filled_holes": 1.0, "b_filled_holes": 0.5, "a_filled_voxels": 15.0,
            "b_filled_voxels": 2.5, "a_nested_voxels": 3.5, "b_nested_voxels": 2.0,
            "dom/d0/a_holes": 4.0, "dom/d0/b_holes": 0.0, "dom/d0/a_filled_holes": 2.0, "dom/d0/b_filled_holes": 0.0,
            "dom/d0/a_filled_voxels": 30.0, "dom/d0/b_filled_voxels": 0.0, "dom/d0/a_nested_voxels": 7.0, "dom/d0/b_nested_voxels": 1.0,
            "dom/d1/a_holes": 2.0, "dom/d1/b_holes": 2.0, "dom/d1/a_filled_holes": 0.0, "dom/d1/b_filled_holes": 1.0,
            "dom/d1/a_filled_voxels": 0.0, "dom/d1/b_filled_voxels": 5.0, "dom/d1/a_nested_voxels": 0.0, "dom/d1/b_nested_voxels": 3.0}
    for k, v in want.items():
        assert m[k] == v, (k, m[k], v)
    base = metrics_from_table(plain, regions, ["d0", "d1"], True, surface, bins, components=True)
    assert {k: m[k] for k in base} == base and set(m) == set(base) | set(want)
    assert not RegionAccumulator(regions, surface).fill_nest


# ----------------------------------------------------------------------------- the C entry point, without a device
def _call(lib, mask=1, label=None, n=1, r=3, d=4, h=4, w=4, conn=6, fill=1, cap=None, chain=(), chain_ptr=True, mode=0, counts=None,
          stats=1, scratch=1, label_shape=None, label_dtype=None):
    from multimodal_tta_amd import _lib
    fh = (ctypes.c_int32 * 64)(*([1] * 64)) if fill else None
    mv = (ctypes.c_int64 * 64)(*(cap or [0] * 64))
    ch = (ctypes.c_int32 * 64)(*chain) if chain_ptr else None
    lab = None
    if label:
        ln, lr, ld, lh, lw = label_shape or (n, r, d, h, w)
        t = _lib.Tensor(4096, ln, lr, ld, lh, lw, lr * ld * lh * lw, ld * lh * lw, lh * lw, lw, 1,
                        _lib.F32 if label_dtype is None else label_dtype, 0)
        lab = ctypes.byref(t)
    return lib.mmtta_mask_fill_nest(mask, lab, n, r, d, h, w, conn, fh, mv, ch, len(chain), mode, counts, stats, scratch, None)


def test_argument_validation_without_a_gpu():
    """Bad arguments are refused before anything touches the device (the pointers here are never followed)."""
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    err = lib.mmtta_last_error
    for kw in (dict(mask=None), dict(scratch=None), dict(stats=None), dict(fill=0)):
        assert _call(lib, **kw) == -1 and b"null" in err(), kw
    assert _call(lib, conn=8) == -1 and b"fill_connectivity 8" in err()
    assert _call(lib, cap=[0, -5] + [0] * 62) == -1 and b"max_hole_voxels[1]" in err()
    assert _call(lib, chain=(1,)) == -1 and b"chain_len 1" in err()
    assert _call(lib, chain=(0, 1, 2, 0)) == -1 and b"chain_len 4" in err()
    assert _call(lib, chain=(0, 1, 0)) == -1 and b"chain[2] = 0 is repeated" in err()
    assert _call(lib, chain=(0, 3)) == -1 and b"chain[1] = 3" in err()
    assert _call(lib, chain=(-1, 2)) == -1 and b"chain[0] = -1" in err()
    assert _call(lib, chain=(0, 1), chain_ptr=False) == -1 and b"null chain" in err()
    assert _call(lib, mode=2) == -1 and b"nest_mode 2" in err()
    assert _call(lib, counts=1) == -1 and b"label" in err()
    assert _call(lib, label=True, label_shape=(1, 3, 4, 4, 5)) == -1 and b"label shape" in err()
    assert _call(lib, label=True, label_dtype=_lib.BF16) == -2 and b"label" in err() and b"fp32" in err()
    assert _call(lib, r=65) == -2 and b"65" in err()
    assert _call(lib, d=0) == -1 and b"extent" in err()
    assert _call(lib, d=2048, h=2048, w=512) == -2 and b"2^31" in err()
    assert _call(lib, n=2, r=1, d=1, h=1, w=2 ** 31 - 2) == -2 and b"split the batch" in err()
    assert _call(lib, n=65536, r=1) == -2 and b"65535" in err()


def test_symbols_and_abi_version():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    assert lib.mmtta_abi_version() == 2
    assert hasattr(lib, "mmtta_mask_fill_nest") and hasattr(lib, "mmtta_mask_fill_nest_scratch_bytes")
    nb = lib.mmtta_mask_fill_nest_scratch_bytes(6, 128, 128, 128)
    assert 6 * 128 ** 3 * 9 <= nb < 6 * 128 ** 3 * 10            # parents, sizes, open flags
    assert lib.mmtta_mask_fill_nest_scratch_bytes(1, 1, 1, 5) > 0
    assert lib.mmtta_mask_fill_nest_scratch_bytes(1, 2048, 2048, 512) < 0
    assert lib.mmtta_mask_fill_nest_scratch_bytes(2, 1, 1, 2 ** 31 - 2) < 0
    assert lib.mmtta_mask_fill_nest_scratch_bytes(0, 4, 4, 4) < 0
    assert lib.mmtta_mask_fill_nest_scratch_bytes(65536, 4, 4, 4) < 0


def test_ops_wrapper_checks_before_the_library():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError
    with pytest.raises(MmttaError, match="uint8"):
        ops.fill_nest(torch.zeros((1, 1, 2, 2, 2), dtype=torch.float32))
    with pytest.raises(MmttaError, match="dense"):
        ops.fill_nest(torch.zeros((1, 1, 2, 2, 2), dtype=torch.uint8))           # not on the device


# ----------------------------------------------------------------------------- sharded seg_eval with the new columns
class _CpuFillEval:
    """The strategy's host logic is the product code; the GPU calls behind ``queue_passes`` are replaced by a scipy restatement:
    no component is dropped (one is counted), then holes are filled and the chain applied as configured."""

    def queue_passes(self, logits, y, channels_last=False):
        import numpy as np
        from test_hip_fill_holes import oracle
        pred = (torch.sigmoid(logits) >= self.threshold).numpy().astype(np.uint8)
        final, counts, fstats = oracle(pred, y.numpy(), self.postprocess_fill_connectivity, self.postprocess_fill_holes,
                                       self.postprocess_max_hole_voxels, self.postprocess_nesting, self.postprocess_nesting_mode)
        raw = {"components": torch.ones((pred.shape[0], pred.shape[1], 3), dtype=torch.int64), "fill_nest": torch.from_numpy(fstats)}
        return {"counts": torch.from_numpy(counts), "shape": tuple(y.shape[2:]), "raw": raw}


def _setup():
    class Strat(_CpuFillEval, SegmentationEvaluationStrategy):
        pass

    cfg = {"evaluation": {"seg": {"threshold": 0.5, "region_order": REGIONS}, "loss": {"report_loss": False},
                          "postprocess": {"enable": True, "fill_holes": [True, True, False], "nesting": ["ET", "WT"],
                                          "nesting_mode": "grow"}},
           "dataset": {"synthetic": {"enabled": True}}}
    torch.manual_seed(3)
    return Strat(cfg), torch.nn.Conv3d(2, len(REGIONS), 1)


def _worker(rank, world, port, n, out_dir, shards):
    import json
    import os

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
    dist.destroy_process_group()


def test_sharded_seg_eval_equals_a_single_run(tmp_path):
    """Two gloo ranks assemble rows with the fill / nest columns, merge them and report what one process reports."""
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
    shards = [[0, 2, 4], [1, 3]]
    strat, model = _setup()
    assert strat.enable_fill_nest
    want = strat.evaluate_epoch(model, _batches(_eval_volumes(n), list(range(n)), 2), "cpu")
    assert "dom/siteA/et_holes" in want and "wt_nested_voxels" in want
    assert sum(want[f"{r.lower()}_nested_voxels"] for r in REGIONS) > 0.0
    mp.spawn(_worker, args=(world, port, n, str(tmp_path), shards), nprocs=world, join=True)
    tabs = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), f"m{r}.json")) as fh:
            got = json.load(fh)
        assert got == want, f"rank {r}: {got} vs {want}"
        tabs.append(torch.load(os.path.join(str(tmp_path), f"tab{r}.pt"), weights_only=True))
    assert torch.equal(tabs[0], tabs[1]) and tabs[0].shape == (n, table_width(R, components=True, fill_nest=True))
    assert metrics_from_table(tabs[0], REGIONS, ["siteA", "siteB", "siteC"], False, components=True, fill_nest=True) == want
