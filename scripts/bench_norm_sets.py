"""Grouped adaptation of a BatchNorm U-Net (method.norm_sets) against its fall-back (one volume per launch sequence), inside
ONE process on one GPU: adapted volumes/s of each arrangement, peak device memory, and whether the grouped run's Dice counts
equal the fall-back's.

Workload: the bench U-Net (channels [32, 64, 128, 256, 512], 2 residual units) with norm BATCH, 4 x 128^3 volumes, S = 10,
bf16 precision (BatchNorm models keep fp32 activation storage), for each `method.params` setting:
  grouped   lanes x group volumes in flight, method.norm_sets: true (every volume with its own affines, Adam state and
            running statistics)
  fallback  lanes x 1 (what such a model runs today)
Both arrangements adapt the same seeded volumes, alternated round by round after a warm-up (graph capture), with at least
--volumes timed volumes each.  Both use the launch geometry of lanes x group volumes in flight (method.tune_volumes), so the
two agree bit for bit and their Dice counts are compared exactly.  If lanes x group does not fit in device memory, the group
is halved until it does (reported).  Prints one JSON line.

usage: python scripts/bench_norm_sets.py [--lanes 3] [--group 8] [--volumes 48] [--params norm_affine all]
"""
import argparse
import gc
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # one hardware queue per lane (see bench.py)
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402

MODEL = dict(name="unet", in_channels=4, num_classes=3, spatial_dims=3, channels=[32, 64, 128, 256, 512],
             strides=[2, 2, 2, 2], num_res_units=2, norm="BATCH", act="RELU", dropout=0.0)


class Arrangement:
    """`lanes` plugins (own model replica, stream and graph each) adapting `group` volumes per launch sequence."""

    def __init__(self, name, params, lanes, group, norm_sets, tune_volumes, streams, device, shape, steps):
        import multimodal_tta_amd  # noqa: F401
        from multimodal_tta_amd.config import compose
        from multimodal_tta_amd.models import UNet
        from multimodal_tta_amd.registry import get_plugin

        self.name, self.lanes, self.group = name, lanes, group
        cfg = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])
        cfg["model"] = dict(MODEL)
        m = cfg["method"]
        m.update(steps=steps, precision="bf16", params=params, group=group, lanes=lanes, norm_sets=norm_sets,
                 tune_volumes=tune_volumes)
        self.streams = streams[:lanes]
        self.plugs = []
        for lane in range(lanes):
            torch.manual_seed(42)                       # the same source weights in every lane and arrangement
            model = UNet(MODEL)
            p = get_plugin("entmin_tta")(cfg)
            p.lane = lane
            self.plugs.append(p.setup(model, device))
            assert p.group == group, f"{name}: the plugin settled on group {p.group}"

    def round(self, xs, ys, counts, first):
        """Adapt volumes [first, first + lanes * group) of the pool (lane l: a slice of `group` volumes)."""
        from multimodal_tta_amd import ops
        for lane in range(self.lanes):
            lo = first + lane * self.group
            with torch.cuda.stream(self.streams[lane]):
                res = self.plugs[lane].adapt_volume(xs[lo:lo + self.group])
                ops.mask_dice_counts(res["logits_cl"], ys[lo:lo + self.group], 0.5, counts[lo:lo + self.group], None)
        return self.lanes * self.group


def measure(params, lanes, group, volumes, shape, steps, device, streams):
    from multimodal_tta_amd.synth import synth_volume

    per_g = lanes * group
    pool_n = per_g                                      # both arrangements adapt the same per_g volumes over and over
    vs = [synth_volume(i, 4, shape, 3) for i in range(pool_n)]
    xs = torch.stack([v["image"] for v in vs]).to(device)
    ys = torch.stack([v["label"] for v in vs]).to(device)
    out = {}
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    grouped = Arrangement("grouped", params, lanes, group, True, per_g, streams, device, shape, steps)
    cg = torch.zeros((pool_n, 3, 3), dtype=torch.int64, device=device)
    grouped.round(xs, ys, cg, 0)                        # warm-up: capture
    torch.cuda.synchronize()
    out["grouped_peak_gb"] = round((torch.cuda.max_memory_allocated(device) - base) / 2 ** 30, 2)
    base_f = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    fallback = Arrangement("fallback", params, lanes, 1, False, per_g, streams, device, shape, steps)
    cf = torch.zeros((pool_n, 3, 3), dtype=torch.int64, device=device)
    for first in range(0, pool_n, lanes):               # warm-up over the whole pool: counts of every volume
        fallback.round(xs, ys, cf, first)
    torch.cuda.synchronize()
    out["fallback_peak_gb"] = round((torch.cuda.max_memory_allocated(device) - base_f) / 2 ** 30, 2)
    out["dice_counts_equal"] = bool(torch.equal(cg, cf))
    t = {"grouped": 0.0, "fallback": 0.0}
    n = {"grouped": 0, "fallback": 0}
    while min(n.values()) < volumes:                    # alternated: one pool's worth of volumes per arrangement and turn
        for arr, counts in ((grouped, cg), (fallback, cf)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for first in range(0, pool_n, arr.lanes * arr.group):
                n[arr.name] += arr.round(xs, ys, counts, first)
            torch.cuda.synchronize()
            t[arr.name] += time.perf_counter() - t0
    out["dice_counts_equal"] = out["dice_counts_equal"] and bool(torch.equal(cg, cf))
    out["grouped_volumes_per_s"] = round(n["grouped"] / t["grouped"], 2)
    out["fallback_volumes_per_s"] = round(n["fallback"] / t["fallback"], 2)
    out["timed_volumes"] = dict(n)
    out["speedup"] = round(out["grouped_volumes_per_s"] / out["fallback_volumes_per_s"], 3)
    del grouped, fallback, xs, ys
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--volumes", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--params", nargs="+", default=["norm_affine", "all"])
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    result = {"workload": f"unet BATCH {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes, "runs": {}}
    for params in a.params:
        group = a.group
        while True:
            try:
                r = measure(params, a.lanes, group, a.volumes, tuple(a.shape), a.steps, device, streams)
                break
            except torch.cuda.OutOfMemoryError:
                gc.collect()
                torch.cuda.empty_cache()
                if group == 1:
                    raise
                group //= 2
        r["group"] = group
        result["runs"][params] = r
    result["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
