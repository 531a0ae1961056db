"""What hole filling and region nesting (evaluation.postprocess.fill_holes / nesting) cost the evaluator, inside ONE process
on one GPU.

Workload: the bench U-Net (channels [32, 64, 128, 256, 512], 2 residual units, INSTANCE norm), 4 x 128^3 volumes, S = 10,
bf16 precision, 3 lanes x group 8.  One `seg_tta_eval` strategy - one set of lanes, plugins and captured graphs - evaluates
the same synthetic volumes (resident on the device) with the pass off, on, off, on after a warm-up epoch.  "Off" is
post-processing enabled with the new keys at their defaults (the component filter alone); "on" adds `fill_holes: true`,
`nesting: [ET, TC, WT]`.  Only the `enable_fill_nest` switch differs between the epochs.  Writes one JSON document:
volumes/s of every epoch, the mean of each arm, the on / off ratio and the fill / nest figures of the last `on` epoch.

Expectation from bytes, per mask voxel: 1 B of mask read and 4 B of parent written by the tile pass, 4 B read by the border
test on the faces only, the merge and flatten passes of the labeller (parents and sizes, 4 B each), then in the finish pass
4 B of parent, 1 B of open flag, 4 B of ground truth read and 1 B of mask written: about 25 B, 0.16 GB for the 3 x 128^3
voxels of a volume, next to the ~39 GB a volume moves while it adapts.

`--trace-pass` instead runs the component filter and the fill / nest pass ALONE, six calls each on 24 masks of 128^3
(tumour-like: about 1 % foreground, cavities inside), for `rocprofv3 --kernel-trace --stats -- python
scripts/bench_fill_holes.py --trace-pass`; MMTTA_FILL_UNIFORM_TILES=0 in the environment gives the tile pass without its
uniform-tile path on the same input.

usage: python scripts/bench_fill_holes.py [--volumes 96] [--pool 24] [--out profiles/fill_holes_bench.json]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # one hardware queue per lane (see bench.py)
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = dict(name="unet", in_channels=4, num_classes=3, spatial_dims=3, channels=[32, 64, 128, 256, 512],
             strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)


def tumour_masks(volumes, shape, device):
    """uint8 [volumes, 3, D, H, W]: nested balls (radius 14 / 22 / 30 at 128^3) around a centre that moves with the volume.
    ET has a core cavity and islands at density 0.002, TC and WT have 2 % of their voxels knocked out (many small holes)."""
    D, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(7)
    z, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    out = torch.zeros((volumes, 3, D, H, W), dtype=torch.uint8)
    for v in range(volumes):
        cz, cy, cx = (int(s // 2 + (torch.rand(1, generator=g).item() - 0.5) * s * 0.3) for s in shape)
        d2 = (z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2
        scale = min(shape) / 128.0
        et = (d2 <= (14 * scale) ** 2) & (d2 > (8 * scale) ** 2)
        et |= torch.rand(shape, generator=g) < 0.002
        tc = (d2 <= (22 * scale) ** 2) & (torch.rand(shape, generator=g) >= 0.02)
        wt = (d2 <= (30 * scale) ** 2) & (torch.rand(shape, generator=g) >= 0.02)
        out[v] = torch.stack([et, tc, wt]).to(torch.uint8)
    return out.to(device)


def trace_pass(a):
    from multimodal_tta_amd import ops
    device = torch.device("cuda", 0)
    shape = tuple(a.shape)
    masks = tumour_masks(8, shape, device)
    label = (torch.rand(masks.shape, device=device) < 0.02).float()
    stats = None
    for _ in range(6):
        m = masks.clone()
        ops.components_filter(m, label, a.connectivity, a.min_voxels, a.keep_largest, out=m)
        stats = ops.fill_nest(m, label, True, 6, 0, (0, 1, 2), "clip")["stats"]
    torch.cuda.synchronize()
    st = stats.sum(0).cpu().tolist()
    print(json.dumps({"masks": list(masks.shape), "foreground_fraction": round(float(masks.float().mean().item()), 4),
                      "uniform_tiles": os.environ.get("MMTTA_FILL_UNIFORM_TILES", "1") != "0",
                      "stats_sum_over_volumes": dict(zip(("et", "tc", "wt"), st))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--volumes", type=int, default=96, help="volumes per epoch")
    ap.add_argument("--pool", type=int, default=24, help="distinct synthetic volumes (repeated to fill an epoch)")
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--connectivity", type=int, default=26)
    ap.add_argument("--min-voxels", type=int, default=50)
    ap.add_argument("--keep-largest", action="store_true")
    ap.add_argument("--trace-pass", action="store_true", help="run the filter and the fill / nest pass alone (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "fill_holes_bench.json"))
    a = ap.parse_args()

    import multimodal_tta_amd  # noqa: F401
    if a.trace_pass:
        return trace_pass(a)
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.models import UNet
    from multimodal_tta_amd.registry import get_evaluation_strategy
    from multimodal_tta_amd.synth import synth_volume

    device = torch.device("cuda", 0)
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])
    cfg["model"] = dict(MODEL)
    cfg["method"].update(steps=a.steps, precision="bf16", lanes=a.lanes, group=a.group)
    cfg["evaluation"]["loss"]["report_loss"] = False
    cfg["evaluation"]["postprocess"] = {"enable": True, "connectivity": a.connectivity, "min_voxels": a.min_voxels,
                                        "keep_largest": a.keep_largest, "fill_holes": True, "nesting": ["ET", "TC", "WT"]}
    torch.manual_seed(42)
    model = UNet(MODEL)
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    assert strat.enable_fill_nest

    shape = tuple(a.shape)
    pool = [synth_volume(i, 4, shape, 3) for i in range(a.pool)]
    xs = [v["image"].unsqueeze(0).to(device) for v in pool]
    ys = [v["label"].unsqueeze(0).to(device) for v in pool]
    loader = [{"image": xs[i % a.pool], "label": ys[i % a.pool], "domain": ["synth"], "index": [i]} for i in range(a.volumes)]

    def epoch(on):
        strat.enable_fill_nest = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = strat.evaluate_epoch(model, loader, device)
        torch.cuda.synchronize()
        return a.volumes / (time.perf_counter() - t0), m

    epoch(True)                                          # warm-up: lanes, graph capture, allocator
    epochs, last_on = [], {}
    for on in (False, True, False, True):
        rate, m = epoch(on)
        epochs.append({"fill_nest": on, "volumes_per_s": round(rate, 2)})
        if on:
            last_on = {k: m[k] for k in ("avg_dc", "avg_components") + tuple(
                f"{r}_{c}" for r in ("et", "tc", "wt") for c in ("holes", "filled_holes", "filled_voxels", "nested_voxels"))}
    off = sum(e["volumes_per_s"] for e in epochs if not e["fill_nest"]) / 2
    on_ = sum(e["volumes_per_s"] for e in epochs if e["fill_nest"]) / 2
    result = {"workload": f"unet INSTANCE 4x{shape[0]}x{shape[1]}x{shape[2]} S={a.steps} bf16, {a.lanes} lanes x group {a.group}, "
                          f"{a.volumes} volumes per epoch, component filter (connectivity {a.connectivity}, min_voxels "
                          f"{a.min_voxels}, keep_largest {a.keep_largest}) in both arms; on = fill_holes true, "
                          f"fill_connectivity 6, nesting [ET, TC, WT] clip",
              "epochs": epochs, "off_volumes_per_s": round(off, 2), "on_volumes_per_s": round(on_, 2),
              "on_over_off": round(on_ / off, 4), "metrics_on": last_on,
              "peak_memory_gb": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
