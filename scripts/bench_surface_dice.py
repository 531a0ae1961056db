"""What the normalised surface Dice costs the evaluator, region-wise (evaluation.surface_dice) and lesion-wise
(evaluation.lesionwise.nsd), inside ONE process on one GPU.

Workload: the bench U-Net (channels [32, 64, 128, 256, 512], 2 residual units, INSTANCE norm), 4 x 128^3 volumes, S = 10,
bf16 precision, 3 lanes x group 8.  One `seg_tta_eval` strategy - one set of lanes, plugins and captured graphs - evaluates
the same synthetic volumes (resident on the device) after a warm-up epoch, twice with the arms off, on, off, on:

  region   off: no evaluation block at all (the parent's default run)      on: plus `evaluation.surface_dice.enable=true`
  lesion   off: `evaluation.lesionwise.enable=true` alone                   on: plus `evaluation.lesionwise.nsd.enable=true`

Only the evaluator's switches differ between the epochs.  Writes one JSON document: volumes/s of every epoch, the mean of each
arm, the on / off ratios and the NSD figures of the last `on` epochs.

Expectation from bytes: both passes move well under 0.1 KB per voxel next to the ~39 GB a volume's adaptation moves, and the
search is linear in the volume whatever the masks look like: the lesion-wise pass should sit beside the lesion-wise Dice
pass, far from the 0.42 of the lesion-wise HD95 on the same masks.

usage: python scripts/bench_surface_dice.py [--volumes 96] [--pool 24] [--out profiles/surface_dice_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--volumes", type=int, default=96, help="volumes per epoch")
    ap.add_argument("--pool", type=int, default=24, help="distinct synthetic volumes (repeated to fill an epoch)")
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--dilation", type=int, default=3)
    ap.add_argument("--dilation-connectivity", type=int, default=18)
    ap.add_argument("--tolerances", type=float, nargs="+", default=[1.0], help="evaluation.surface_dice.tolerances")
    ap.add_argument("--lesion-tolerances", type=float, nargs="+", default=[0.5, 1.0], help="evaluation.lesionwise.nsd.tolerances")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "surface_dice_bench.json"))
    a = ap.parse_args()

    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.models import UNet
    from multimodal_tta_amd.registry import get_evaluation_strategy
    from multimodal_tta_amd.synth import synth_volume

    device = torch.device("cuda", 0)
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])
    cfg["model"] = dict(MODEL)
    cfg["method"].update(steps=a.steps, precision="bf16", lanes=a.lanes, group=a.group)
    cfg["evaluation"]["loss"]["report_loss"] = False
    cfg["evaluation"]["surface_dice"] = {"enable": True, "tolerances": list(a.tolerances)}
    cfg["evaluation"]["lesionwise"] = {"enable": True, "dilation": a.dilation, "dilation_connectivity": a.dilation_connectivity,
                                       "nsd": {"enable": True, "tolerances": list(a.lesion_tolerances)}}
    torch.manual_seed(42)
    model = UNet(MODEL)
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)

    shape = tuple(a.shape)
    pool = [synth_volume(i, 4, shape, 3) for i in range(a.pool)]
    xs = [v["image"].unsqueeze(0).to(device) for v in pool]
    ys = [v["label"].unsqueeze(0).to(device) for v in pool]
    loader = [{"image": xs[i % a.pool], "label": ys[i % a.pool], "domain": ["synth"], "index": [i]} for i in range(a.volumes)]

    def epoch(surface_dice, lesionwise, nsd):
        strat.enable_surface_dice, strat.enable_lesionwise, strat.enable_lesionwise_nsd = surface_dice, lesionwise, nsd
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = strat.evaluate_epoch(model, loader, device)
        torch.cuda.synchronize()
        return a.volumes / (time.perf_counter() - t0), m

    epoch(True, True, True)                              # warm-up: lanes, graph capture, allocator, every scratch
    result = {"workload": f"unet INSTANCE 4x{shape[0]}x{shape[1]}x{shape[2]} S={a.steps} bf16, {a.lanes} lanes x group {a.group}, "
                          f"{a.volumes} volumes per epoch, dilation {a.dilation} x {a.dilation_connectivity}, tolerances "
                          f"{a.tolerances} (region) {a.lesion_tolerances} (lesion)"}
    for name, off_arm, on_arm in (("region", (False, False, False), (True, False, False)),
                                  ("lesion", (False, True, False), (False, True, True))):
        epochs, last_on = [], {}
        for on in (False, True, False, True):
            rate, m = epoch(*(on_arm if on else off_arm))
            epochs.append({"on": on, "volumes_per_s": round(rate, 2)})
            if on:
                last_on = {k: v for k, v in m.items() if "/" not in k and ("nsd" in k or k in ("avg_dc", "avg_lw_dc"))}
        off = sum(e["volumes_per_s"] for e in epochs if not e["on"]) / 2
        on_ = sum(e["volumes_per_s"] for e in epochs if e["on"]) / 2
        result[name] = {"epochs": epochs, "off_volumes_per_s": round(off, 2), "on_volumes_per_s": round(on_, 2),
                        "on_over_off": round(on_ / off, 4), "metrics_on": last_on}
    # what the process really ran with: a value already in the environment wins over the setdefault above
    result["gpu_max_hw_queues"] = os.environ.get("GPU_MAX_HW_QUEUES")
    result["hw_queues"] = ops.hw_queue_status()
    result["peak_memory_gb"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
