"""What the lesion-wise HD95 (evaluation.lesionwise.hd95) costs the evaluator on top of the lesion-wise scores, inside ONE
process on one GPU.

Workload: the bench U-Net (channels [32, 64, 128, 256, 512], 2 residual units, INSTANCE norm), 4 x 128^3 volumes, S = 10,
bf16 precision, 3 lanes x group 8.  One `seg_tta_eval` strategy - one set of lanes, plugins and captured graphs - evaluates
the same synthetic volumes (resident on the device) after a warm-up epoch with the HD95 pass off, on, off, on; only the
`enable_lesionwise_hd95` switch differs between the epochs.  Off is `evaluation.lesionwise.enable=true` alone, on is the same
plus `hd95.enable=true`: the ratio is what the HD95 pass adds to a run that already scores lesion-wise.  Writes one JSON
document: volumes/s of every epoch, the mean of each arm, the on / off ratio and the lesion-wise figures of the last `on`
epoch.

Expectation: the voxel passes (edges, roots, pool, fill; two walks of the pair table) move about 0.1 KB per voxel, like the
lesion-wise scores themselves; the brute-force pass evaluates, per direction, sum over the (component, lesion) pairs of
|edge(c)| |edge(A_g)| distances in fp64 and is the part nobody can predict from the shape: it depends on the masks.

usage: python scripts/bench_lesionwise_hd95.py [--volumes 96] [--pool 24] [--out profiles/lesionwise_hd95_bench.json]
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
    ap.add_argument("--min-lesion-voxels", type=int, default=0)
    ap.add_argument("--percentile", type=float, default=95.0)
    ap.add_argument("--penalty", default="diagonal", help="diagonal, or a positive number (BraTS-2023: 374)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "lesionwise_hd95_bench.json"))
    a = ap.parse_args()

    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.models import UNet
    from multimodal_tta_amd.registry import get_evaluation_strategy
    from multimodal_tta_amd.synth import synth_volume

    device = torch.device("cuda", 0)
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])
    cfg["model"] = dict(MODEL)
    cfg["method"].update(steps=a.steps, precision="bf16", lanes=a.lanes, group=a.group)
    cfg["evaluation"]["loss"]["report_loss"] = False
    cfg["evaluation"]["lesionwise"] = {"enable": True, "dilation": a.dilation, "dilation_connectivity": a.dilation_connectivity,
                                       "min_lesion_voxels": a.min_lesion_voxels,
                                       "hd95": {"enable": True, "percentile": a.percentile,
                                                "penalty": a.penalty if a.penalty == "diagonal" else float(a.penalty)}}
    torch.manual_seed(42)
    model = UNet(MODEL)
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)

    shape = tuple(a.shape)
    pool = [synth_volume(i, 4, shape, 3) for i in range(a.pool)]
    xs = [v["image"].unsqueeze(0).to(device) for v in pool]
    ys = [v["label"].unsqueeze(0).to(device) for v in pool]
    loader = [{"image": xs[i % a.pool], "label": ys[i % a.pool], "domain": ["synth"], "index": [i]} for i in range(a.volumes)]

    def epoch(on):
        strat.enable_lesionwise_hd95 = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = strat.evaluate_epoch(model, loader, device)
        torch.cuda.synchronize()
        return a.volumes / (time.perf_counter() - t0), m

    epoch(True)                                          # warm-up: lanes, graph capture, allocator
    epochs, last_on = [], {}
    for on in (False, True, False, True):
        rate, m = epoch(on)
        epochs.append({"lesionwise_hd95": on, "volumes_per_s": round(rate, 2)})
        if on:
            last_on = {k: m[k] for k in ("avg_dc", "avg_lw_dc", "avg_lw_hd95", "et_lw_hd95", "tc_lw_hd95", "wt_lw_hd95",
                                         "wt_lw_hd95_overflow", "wt_lesions", "wt_lesions_found", "wt_fp_components")}
    off = sum(e["volumes_per_s"] for e in epochs if not e["lesionwise_hd95"]) / 2
    on_ = sum(e["volumes_per_s"] for e in epochs if e["lesionwise_hd95"]) / 2
    result = {"workload": f"unet INSTANCE 4x{shape[0]}x{shape[1]}x{shape[2]} S={a.steps} bf16, {a.lanes} lanes x group {a.group}, "
                          f"{a.volumes} volumes per epoch, dilation {a.dilation} x {a.dilation_connectivity}, "
                          f"min_lesion_voxels {a.min_lesion_voxels}, percentile {a.percentile}, penalty {a.penalty}",
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
