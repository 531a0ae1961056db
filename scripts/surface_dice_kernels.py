"""The two NSD entry points alone, for a kernel trace: `ops.surface_dice` and `ops.lesionwise_nsd` (which queues
`mmtta_lesionwise_scores` first) on 8 synthetic volumes x 3 regions x 128^3 in one call, as a group of the bench scores them.

Two sets of masks: `speckle`, what the untrained bench model predicts (about 60 % of a volume, more than half of its voxels
surface, one component that holds nearly everything: the worst case of the lesion-wise passes), and `compact`, the ground
truth moved by one voxel (a prediction whose surface is the size of the lesion's).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/surface_dice_kernels.py

Prints one JSON line: per set the event-timed average per call of the region pass, of the lesion-wise scores alone and of
the lesion-wise scores with the NSD pass behind them, in ms."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=8)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tolerances", type=float, nargs="+", default=[1.0])
    ap.add_argument("--lesion-tolerances", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--spacing", type=float, nargs=3, default=[1.0, 1.0, 1.0])
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    device = torch.device("cuda", 0)
    shape = tuple(a.shape)
    label = torch.stack([synth_volume(i, 4, shape, 3)["label"] for i in range(a.volumes)]).float().to(device)
    gen = torch.Generator(device=device).manual_seed(7)
    masks = {"speckle": (torch.rand(label.shape, generator=gen, device=device) < 0.6).to(torch.uint8),
             "compact": torch.roll(label > 0.5, 1, dims=4).to(torch.uint8).contiguous()}
    out = {"masks": a.volumes * 3, "shape": list(shape), "tolerances": a.tolerances, "lesion_tolerances": a.lesion_tolerances,
           "radius": {"region": ops.surface_dice_radius(a.spacing, max(a.tolerances)),
                      "lesion": ops.surface_dice_radius(a.spacing, max(a.lesion_tolerances))}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for name, m in masks.items():
        t = [0.0, 0.0, 0.0]
        for rep in range(a.reps + 1):
            ev[0].record()
            counts = ops.surface_dice(m, label, a.spacing, a.tolerances)
            ev[1].record()
            ops.lesionwise_scores(m, label, 3, 18, 0)
            ev[2].record()
            res = ops.lesionwise_nsd(m, label, 3, 18, 0, a.spacing, a.lesion_tolerances)
            ev[3].record()
            torch.cuda.synchronize()
            if rep > 0:          # (the first call warms up)
                for k in range(3):
                    t[k] += ev[k].elapsed_time(ev[k + 1])
        c = counts.sum((0, 1))[0].tolist()
        out[name] = {"surface_dice_ms": round(t[0] / a.reps, 3), "lesionwise_scores_ms": round(t[1] / a.reps, 3),
                     "lesionwise_scores_and_nsd_ms": round(t[2] / a.reps, 3), "edge_pred": c[1], "edge_gt": c[3],
                     "nsd": round((c[0] + c[2]) / max(1, c[1] + c[3]), 4),
                     "lesions_scored": int(res["stats"][..., 2].sum())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
