"""CoTTA (`cotta_tta`) at V = 4 with the mirror group (`mirror_axes: [h, w]`) against two coded + two affine views
(`mirror_axes: [h]`, `affine: {views: 2, ...}`) on the bench U-Net, inside ONE process on one GPU, each arm TWICE (mirror,
affine, mirror, affine): adapted volumes/s and peak device memory of each run, the affine rate as a fraction of the
mirrored one and the spread of the repeated arms.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 2) with 4 views each.  The step is four teacher forwards, the student's forward
and backward and two repacks in both arms; what differs is the ensemble (`mmtta_affine_ensemble` reads V x 16 B per voxel and
writes 16 B like `mmtta_memo_ensemble`, plus cached corner reads and 8x the sigmoids on the affine views) and, once per volume,
the staging of two resampled views.  From bytes a ratio near 1 is the expectation.  The arms run one after another on the same
seeded volumes (each is built, warmed up - graph capture -, timed over at least --volumes volumes and released).  Prints one
JSON line; `--out` also writes it to a file.

usage: python scripts/bench_affine.py [--lanes 3] [--group 2] [--volumes 48] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402
from method_bench import Method, measure  # noqa: E402

OFF = {"views": 0, "rotate": [0.0, 0.0, 0.0], "scale": 0.0, "translate": [0.0, 0.0, 0.0], "seed": 0}
ON = {"views": 2, "rotate": [10.0, 10.0, 10.0], "scale": 0.1, "translate": [2.0, 2.0, 2.0], "seed": 0}
ARMS = {"mirror": {"mirror_axes": ["h", "w"], "affine": OFF}, "affine": {"mirror_axes": ["h"], "affine": ON}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=2)
    ap.add_argument("--volumes", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16 V=4", "lanes": a.lanes,
           "group": a.group, "affine_block": ON, "runs": []}
    rates = {name: [] for name in ARMS}
    for _ in range(2):
        for name, views in ARMS.items():
            r, p, n = measure(lambda: Method("tta_cotta", a.lanes, a.group, streams, device, a.steps, ("cotta", views)), xs,
                              a.volumes, device)
            out["runs"].append({"arm": name, "volumes_per_s": r, "peak_memory_gb": p, "timed_volumes": n})
            rates[name].append(r)
    mean = {name: sum(v) / len(v) for name, v in rates.items()}
    out["affine_over_mirror"] = round(mean["affine"] / mean["mirror"], 3)
    out["spread_of_repeats"] = {name: round((max(v) - min(v)) / mean[name], 4) for name, v in rates.items()}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
