"""CoTTA (`cotta_tta`) against PETAL (`petal_tta`) on the bench U-Net, inside ONE process on one GPU, arms CoTTA / PETAL /
CoTTA / PETAL: adapted volumes/s and peak device memory of each arm, the spread between the two arms of a method (the noise
the ratio is read against) and the PETAL rate as a fraction of the CoTTA rate.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision, both
methods with V = 4 teacher views from mirror_axes [h, w] on the shipped lanes x group (3 x 2).  PETAL adds to a CoTTA step the
magnitude select (three reads of the gradient) and one more read of the gradient in the update pass: from bytes about 0.3 GB
per replica and step.  The arms run one after another on the same seeded volumes (each is built, warmed up - graph capture -,
timed over at least --volumes volumes and released).  Prints one JSON line; `--out` also writes it to a file.

usage: python scripts/bench_petal.py [--lanes 3] [--group 2] [--volumes 48] [--quantile 0.03] [--out profiles/petal_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402
from method_bench import AXES, Method, measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=2)
    ap.add_argument("--views", type=int, default=4, choices=sorted(AXES))
    ap.add_argument("--volumes", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--quantile", type=float, default=0.03)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    sections = {"cotta": ("tta_cotta", ("cotta", {"mirror_axes": AXES[a.views]})),
                "petal": ("tta_petal", ("petal", {"mirror_axes": AXES[a.views], "quantile": a.quantile}))}
    arms = []
    for name in ("cotta", "petal", "cotta", "petal"):
        method, section = sections[name]
        r, p, n = measure(lambda: Method(method, a.lanes, a.group, streams, device, a.steps, section), xs, a.volumes, device)
        arms.append({"method": name, "volumes_per_s": r, "peak_memory_gb": p, "timed_volumes": n})
    rate = {name: [arm["volumes_per_s"] for arm in arms if arm["method"] == name] for name in sections}
    mean = {name: sum(v) / len(v) for name, v in rate.items()}
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16 V={a.views}", "lanes": a.lanes,
           "group": a.group, "quantile": a.quantile, "arms": arms,
           "spread": {name: round(abs(v[0] - v[1]) / mean[name], 4) for name, v in rate.items()},
           "petal_over_cotta": round(mean["petal"] / mean["cotta"], 4)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
