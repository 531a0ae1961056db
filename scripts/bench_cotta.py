"""Tent (`entmin_tta`) against CoTTA (`cotta_tta`) with V = 1, 2, 4 teacher views on the bench U-Net, inside ONE process on
one GPU: adapted volumes/s and peak device memory of each, and the CoTTA rates as fractions of the Tent rate.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision.
Tent runs lanes x group volumes in flight (default 3 x 8, what bench.py runs), CoTTA lanes x cotta-group (default 3 x 2).  From
launch counts a CoTTA step is V teacher forwards + Tent's step (forward + backward, about 3 forwards' worth) + two repacks,
so a rate near Tent * 3 / (3 + V) is the expectation (`over_expected` is the measured rate over that figure).  The methods
run one after another on the same seeded volumes (each is built, warmed up - graph capture -, timed over at least --volumes
volumes and released, so that the peak-memory column is the method's own).  Prints one JSON line; `--out` also writes it to a
file.

usage: python scripts/bench_cotta.py [--lanes 3] [--group 8] [--cotta-group 2] [--views 1 2 4] [--volumes 48] [--out FILE]
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
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--cotta-group", type=int, default=2)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2, 4], choices=sorted(AXES))
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
    n_in = a.lanes * max(a.group, a.cotta_group)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(n_in)]).to(device)
    rate, peak, n = measure(lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps), xs, a.volumes, device)
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "entmin": {"group": a.group, "volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n}, "cotta": {}}
    for v in a.views:
        cotta = ("cotta", {"mirror_axes": AXES[v]})
        r, p, n = measure(lambda: Method("tta_cotta", a.lanes, a.cotta_group, streams, device, a.steps, cotta), xs,
                          a.volumes, device)
        out["cotta"][f"V{v}"] = {"group": a.cotta_group, "volumes_per_s": r, "peak_memory_gb": p, "timed_volumes": n,
                                 "over_entmin": round(r / rate, 3), "over_expected": round(r / (rate * 3.0 / (3.0 + v)), 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
