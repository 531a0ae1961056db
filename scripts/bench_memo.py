"""Tent (`entmin_tta`) against MEMO (`memo_tta`) with V = 2, 4, 8 mirrored views on the bench U-Net, inside ONE process on
one GPU: adapted volumes/s and peak device memory of each, and the MEMO rates as fractions of the Tent rate.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision.
Tent runs lanes x group volumes in flight (default 3 x 8, what bench.py runs), MEMO lanes x memo-group (default 3 x 2) with V
views each.  V views cost V forward / backward passes, so a rate near Tent / V is the expectation.  The methods run one after
another on the same seeded volumes (each is built, warmed up - graph capture -, timed over at least --volumes volumes and
released, so that the peak-memory column is the method's own).  Prints one JSON line; `--out` also writes it to a file.

usage: python scripts/bench_memo.py [--lanes 3] [--group 8] [--memo-group 2] [--views 2 4 8] [--volumes 48] [--out FILE]
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
    ap.add_argument("--memo-group", type=int, default=2)
    ap.add_argument("--views", type=int, nargs="+", default=[2, 4, 8], choices=sorted(AXES))
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
    n_in = a.lanes * max(a.group, a.memo_group)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(n_in)]).to(device)
    rate, peak, n = measure(lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps), xs, a.volumes, device)
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "entmin": {"group": a.group, "volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n}, "memo": {}}
    for v in a.views:
        memo = ("memo", {"mirror_axes": AXES[v], "ensemble": False})
        r, p, n = measure(lambda: Method("tta_memo", a.lanes, a.memo_group, streams, device, a.steps, memo), xs, a.volumes,
                          device)
        out["memo"][f"V{v}"] = {"group": a.memo_group, "volumes_per_s": r, "peak_memory_gb": p, "timed_volumes": n,
                                "over_entmin": round(r / rate, 3), "over_entmin_per_view": round(r * v / rate, 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
