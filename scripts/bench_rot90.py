"""MEMO (`memo_tta`) and CoTTA (`cotta_tta`) at V = 4 with the mirror group (`mirror_axes: [h, w]`) against the rotation
group (`mirror_axes: [], rot90: {k: [1, 2, 3]}`) on the bench U-Net, inside ONE process on one GPU: adapted volumes/s and
peak device memory of each, and the rotated rate as a fraction of the mirrored one.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 2) with 4 views each.  The step is V forward / backward passes; the loss
(MEMO) and ensemble (CoTTA) kernels, which are what differs - the tiled, LDS-transposed forms against the mirror forms - are
about 1 % of it.  The methods run one after another on the same seeded volumes (each is built, warmed up - graph capture -,
timed over at least --volumes volumes and released).  Prints one JSON line; `--out` also writes it to a file.

usage: python scripts/bench_rot90.py [--lanes 3] [--group 2] [--volumes 48] [--methods memo cotta] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402
from method_bench import Method, measure  # noqa: E402

VIEWS = {"mirror": {"mirror_axes": ["h", "w"], "rot90": {"k": []}}, "rot90": {"mirror_axes": [], "rot90": {"k": [1, 2, 3]}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=2)
    ap.add_argument("--volumes", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--methods", nargs="+", default=["memo", "cotta"], choices=["memo", "cotta"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16 V=4", "lanes": a.lanes,
           "group": a.group}
    for method in a.methods:
        res = {}
        for name, views in VIEWS.items():
            r, p, n = measure(lambda: Method(f"tta_{method}", a.lanes, a.group, streams, device, a.steps, (method, views)), xs,
                              a.volumes, device)
            res[name] = {"volumes_per_s": r, "peak_memory_gb": p, "timed_volumes": n}
        res["rot90_over_mirror"] = round(res["rot90"]["volumes_per_s"] / res["mirror"]["volumes_per_s"], 3)
        out[method] = res
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
