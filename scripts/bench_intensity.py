"""MEMO (`memo_tta`) at V = 4 views on the bench U-Net with the views made three ways, inside ONE process on one GPU:
mirrors alone (`mirror_axes: [h, w]`), `[h]` x `copies: 2` with scale, shift, gamma and noise all on, and `[]` x `copies: 4`.
Adapted volumes/s and peak device memory of each, and the intensity rates as fractions of the mirror-only rate.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group = 3 x 2 (tta_memo.yaml's).  The views are staged once per volume - (1 + V) input rows moved per voxel,
against S forward / backward passes over V views - so rates equal to the mirror-only run within the noise of the machine
are the expectation; that is arithmetic, the JSON line is the measurement.  The methods run one after another on the same
seeded volumes (each is built, warmed up - graph capture -, timed over at least --volumes volumes and released).  Prints one
JSON line; `--out` also writes it to a file.

usage: python scripts/bench_intensity.py [--lanes 3] [--group 2] [--volumes 48] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402
from method_bench import Method, measure  # noqa: E402

ALL_ON = dict(scale=0.1, shift=0.1, gamma=0.3, noise_std=0.05)
CASES = {
    "mirror_hw": {"mirror_axes": ["h", "w"]},
    "h_x_copies2": {"mirror_axes": ["h"], "intensity": dict(copies=2, **ALL_ON)},
    "copies4": {"mirror_axes": [], "intensity": dict(copies=4, **ALL_ON)},
}


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
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16, memo_tta V=4", "lanes": a.lanes,
           "group": a.group, "cases": {}}
    base = None
    for name, section in CASES.items():
        memo = ("memo", dict(section, ensemble=False))
        r, p, n = measure(lambda: Method("tta_memo", a.lanes, a.group, streams, device, a.steps, memo), xs, a.volumes, device)
        base = r if base is None else base
        out["cases"][name] = {"memo": section, "volumes_per_s": r, "peak_memory_gb": p, "timed_volumes": n,
                              "over_mirror_only": round(r / base, 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
