"""Whole-volume Tent (`entmin_tta`) against sliding-window Tent (`window_tta`) on the bench U-Net at a volume larger than the
training patch, inside ONE process on one GPU, in the order Tent / window / Tent / window: adapted volumes/s and peak device
memory of each arm, the window rate as a fraction of the whole-volume rate, and the run-to-run spread of the repeated arms.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 160 x 192 x 160 volumes (the full BraTS
volume, every extent divisible by 16, so the whole-volume arm can run it), S = 10, bf16 precision.  Tent runs lanes x group
whole volumes in flight (default 3 x 2), window_tta lanes x window-group volumes (default 3 x 1) with W_n = 8 windows of 128^3
each at overlap 0.5.  The windows hold 8 x 128^3 = 16.8 M voxels for the volume's 4.9 M: the expectation from the operation
count is 0.29 of the whole-volume rate; the crop, loss and blend passes stream 0.2 - 0.4 GB each next to milliseconds of
convolutions.  The arms run one after another on the same seeded volumes (each is built, warmed up - graph capture -, timed
over at least --volumes volumes and released).  Prints one JSON line and writes it to --out.

usage: python scripts/bench_window.py [--lanes 3] [--group 2] [--window-group 1] [--volumes 96] [--out profiles/window_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402
from method_bench import Method, measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=2)
    ap.add_argument("--window-group", type=int, default=1)
    ap.add_argument("--volumes", type=int, default=96)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[160, 192, 160])
    ap.add_argument("--roi", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--overlap", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "window_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    n_in = a.lanes * max(a.group, a.window_group)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(n_in)]).to(device)
    last = {}

    class WindowMethod(Method):
        def round(self, xs):
            n = super().round(xs)
            last["result"] = self.result
            return n

    entmin = lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps)
    window = lambda: WindowMethod("tta_window", a.lanes, a.window_group, streams, device, a.steps,
                                  ("window", {"roi": list(a.roi), "overlap": a.overlap}))
    arms = [("entmin", entmin), ("window", window), ("entmin", entmin), ("window", window)]
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "roi": list(a.roi),
           "overlap": a.overlap, "lanes": a.lanes, "group": a.group, "window_group": a.window_group, "arms": []}
    rates = {}
    for name, make in arms:
        rate, peak, n = measure(make, xs, a.volumes, device)
        rates.setdefault(name, []).append(rate)
        out["arms"].append({"method": name, "volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n})
    r = last["result"]
    out["windows"] = int(r["windows"])
    out["window_loss_first_step"] = round(float(r["losses"].float()[0].mean().item()), 6)
    out["window_loss_last_step"] = round(float(r["losses"].float()[-1].mean().item()), 6)
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    for k, v in rates.items():
        out[f"{k}_volumes_per_s"] = round(mean[k], 2)
        out[f"{k}_spread"] = round((max(v) - min(v)) / mean[k], 4)
    out["window_over_entmin"] = round(mean["window"] / mean["entmin"], 3)
    out["windows_per_s_over_entmin"] = round(mean["window"] * out["windows"] / mean["entmin"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
