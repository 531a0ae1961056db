"""Tent (`entmin_tta`) and CRF-regularised Tent (`crf_tta`) on the bench U-Net, inside ONE process on one GPU, in the order
Tent / CRF / Tent / CRF: adapted volumes/s and peak device memory of each arm, the mean rate of each method, the CRF rate as a
fraction of the Tent rate with both arms' spread, and the last step's entropy and pairwise term of the last group.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  Every step of the CRF arm stores its logits (it gives up
the head-loss epilogue of the last convolution) and runs one stencil pass over them in place of the entropy pass.  The arms
run one after another on the same seeded volumes (each is built, warmed up - graph capture -, timed over at least --volumes
volumes and released).  Prints one JSON line and writes it to --out.

usage: python scripts/bench_crf.py [--lanes 3] [--group 8] [--volumes 96] [--weight 1] [--sigma 1] [--out profiles/crf_bench.json]
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
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--volumes", type=int, default=96)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--weight", type=float, default=1.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--connectivity", type=int, default=26)
    ap.add_argument("--form", default="potts")
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "crf_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    crf = ("crf", {"weight": a.weight, "sigma": a.sigma, "connectivity": a.connectivity, "form": a.form})
    last = {}

    class CrfMethod(Method):
        def round(self, xs):
            n = super().round(xs)
            last["result"] = self.result
            return n

    makers = {"entmin": lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps),
              "crf": lambda: CrfMethod("tta_crf", a.lanes, a.group, streams, device, a.steps, crf)}
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "group": a.group, **crf[1], "arms": []}
    rates = {name: [] for name in makers}
    for _ in range(2):
        for name, make in makers.items():
            rate, peak, n = measure(make, xs, a.volumes, device)
            rates[name].append(rate)
            out["arms"].append({"method": name, "volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n})
    mean = {name: sum(r) / len(r) for name, r in rates.items()}
    for name in makers:
        out[f"{name}_volumes_per_s"] = round(mean[name], 2)
        out[f"{name}_spread"] = round((max(rates[name]) - min(rates[name])) / mean[name], 4)
    out["crf_over_entmin"] = round(mean["crf"] / mean["entmin"], 3)
    for key in ("entropy", "pairwise"):
        hist = last["result"][key].float()
        out[f"{key}_first_step"] = round(float(hist[0].mean().item()), 6)
        out[f"{key}_last_step"] = round(float(hist[-1].mean().item()), 6)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
