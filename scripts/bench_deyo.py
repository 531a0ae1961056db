"""Tent (`entmin_tta`), SAR (`sar_tta`) and DeYO (`deyo_tta`) on the bench U-Net, inside ONE process on one GPU, in the order
Tent / SAR / DeYO / Tent / SAR / DeYO: adapted volumes/s and peak device memory of each arm, the mean rate of each method,
the DeYO rate as a fraction of the Tent and of the SAR rate, and the shares of the elements DeYO's two filters keep.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  A Tent step is one forward, one input-gradient pass and
one weight-gradient pass; SAR runs two forwards and two backwards per step, DeYO two forwards and one backward - by operation
count about 3/4 of the Tent rate, and strictly less work than SAR.  The arms run one after another on the same seeded
volumes (each is built, warmed up - graph capture -, timed over at least --volumes volumes and released).  Prints one JSON
line and writes it to --out.

usage: python scripts/bench_deyo.py [--lanes 3] [--group 8] [--volumes 96] [--patches 4 4 4] [--out profiles/deyo_bench.json]
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
    ap.add_argument("--e-margin", type=float, default=0.5)
    ap.add_argument("--e-margin0", type=float, default=0.4)
    ap.add_argument("--plpd-threshold", type=float, default=0.2)
    ap.add_argument("--patches", type=int, nargs=3, default=[4, 4, 4])
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "deyo_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    deyo = ("deyo", {"e_margin": a.e_margin, "e_margin0": a.e_margin0, "plpd_threshold": a.plpd_threshold,
                     "patches": list(a.patches)})
    shares = {}

    class DeyoMethod(Method):
        def round(self, xs):
            n = super().round(xs)
            shares["last"] = self.result
            return n

    makers = {"entmin": lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps),
              "sar": lambda: Method("tta_sar", a.lanes, a.group, streams, device, a.steps),
              "deyo": lambda: DeyoMethod("tta_deyo", a.lanes, a.group, streams, device, a.steps, deyo)}
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "group": a.group, "e_margin": a.e_margin, "e_margin0": a.e_margin0, "plpd_threshold": a.plpd_threshold,
           "patches": list(a.patches), "arms": []}
    rates = {name: [] for name in makers}
    for _ in range(2):
        for name, make in makers.items():
            rate, peak, n = measure(make, xs, a.volumes, device)
            rates[name].append(rate)
            out["arms"].append({"method": name, "volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n})
    mean = {name: sum(r) / len(r) for name, r in rates.items()}
    for name in makers:
        out[f"{name}_volumes_per_s"] = round(mean[name], 2)
    out["deyo_over_entmin"] = round(mean["deyo"] / mean["entmin"], 3)
    out["deyo_over_sar"] = round(mean["deyo"] / mean["sar"], 3)
    out["sar_over_entmin"] = round(mean["sar"] / mean["entmin"], 3)
    elems = a.shape[0] * a.shape[1] * a.shape[2] * 3
    r = shares["last"]
    for key in ("kept_entropy", "kept"):
        f = r[key].float() / elems
        out[f"deyo_{key}_fraction_first_last_step"] = [round(f[0].mean().item(), 4), round(f[-1].mean().item(), 4)]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
