"""Tent (`entmin_tta`) and BNM (`bnm_tta`) on the bench U-Net, inside ONE process on one GPU, in the order
Tent / BNM whole-volume / Tent / BNM [16,16,16]: adapted volumes/s and peak device memory of each arm, the mean Tent rate with
the spread of its two arms, each BNM arm's rate as a fraction of it, and the first and last step's entropy and nuclear term of
the last group of each BNM arm.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  Every step of a BNM arm stores its logits (it gives up
the head-loss epilogue of the last convolution) and runs the Gram, spectrum and gradient passes over them in place of the
entropy pass.  The arms run one after another on the same seeded volumes (each is built, warmed up - graph capture -, timed
over at least --volumes volumes and released).  Prints one JSON line and writes it to --out.

usage: python scripts/bench_bnm.py [--lanes 3] [--group 8] [--volumes 96] [--weight 1] [--out profiles/bnm_bench.json]
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
    ap.add_argument("--entropy-weight", type=float, default=1.0)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--block", type=int, nargs=3, default=[16, 16, 16], help="the regional arm's box")
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bnm_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    common = {"weight": a.weight, "entropy_weight": a.entropy_weight, "eps": a.eps}
    last = {}

    class BnmMethod(Method):
        def round(self, xs):
            n = super().round(xs)
            last["result"] = self.result
            return n

    def bnm(block):
        return lambda: BnmMethod("tta_bnm", a.lanes, a.group, streams, device, a.steps, ("bnm", dict(common, block=list(block))))

    entmin = lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps)
    arms = [("entmin", entmin), ("bnm_whole", bnm([0, 0, 0])), ("entmin", entmin), ("bnm_regional", bnm(a.block))]
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "group": a.group, **common, "regional_block": list(a.block), "arms": []}
    rates = {}
    for name, make in arms:
        rate, peak, n = measure(make, xs, a.volumes, device)
        rates.setdefault(name, []).append(rate)
        out["arms"].append({"method": name, "volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n})
        if name != "entmin":
            for key in ("entropy", "nuclear"):
                hist = last["result"][key].float()
                out[f"{name}_{key}_first_step"] = round(float(hist[0].mean().item()), 6)
                out[f"{name}_{key}_last_step"] = round(float(hist[-1].mean().item()), 6)
    mean = sum(rates["entmin"]) / len(rates["entmin"])
    out["entmin_volumes_per_s"] = round(mean, 2)
    out["entmin_spread"] = round((max(rates["entmin"]) - min(rates["entmin"])) / mean, 4)
    for name in ("bnm_whole", "bnm_regional"):
        out[f"{name}_volumes_per_s"] = round(rates[name][0], 2)
        out[f"{name}_over_entmin"] = round(rates[name][0] / mean, 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
