"""Tent (`entmin_tta`) without and with the do-no-harm guard (`method.guard`) on the bench U-Net, inside ONE process on one
GPU, in the order Tent / guarded Tent / Tent / guarded Tent: adapted volumes/s and peak device memory of each arm, the mean
rate of each, the guarded rate as a fraction of the Tent rate with both arms' spread, and what the guard saw on the last
round (fall-backs, share of flipped elements).

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  The guard adds one eval-mode forward before the first
step (about 1 in 32 forward-equivalents at S = 10: the estimate from the operation count is 31/32 = 0.97 of the Tent
rate), a copy of the logits and two streaming passes over them behind the last step; the steps themselves are unchanged.
The arms run one after another on the same seeded volumes (each is built, warmed up - graph capture -, timed over at least
--volumes volumes and released).  Prints one JSON line and writes it to --out.

usage: python scripts/bench_guard.py [--lanes 3] [--group 8] [--volumes 96] [--out profiles/guard_bench.json]
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
    ap.add_argument("--scope", default="volume")
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "guard_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    guard = ("guard", {"enable": True, "scope": a.scope})          # the shipped thresholds
    last = {}

    class GuardedMethod(Method):
        def round(self, xs):
            n = super().round(xs)
            last["result"] = self.result
            return n

    makers = {"entmin": lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps),
              "guarded": lambda: GuardedMethod("tta_entmin", a.lanes, a.group, streams, device, a.steps, guard)}
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "group": a.group, "scope": a.scope, "arms": []}
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
    out["guarded_over_entmin"] = round(mean["guarded"] / mean["entmin"], 3)
    out["estimate_from_operation_count"] = round(31.0 / 32.0, 3)
    res = last["result"]
    s, adapted, both = res["guard_counts"].unbind(-1)
    elems = a.shape[0] * a.shape[1] * a.shape[2] * 3
    out["fallback_fraction"] = round(float(res["guard_fallback"].float().mean().item()), 4)
    out["flipped_fraction"] = round(float((s + adapted - 2 * both).sum(-1).float().mean().item()) / elems, 5)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
