"""Tent (`entmin_tta`) and the bias field (`biasfield_tta`) on the bench U-Net, inside ONE process on one GPU, in the order
Tent / biasfield order 2 with `params: all` / Tent / biasfield order 3 with `params: []` (the frozen network): adapted
volumes/s and peak device memory of each arm, the mean Tent rate with the spread of its two arms, each biasfield arm's rate as
a fraction of it, and the first and last step's loss and the final coefficients of volume 0 of each biasfield arm.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  The bytes are the input normaliser's: every step of a
biasfield arm writes x' from the raw volume (34 MB read, 17 MB written per volume) and, after the backward, gathers the
first level's reduced input gradient (34 MB of x and 2 x 17 MB of dy read, about 1.8 GMAC): about 120 MB next to the step's
3.9 GB per volume.  The field adds K fused multiply-adds per voxel and channel to both passes (K = 10 / 20 terms), an expf per
voxel and channel, and 4 K fp64 sums per tile to the gradient.  Estimate, written down before the first run: the input
normaliser measured 0.90 of the Tent rate (its gather 75 us per volume and step), so its ratio or slightly below.  The frozen
arm runs the whole backward for its input gradient but no weight gradient and no optimizer.  The arms run one after another
on the same seeded volumes (each is built, warmed up - graph capture -, timed over at least --volumes volumes and released).
Prints one JSON line and writes it to --out.

usage: python scripts/bench_biasfield.py [--lanes 3] [--group 8] [--volumes 96] [--out profiles/biasfield_bench.json]
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
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--anchor", default="min", choices=["min", "zero"])
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "biasfield_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    common = {"lr": a.lr, "anchor": a.anchor}
    last = {}

    class FieldMethod(Method):
        def round(self, xs):
            n = super().round(xs)
            last["result"] = self.result
            return n

    def field(order, params):
        return lambda: FieldMethod("tta_biasfield", a.lanes, a.group, streams, device, a.steps,
                                   ("biasfield", dict(common, order=order)), overrides={"params": params})

    entmin = lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps)
    arms = [("entmin", entmin), ("biasfield_o2_all", field(2, "all")), ("entmin", entmin), ("biasfield_o3_frozen", field(3, []))]
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "group": a.group, **common, "arms": []}
    rates = {}
    for name, make in arms:
        rate, peak, n = measure(make, xs, a.volumes, device)
        rates.setdefault(name, []).append(rate)
        out["arms"].append({"method": name, "volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n})
        if name != "entmin":
            r = last["result"]
            hist = r["losses"].float()
            out[f"{name}_loss_first_step"] = round(float(hist[0].mean().item()), 6)
            out[f"{name}_loss_last_step"] = round(float(hist[-1].mean().item()), 6)
            out[f"{name}_coeff_volume0"] = [[round(float(v), 4) for v in row] for row in r["field_coeff"][0].tolist()]
    mean = sum(rates["entmin"]) / len(rates["entmin"])
    out["entmin_volumes_per_s"] = round(mean, 2)
    out["entmin_spread"] = round((max(rates["entmin"]) - min(rates["entmin"])) / mean, 4)
    for name in ("biasfield_o2_all", "biasfield_o3_frozen"):
        out[f"{name}_volumes_per_s"] = round(rates[name][0], 2)
        out[f"{name}_over_entmin"] = round(rates[name][0] / mean, 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
