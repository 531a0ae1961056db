"""Tent (`entmin_tta`), MEMO (`memo_tta`) at V = 4 mirrored views and the modality-consistency objective (`modcons_tta`) at
V = 5 leave-one-out views on the bench U-Net, inside ONE process on one GPU, in the order Tent / MEMO / modcons / modcons:
adapted volumes/s and peak device memory of each arm, the rate per view (rate x V) of MEMO and of modcons as fractions of
the Tent rate and of each other, and the run-to-run spread of the two modcons arms.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision.
Tent runs lanes x group volumes in flight (default 3 x 8, what bench.py runs), MEMO and modcons lanes x view-group (default
3 x 2) with V views each.  V views cost V forward / backward passes; the loss pass of modcons moves V x (16 + 8) B per voxel
(fp32 logits read, bf16 gradients written: about 250 MB per volume and step at V = 5) next to them, so a rate per view close
to MEMO's is the expectation.  The arms run one after another on the same seeded volumes (each is built, warmed up - graph
capture -, timed over at least --volumes volumes and released).  Prints one JSON line and writes it to --out.

usage: python scripts/bench_modcons.py [--lanes 3] [--group 8] [--view-group 2] [--volumes 48] [--out profiles/modcons_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402
from method_bench import AXES, Method, measure  # noqa: E402

MEMO_V = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--view-group", type=int, default=2)
    ap.add_argument("--subsets", default="leave_one_out", choices=["leave_one_out", "single"])
    ap.add_argument("--volumes", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "modcons_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    n_in = a.lanes * max(a.group, a.view_group)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(n_in)]).to(device)
    last = {}

    class ModconsMethod(Method):
        def round(self, xs):
            n = super().round(xs)
            last["result"], last["views"] = self.result, self.plugs[0].views
            return n

    entmin = lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps)
    memo = lambda: Method("tta_memo", a.lanes, a.view_group, streams, device, a.steps,
                          ("memo", {"mirror_axes": AXES[MEMO_V], "ensemble": False}))
    modcons = lambda: ModconsMethod("tta_modcons", a.lanes, a.view_group, streams, device, a.steps,
                                    ("modcons", {"subsets": a.subsets}))
    arms = [("entmin", entmin, 1), ("memo", memo, MEMO_V), ("modcons", modcons, None), ("modcons", modcons, None)]
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "group": a.group, "view_group": a.view_group, "subsets": a.subsets, "arms": []}
    rates = {}
    for name, make, views in arms:
        rate, peak, n = measure(make, xs, a.volumes, device)
        views = last["views"] if views is None else views
        rates.setdefault(name, []).append(rate * views)
        out["arms"].append({"method": name, "views": views, "volumes_per_s": rate, "views_per_s": round(rate * views, 2),
                            "peak_memory_gb": peak, "timed_volumes": n})
    r = last["result"]
    for key in ("losses", "entropy", "consistency"):
        hist = r[key].float()
        out[f"modcons_{key}_first_step"] = round(float(hist[0].mean().item()), 6)
        out[f"modcons_{key}_last_step"] = round(float(hist[-1].mean().item()), 6)
    out["modcons_disagree_volume0_last_step"] = [int(v) for v in r["disagree"][-1, 0].tolist()]
    mean = sum(rates["modcons"]) / len(rates["modcons"])
    out["entmin_volumes_per_s"] = rates["entmin"][0]
    out["memo_views_per_s"] = round(rates["memo"][0], 2)
    out["modcons_views_per_s"] = round(mean, 2)
    out["modcons_spread"] = round((max(rates["modcons"]) - min(rates["modcons"])) / mean, 4)
    out["memo_per_view_over_entmin"] = round(rates["memo"][0] / rates["entmin"][0], 3)
    out["modcons_per_view_over_entmin"] = round(mean / rates["entmin"][0], 3)
    out["modcons_per_view_over_memo"] = round(mean / rates["memo"][0], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
