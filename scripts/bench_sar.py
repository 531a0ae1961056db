"""Tent (`entmin_tta`) against SAR (`sar_tta`) on the bench U-Net, inside ONE process on one GPU: adapted volumes/s of each
objective and the SAR rate as a fraction of the Tent rate.

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  SAR runs two forward / backward passes per step, so
about half the Tent rate is the expectation.  Both plugins adapt the same seeded volumes, alternated round by round after a
warm-up (graph capture), with at least --volumes timed volumes each.  Prints one JSON line.

usage: python scripts/bench_sar.py [--lanes 3] [--group 8] [--volumes 48] [--e-margin 0.4] [--rho 0.05]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_tta_amd import _lib  # noqa: E402
from method_bench import Method  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--volumes", type=int, default=48)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--e-margin", type=float, default=0.4)
    ap.add_argument("--rho", type=float, default=0.05)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.synth import synth_volume
    _lib.load()
    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    n_in = a.lanes * a.group
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(n_in)]).to(device)
    sar = ("sar", {"e_margin": a.e_margin, "rho": a.rho})
    methods = {"entmin_tta": Method("tta_entmin", a.lanes, a.group, streams, device, a.steps),
               "sar_tta": Method("tta_sar", a.lanes, a.group, streams, device, a.steps, sar)}
    for m in methods.values():                          # warm-up: capture
        m.round(xs)
    torch.cuda.synchronize()
    t = {name: 0.0 for name in methods}
    n = {name: 0 for name in methods}
    while min(n.values()) < a.volumes:                  # alternated, one round per method and turn
        for name, m in methods.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n[name] += m.round(xs)
            torch.cuda.synchronize()
            t[name] += time.perf_counter() - t0
    rate = {k: round(n[k] / t[k], 2) for k in n}
    elems = a.shape[0] * a.shape[1] * a.shape[2] * 3
    kept = methods["sar_tta"].result["kept"].float() / elems
    print(json.dumps({"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16",
                      "lanes": a.lanes, "group": a.group, "e_margin": a.e_margin, "rho": a.rho, "timed_volumes": n,
                      "entmin_volumes_per_s": rate["entmin_tta"], "sar_volumes_per_s": rate["sar_tta"],
                      "sar_over_entmin": round(rate["sar_tta"] / rate["entmin_tta"], 3),
                      "sar_kept_fraction_first_last_step": [round(kept[0].mean().item(), 4), round(kept[-1].mean().item(), 4)],
                      "peak_memory_gb": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2)}), flush=True)


if __name__ == "__main__":
    main()
