"""Tent (`entmin_tta`), Tent with the fused weight-gradient update off and EATA (`eata_tta`, lambda > 0, Fisher estimate from
one group of volumes) on the bench U-Net, inside ONE process on one GPU: adapted volumes/s and peak device memory of each,
the EATA rate as a fraction of both Tent rates, and the time the Fisher estimate took (`fisher_estimate_s`: one cold call
for one group of volumes, buffer allocation and workspace sizing included).

Workload: channels [32, 64, 128, 256, 512], 2 residual units, norm INSTANCE, 4 x 128^3 volumes, S = 10, bf16 precision,
lanes x group volumes in flight (default 3 x 8, what bench.py runs).  EATA takes its gradient with the separate
weight-gradient passes (the penalty is added to the gradient in the arena), so Tent with `fused_update = False` is the
like-for-like baseline: against it EATA adds the penalty pass (20 B per parameter, replica and step) and two more launches of
the objective.  The methods run one after another on the same seeded volumes (each is built, warmed up - graph capture -,
timed over at least --volumes volumes and released).  Prints one JSON line and writes it to --out.

usage: python scripts/bench_eata.py [--lanes 3] [--group 8] [--volumes 96] [--fisher-alpha 2000] [--out profiles/eata_bench.json]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--e-margin", type=float, default=0.4)
    ap.add_argument("--fisher-alpha", type=float, default=2000.0)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "eata_bench.json"))
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import register_plugin
    from multimodal_tta_amd.synth import synth_volume
    from multimodal_tta_amd.tta import EntropyMinimizationTTA
    _lib.load()

    @register_plugin("entmin_unfused_tta")
    class UnfusedTent(EntropyMinimizationTTA):
        fused_update = False

    def unfused():          # tta_entmin's config, the subclass above as its plugin
        m = Method("tta_entmin", a.lanes, a.group, streams, device, a.steps, None, "entmin_unfused_tta")
        assert all(type(p) is UnfusedTent and not p.rt.fused_layers for p in m.plugs), "the baseline runs the fused update"
        return m

    fisher_s = {}

    class EataMethod(Method):
        def __init__(self, *args):
            super().__init__(*args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.plugs[0].estimate_fisher([xs[:self.group]])
            torch.cuda.synchronize()
            fisher_s["s"] = time.perf_counter() - t0
            for p in self.plugs[1:]:
                p.set_fisher(self.plugs[0].fisher, self.plugs[0].fisher_count)

    device = torch.device("cuda", 0)
    streams = ops.lane_streams(a.lanes, device)
    xs = torch.stack([synth_volume(i, 4, tuple(a.shape), 3)["image"] for i in range(a.lanes * a.group)]).to(device)
    eata = ("eata", {"e_margin": a.e_margin, "fisher_alpha": a.fisher_alpha})
    runs = {"entmin": lambda: Method("tta_entmin", a.lanes, a.group, streams, device, a.steps),
            "entmin_unfused": unfused,
            "eata": lambda: EataMethod("tta_eata", a.lanes, a.group, streams, device, a.steps, eata)}
    out = {"workload": f"unet INSTANCE {a.shape[0]}x{a.shape[1]}x{a.shape[2]} S={a.steps} bf16", "lanes": a.lanes,
           "group": a.group, "e_margin": a.e_margin, "fisher_alpha": a.fisher_alpha}
    for name, make in runs.items():
        rate, peak, n = measure(make, xs, a.volumes, device)
        out[name] = {"volumes_per_s": rate, "peak_memory_gb": peak, "timed_volumes": n}
    out["eata_over_entmin"] = round(out["eata"]["volumes_per_s"] / out["entmin"]["volumes_per_s"], 3)
    out["eata_over_entmin_unfused"] = round(out["eata"]["volumes_per_s"] / out["entmin_unfused"]["volumes_per_s"], 3)
    out["fisher_estimate_s"] = round(fisher_s["s"], 3)
    out["fisher_volumes"] = a.group
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
