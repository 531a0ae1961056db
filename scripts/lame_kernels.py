"""The refinement launches of ``mmtta_lame_refine`` on their own, tiled route and generic route on the same input, for a
kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/lame_kernels.py --size 128

Default: 1 volume x SIZE^3 x 3 regions (fp32 logits in 16-byte rows), 4 input channels in 8-byte bf16 rows (what bf16 precision
stages), connectivity 26, weight 1, sigma 1 and sigma 0, T = 10 iterations per call, --reps calls after one warm-up.  The generic
route is forced with MMTTA_OPT_LAME_TILED = 0 on the same tensors.  Prints the event-timed mean per launch of every arm as one
JSON line (the trace names the kernels: lame_tiled_kernel<affinity, softmax, bf16 input>, lame_generic_kernel).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPT_LAME_TILED = 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=1)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--softmax", action="store_true")
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    G, S, R, C, T = a.volumes, a.size, 3, 4, a.iterations
    gen = torch.Generator(device="cuda").manual_seed(0)
    l0 = ops.new_cl(G, S, S, S, R, "cuda", ldc=4, zero=True)
    l0.copy_(torch.randn((G, S, S, S, R), device="cuda", generator=gen) * 3.0)
    x = ops.new_cl(G, S, S, S, C, "cuda", ldc=4, dtype=torch.bfloat16)
    x.copy_(torch.randn((G, S, S, S, C), device="cuda", generator=gen).to(torch.bfloat16))
    out = ops.new_cl(G, S, S, S, R, "cuda", ldc=4, zero=True)
    work = ops.new_cl(G, S, S, S, R, "cuda", ldc=4, zero=True)
    fl = torch.zeros(G, dtype=torch.int64, device="cuda")
    res = {"volumes": G, "size": S, "regions": R, "channels": C, "iterations": T, "reps": a.reps, "softmax": bool(a.softmax)}
    results = {}
    for route, tiled in (("tiled", 1), ("generic", 0)):
        ops.set_option(OPT_LAME_TILED, tiled)
        for sigma in (1.0, 0.0):
            times = []
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.lame_refine(l0, x, out, work, fl, connectivity=26, weight=1.0, sigma=sigma, iterations=T, softmax=a.softmax)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times.append(e0.elapsed_time(e1) * 1e3 / T)
            key = f"{route}_sigma{int(sigma)}"
            res[key + "_us_per_launch"] = [round(min(times), 1), round(sum(times) / len(times), 1), round(max(times), 1)]
            results[key] = (out.clone(), fl.clone())
    ops.set_option(OPT_LAME_TILED, 1)
    for sigma in ("sigma1", "sigma0"):
        (zt, ft), (zg, fg) = results["tiled_" + sigma], results["generic_" + sigma]
        res["routes_max_abs_diff_" + sigma] = float((zt - zg).abs().max())
        res["flipped_" + sigma] = [ft.tolist(), fg.tolist()]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
