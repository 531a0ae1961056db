"""The two launches of ``mmtta_crf_entropy_items`` on their own, next to ``mmtta_entropy_loss_items`` on the same logits, for a
kernel trace or event timing:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/crf_kernels.py --size 128

Default: --volumes x SIZE^3 x 3 regions (fp32 logits in 16-byte rows), bf16 gradients in 8-byte rows, 4 input channels in 8-byte
bf16 rows (what bf16 precision stages), connectivity 26, weight 1, sigma 1 and sigma 0, Potts and quadratic, --reps calls after
one warm-up.  The generic route runs on the same values with fp32 gradients and rows of 3 floats (which the tiled route cannot
take).  Prints the event-timed min / mean / max per call of every arm as one JSON line (the trace names the kernels:
crf_tiled_kernel<affinity, softmax, bf16 input, bf16 gradient, form>, crf_generic_kernel, crf_finish_kernel).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    times = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            times.append(e0.elapsed_time(e1) * 1e3)
    return [round(min(times), 1), round(sum(times) / len(times), 1), round(max(times), 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=1)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--softmax", action="store_true")
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    G, S, R, C = a.volumes, a.size, 3, 4
    gdt = torch.float32 if a.softmax else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)
    l = ops.new_cl(G, S, S, S, R, "cuda", ldc=4, zero=True)
    l.copy_(torch.randn((G, S, S, S, R), device="cuda", generator=gen) * 3.0)
    x = ops.new_cl(G, S, S, S, C, "cuda", ldc=4, dtype=torch.bfloat16)
    x.copy_(torch.randn((G, S, S, S, C), device="cuda", generator=gen).to(torch.bfloat16))
    dl = ops.new_cl(G, S, S, S, R, "cuda", ldc=4, zero=True, dtype=gdt)
    thin_l = l.contiguous()                      # rows of 3 floats: the generic route
    thin_dl = torch.zeros_like(thin_l)
    part = torch.zeros(ops.crf_partials(l), dtype=torch.float64, device="cuda")
    epart = torch.zeros(ops.entropy_partials_items(l), dtype=torch.float64, device="cuda")
    s = [torch.zeros(G, device="cuda") for _ in range(3)]
    res = {"volumes": G, "size": S, "regions": R, "channels": C, "reps": a.reps, "softmax": bool(a.softmax)}
    res["entropy_loss_items_us"] = timed(lambda: ops.entropy_loss_items(l, dl, epart, s[0], softmax=a.softmax), a.reps)
    sums = {}
    for route, (zl, zd) in (("tiled", (l, dl)), ("generic", (thin_l, thin_dl))):
        for form in ops.CRF_FORMS:
            for sigma in (1.0, 0.0):
                key = f"{route}_{form}_sigma{int(sigma)}"
                res[key + "_us"] = timed(lambda: ops.crf_entropy_items(zl, x, zd, part, *s, connectivity=26, weight=1.0,
                                                                       sigma=sigma, form=form, softmax=a.softmax), a.reps)
                sums[key] = [t.clone() for t in s]
    for form in ops.CRF_FORMS:
        for sigma in ("sigma1", "sigma0"):
            t, g = sums[f"tiled_{form}_{sigma}"], sums[f"generic_{form}_{sigma}"]
            res[f"routes_max_rel_diff_{form}_{sigma}"] = max(float(((a_ - b_).abs() / b_.abs()).max()) for a_, b_ in zip(t, g))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
