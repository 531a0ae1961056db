"""The four launches of ``mmtta_nuclear_entropy_items`` on their own, next to ``mmtta_entropy_loss_items`` on the same logits,
for a kernel trace or event timing:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/nuclear_kernels.py --size 128

Default: --volumes x SIZE^3 x 3 regions (fp32 logits in 16-byte rows), bf16 gradients in 8-byte rows, weight 1, entropy weight
1, eps 1e-4, the whole-volume box and boxes of [16,16,16], [8,8,8] and [4,4,4], --reps calls after one warm-up.  The generic
route runs on the same values with fp32 gradients and rows of 3 floats (which the fast route cannot take).  Prints the
event-timed min / mean / max per call of every arm as one JSON line (the trace names the kernels: nuc_gram_fast_kernel<softmax>,
nuc_gram_generic_kernel<softmax>, nuc_spectrum_kernel<softmax>, nuc_grad_kernel<softmax, fast, bf16 gradient>,
nuc_finish_kernel).
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
    G, S, R = a.volumes, a.size, 3
    gdt = torch.float32 if a.softmax else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)
    l = ops.new_cl(G, S, S, S, R, "cuda", ldc=4, zero=True)
    l.copy_(torch.randn((G, S, S, S, R), device="cuda", generator=gen) * 3.0)
    dl = ops.new_cl(G, S, S, S, R, "cuda", ldc=4, zero=True, dtype=gdt)
    thin_l = l.contiguous()                      # rows of 3 floats: the generic route
    thin_dl = torch.zeros_like(thin_l)
    epart = torch.zeros(ops.entropy_partials_items(l), dtype=torch.float64, device="cuda")
    s = [torch.zeros(G, device="cuda") for _ in range(3)]
    res = {"volumes": G, "size": S, "regions": R, "reps": a.reps, "softmax": bool(a.softmax)}
    res["entropy_loss_items_us"] = timed(lambda: ops.entropy_loss_items(l, dl, epart, s[0], softmax=a.softmax), a.reps)
    sums = {}
    for route, (zl, zd) in (("fast", (l, dl)), ("generic", (thin_l, thin_dl))):
        for block in ([0, 0, 0], [16, 16, 16], [8, 8, 8], [4, 4, 4]):
            key = f"{route}_block{block[0]}"
            scratch = torch.zeros(ops.nuclear_scratch(zl, block, a.softmax), dtype=torch.float64, device="cuda")
            res[key + "_us"] = timed(lambda: ops.nuclear_entropy_items(zl, zd, scratch, *s, block=block, weight=1.0,
                                                                       softmax=a.softmax), a.reps)
            sums[key] = [t.clone() for t in s]
    for block in (0, 16, 8, 4):
        t, g = sums[f"fast_block{block}"], sums[f"generic_block{block}"]
        res[f"routes_max_rel_diff_block{block}"] = max(float(((a_ - b_).abs() / b_.abs()).max()) for a_, b_ in zip(t, g))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
