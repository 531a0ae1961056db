"""The launches of ``mmtta_modality_views`` and ``mmtta_modcons_loss_items`` on their own, next to ``mmtta_memo_loss_items`` (V =
4) and ``mmtta_entropy_loss_items`` on logits of the same size, for a kernel trace or event timing:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/modcons_kernels.py --size 128

Default: --volumes x SIZE^3, 4 input channels (bf16 rows of 8 bytes, as the network input of bf16 precision), 3 regions
(fp32 logits in 16-byte rows), bf16 gradients in 8-byte rows, V = 5 leave-one-out views, weight 1, entropy weight 1, detach
on, --reps calls after one warm-up.  The generic route runs on the same logits in rows of 3 floats with fp32 gradients, the
categorical head on the fast route's rows with fp32 gradients.  Prints the event-timed min / mean / max per call of every arm
as one JSON line (the trace names the kernels: modality_views_vec_kernel, modcons_bernoulli_vec_kernel<V, bf16 gradient>,
modcons_bernoulli_kernel, modcons_categorical_kernel, modcons_finish_kernel).
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
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.modcons import keep_masks
    G, S, R, C, V = a.volumes, a.size, 3, 4, a.views
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"volumes": G, "size": S, "regions": R, "channels": C, "views": V, "reps": a.reps}
    # the views of the staged input
    masks = (keep_masks("leave_one_out", C) + [1, 2, 4, 8])[:V]
    for dt, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        x = ops.new_cl(G, S, S, S, C, "cuda", ldc=4, zero=True, dtype=dt)
        x.copy_(torch.randn((G, S, S, S, C), device="cuda", generator=gen).to(dt))
        y = ops.new_cl(G * V, S, S, S, C, "cuda", ldc=4, zero=True, dtype=dt)
        res[f"modality_views_{name}_us"] = timed(lambda: ops.modality_views(x, y, masks), a.reps)
        del x, y
    # the objective
    z = ops.new_cl(G * V, S, S, S, R, "cuda", ldc=4, zero=True)
    z.copy_(torch.randn((G * V, S, S, S, R), device="cuda", generator=gen) * 3.0)
    out = dict(loss=torch.zeros(G, device="cuda"), entropy=torch.zeros(G, device="cuda"), consistency=torch.zeros(G, device="cuda"),
               view_kl=torch.zeros(G * (V - 1), device="cuda"), disagree=torch.zeros(G * (V - 1), dtype=torch.int64, device="cuda"))
    partial = torch.zeros(ops.modcons_partials(z, V), dtype=torch.float64, device="cuda")

    def modcons(zz, gg, softmax=False):
        ops.modcons_loss_items(zz, gg, V, partial, out["loss"], out["entropy"], out["consistency"], out["view_kl"], out["disagree"],
                               softmax=softmax)

    g16 = ops.new_cl(G * V, S, S, S, R, "cuda", ldc=4, zero=True, dtype=torch.bfloat16)
    g32 = ops.new_cl(G * V, S, S, S, R, "cuda", ldc=4, zero=True)
    res["modcons_fast_bf16_us"] = timed(lambda: modcons(z, g16), a.reps)
    fast = {k: t.clone() for k, t in out.items()}
    res["modcons_fast_fp32_us"] = timed(lambda: modcons(z, g32), a.reps)
    res["modcons_categorical_us"] = timed(lambda: modcons(z, g32, softmax=True), a.reps)
    thin_z = z.contiguous()                      # rows of 3 floats: the generic route
    thin_g = torch.zeros_like(thin_z)
    res["modcons_generic_us"] = timed(lambda: modcons(thin_z, thin_g), a.reps)
    res["routes_max_rel_diff"] = max(float(((out[k] - fast[k]).abs() / fast[k].abs()).max()) for k in ("loss", "entropy", "view_kl"))
    res["routes_disagree_equal"] = bool(torch.equal(out["disagree"], fast["disagree"]))
    del thin_z, thin_g, g32
    # MEMO's pass at V = 4 and Tent's at V = 1 on the same rows
    zm, gm, ge = z[:G * 4], g16[:G * 4], g16[:G]
    gm._mmtta_owns_pad = ge._mmtta_owns_pad = True          # (leading items of a buffer that owns its pad lanes)
    mpart = torch.zeros(ops.memo_partials(zm, 4), dtype=torch.float64, device="cuda")
    res["memo_loss_items_v4_bf16_us"] = timed(lambda: ops.memo_loss_items(zm, gm, view_masks(["h", "w"]), mpart, out["loss"]),
                                              a.reps)
    ze = z[:G]
    epart = torch.zeros(ops.entropy_partials_items(ze), dtype=torch.float64, device="cuda")
    res["entropy_loss_items_bf16_us"] = timed(lambda: ops.entropy_loss_items(ze, ge, epart, out["loss"]), a.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
