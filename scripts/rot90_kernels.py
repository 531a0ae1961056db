"""The loss, ensemble and staging kernels with the mirror group's codes [0, 2, 1, 3] and the rotation group's [0, 18, 3, 17]
on one set of shapes, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/rot90_kernels.py

Default shapes: 8 volumes x 128^3 x 3 regions, V = 4 (fp32 logits, bf16-stored gradients: what the bf16 precision runs);
staging: 2 volumes x 4 channels in 8-byte bf16 rows -> 8 items.  Every kernel is launched --reps times after one warm-up.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIRROR, ROT = [0, 2, 1, 3], [0, 18, 3, 17]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.intensity import parse_intensity, view_parameters
    G, S, R, V = a.volumes, a.size, 3, 4
    z = ops.new_cl(G * V, S, S, S, R, "cuda", ldc=4, zero=True)
    (z if z._base is None else z._base).normal_(0.0, 3.0)
    g = ops.new_cl(G * V, S, S, S, R, "cuda", ldc=4, dtype=torch.bfloat16)
    out = ops.new_cl(G, S, S, S, R, "cuda", ldc=4)
    partial = torch.empty(ops.memo_partials(z, V), dtype=torch.float64, device="cuda")
    loss = torch.empty(G, device="cuda")
    x = ops.new_cl(2, S, S, S, 4, "cuda", ldc=4, dtype=torch.bfloat16)
    x.normal_()
    xv = ops.new_cl(2 * V, S, S, S, 4, "cuda", ldc=4, dtype=torch.bfloat16)
    spec = parse_intensity({"copies": 4, "scale": 0.1, "shift": 0.1, "gamma": 0.3, "noise_std": 0.05}, [])
    table_host = torch.from_numpy(view_parameters(spec, [0, 1], 4))
    table = table_host.cuda()
    rng = torch.empty(2 * 4 * 2, device="cuda")
    rpart = torch.empty(ops.intensity_range_partials(x), device="cuda")
    ops.intensity_range(x, rpart, rng)
    ords = torch.from_numpy(np.array([0, 1], dtype=np.int32)).cuda()
    for rep in range(a.reps + 1):
        for codes in (MIRROR, ROT):
            ops.memo_loss_items(z, g, codes, partial, loss)
            ops.memo_ensemble(z, out, codes)
            ops.mirror_views(x, xv, codes)
            ops.augment_views(x, xv, codes, table_host, table, rng, 0, ords)
        torch.cuda.synchronize()
    print("losses", loss.cpu().tolist())


if __name__ == "__main__":
    main()
