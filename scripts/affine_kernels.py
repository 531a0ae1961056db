"""The two affine entry points alone, next to the mirror group's ensemble and staging on the same shapes, for a kernel
trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/affine_kernels.py

Default shapes: 2 volumes x 128^3 x 3 regions, V = 4 (fp32 logits): mmtta_memo_ensemble with [0, 2, 1, 3] against
mmtta_affine_ensemble with [0, 2] + 2 affine views; staging: 2 volumes x 4 channels in 8-byte bf16 rows -> 8 items
(mmtta_mirror_views, 4 views) against the 2 x 2 affine items of mmtta_affine_views.  Every kernel is launched --reps times
after one warm-up.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=2)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.affine import AffineSpec, view_matrices
    G, S, R, V = a.volumes, a.size, 3, 4
    spec = AffineSpec(views=2, rotate=(10.0, 10.0, 10.0), scale=0.1, translate=(2.0, 2.0, 2.0))
    m_host, inv_host = (torch.from_numpy(t) for t in view_matrices(spec, list(range(G)), (S, S, S)))
    m, inv = m_host.cuda(), inv_host.cuda()
    z = ops.new_cl(G * V, S, S, S, R, "cuda", ldc=4, zero=True)
    (z if z._base is None else z._base).normal_(0.0, 3.0)
    out = ops.new_cl(G, S, S, S, R, "cuda", ldc=4)
    x = ops.new_cl(G, S, S, S, 4, "cuda", ldc=4, dtype=torch.bfloat16)
    x.normal_()
    xv = ops.new_cl(G * V, S, S, S, 4, "cuda", ldc=4, dtype=torch.bfloat16)
    for rep in range(a.reps + 1):
        ops.memo_ensemble(z, out, [0, 2, 1, 3])
        ops.affine_ensemble(z, out, [0, 2, 0, 0], 2, inv_host, inv)
        ops.mirror_views(x, xv, [0, 2, 1, 3])
        ops.affine_views(x, xv, 2, m_host, m)
        torch.cuda.synchronize()
    print("ensemble checksum", float(out.float().abs().mean()))


if __name__ == "__main__":
    main()
