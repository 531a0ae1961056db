"""Partial rows of the two-stage channel reductions (tests/golden/norm_reduce_rows.npz, checked by
tests/test_hip_norm_reduce_stream.py).

``mmtta_channel_stats`` (sum x, sum x^2) and ``mmtta_norm_bwd_reduce`` (sum dz, sum dz * xhat) write ``part``
[N * rows_per_n][2][C]; the statistics and every norm backward are finished from it, so its bits are the contract of any
re-scheduling of the first stage.  ``compute()`` builds the seeded inputs of every case below on the CPU, runs the library
of the importable package on them and returns the ``part`` arrays by case name.  Needs a GPU.

    python tests/golden/make_norm_reduce_rows.py [--repo ROOT]      # writes tests/golden/norm_reduce_rows.npz

``--repo`` names the checkout whose built library is asked (default: this one).  The committed file was written from the
commit before the streamed form of the reduction (csrc/pointwise.hip: channel_reduce_stream_kernel) existed; regenerate it
only from a commit whose rows are the reference.
"""
import argparse
import os
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "norm_reduce_rows.npz")

# mode: 0 = channel_stats, 1 = norm_bwd_reduce.  x / d: storage of the activation and of the gradient ("f" fp32, "b" bf16).
# act: "relu", "none" or "leaky" (slope 0.01).  affine: "none", "shared" ([C] gamma / beta) or "item" ([N*C], per_item).
# layout: "pad" rows padded as the engine allocates them (ops.row_pad); "tight" rows of exactly C elements;
#         "wstride" every second voxel along W of a tensor twice as wide (still voxel-dense: a longer voxel stride);
#         "wslice" W voxels out of the middle of a wider tensor (not voxel-dense).
Case = namedtuple("Case", "name mode n c dhw x d act affine layout")
SMALL, BIG, CUBE = (5, 6, 7), (33, 32, 32), (8, 8, 8)


def cases():
    out = []
    for c in (8, 12, 32, 64, 256):      # cpl = 2 / 4 (one idle channel lane) / 8 / 16 / 64; 7 rows, the last of 18 voxels
        out.append(Case(f"bwd_c{c}_small_bb", 1, 1, c, SMALL, "b", "b", "relu", "none", "pad"))
        out.append(Case(f"stats_c{c}_small_b", 0, 1, c, SMALL, "b", "-", "none", "none", "pad"))
    for x, d in (("f", "f"), ("b", "f")):
        out.append(Case(f"bwd_c32_small_{x}{d}", 1, 1, 32, SMALL, x, d, "relu", "shared", "pad"))
    out.append(Case("stats_c32_small_f", 0, 1, 32, SMALL, "f", "-", "none", "none", "pad"))
    # a bf16-stored gradient next to an fp32-stored activation: the thin tensors only (C <= 4)
    out.append(Case("bwd_c4_small_fb", 1, 1, 4, SMALL, "f", "b", "relu", "none", "pad"))
    out.append(Case("bwd_c3_padded_small_fb", 1, 2, 3, SMALL, "f", "b", "relu", "none", "pad"))
    out.append(Case("bwd_c32_n3_item", 1, 3, 32, SMALL, "b", "b", "relu", "item", "pad"))
    out.append(Case("bwd_c32_n3_shared", 1, 3, 32, SMALL, "b", "b", "none", "shared", "pad"))
    out.append(Case("stats_c32_n3", 0, 3, 32, SMALL, "b", "-", "none", "none", "pad"))
    out.append(Case("bwd_c32_small_leaky", 1, 1, 32, SMALL, "b", "b", "leaky", "shared", "pad"))
    out.append(Case("bwd_c32_big_bb", 1, 1, 32, BIG, "b", "b", "relu", "none", "pad"))     # 33 voxels a row, 1024 rows
    out.append(Case("bwd_c32_cube_bb", 1, 1, 32, CUBE, "b", "b", "relu", "none", "pad"))   # 16 full rows, one trip
    out.append(Case("stats_c32_cube_f", 0, 1, 32, CUBE, "f", "-", "none", "none", "pad"))
    # several rows per workgroup (5 x 1023 rows), the last workgroup of an item one row short
    out.append(Case("bwd_c4_rows_fb", 1, 5, 4, (33, 32, 31), "f", "b", "relu", "none", "pad"))
    out.append(Case("stats_c4_rows_f", 0, 5, 4, (33, 32, 31), "f", "-", "none", "none", "pad"))
    # operands of the scalar / irregular kernel
    out.append(Case("bwd_c3_tight_ff", 1, 2, 3, SMALL, "f", "f", "relu", "none", "tight"))
    out.append(Case("stats_c3_tight_f", 0, 2, 3, SMALL, "f", "-", "none", "none", "tight"))
    out.append(Case("bwd_c32_wslice_bb", 1, 1, 32, SMALL, "b", "b", "relu", "none", "wslice"))
    out.append(Case("stats_c32_wslice_b", 0, 1, 32, SMALL, "b", "-", "none", "none", "wslice"))
    out.append(Case("bwd_c32_wstride_bb", 1, 1, 32, SMALL, "b", "b", "relu", "none", "wstride"))
    out.append(Case("stats_c32_wstride_f", 0, 1, 32, SMALL, "f", "-", "none", "none", "wstride"))
    return out


def _device_view(ops, torch, values, storage, layout):
    """[n, d, h, w, c] CPU values (already representable in `storage`) -> the view of a GPU buffer laid out as `layout`."""
    n, d, h, w, c = values.shape
    dtype = torch.bfloat16 if storage == "b" else torch.float32
    ldc = c if layout == "tight" else ops.row_pad(c, dtype)
    if layout == "wstride":
        buf = torch.zeros((n, d, h, 2 * w, ldc), dtype=dtype, device="cuda")
        view = buf[:, :, :, ::2, :c]
    elif layout == "wslice":
        buf = torch.zeros((n, d, h, w + 3, ldc), dtype=dtype, device="cuda")
        view = buf[:, :, :, 2:2 + w, :c]
    else:
        buf = torch.zeros((n, d, h, w, ldc), dtype=dtype, device="cuda")
        view = buf[..., :c]
    view.copy_(values.to(dtype))
    return view


def inputs(case, index):
    """The CPU tensors of a case: seeded, so that every library sees the same bits."""
    import torch

    gen = torch.Generator().manual_seed(1000 + index)
    n, c, (d, h, w) = case.n, case.c, case.dhw

    def stored(t, storage):
        return t.to(torch.bfloat16).float() if storage == "b" else t

    r = {"x": stored(torch.randn((n, d, h, w, c), generator=gen) * 1.7 + 0.3, case.x)}
    if case.mode == 1:
        r["d"] = stored(torch.randn((n, d, h, w, c), generator=gen), case.d)
        r["mean"] = torch.randn(n * c, generator=gen) * 0.3 + 0.3
        r["rstd"] = torch.rand(n * c, generator=gen) + 0.5
        m = {"none": 0, "shared": c, "item": n * c}[case.affine]
        r["gamma"] = torch.rand(m, generator=gen) + 0.5 if m else None
        r["beta"] = torch.randn(m, generator=gen) * 0.1 if m else None
    return r


def run_case(case, index):
    """`part` [N * rows][2][C] of one case, as a CPU tensor."""
    import torch

    from multimodal_tta_amd import ops

    t = inputs(case, index)
    x = _device_view(ops, torch, t["x"], case.x, case.layout)
    rows = ops.reduce_rows_per_n(x)
    part = torch.full((case.n * rows, 2, case.c), float("nan"), device="cuda")
    if case.mode == 0:
        ops.channel_stats(x, part)
    else:
        dout = _device_view(ops, torch, t["d"], case.d, case.layout)
        gamma = t["gamma"].cuda() if t["gamma"] is not None else None
        beta = t["beta"].cuda() if t["beta"] is not None else None
        act = {"relu": ops.ACT_RELU, "none": ops.ACT_NONE, "leaky": ops.ACT_LEAKY_RELU}[case.act]
        nl = ops.NL(t["mean"].cuda(), t["rstd"].cuda(), gamma, beta, per_item=case.affine == "item", act=act,
                    negative_slope=0.01 if case.act == "leaky" else 0.0)
        ops.norm_bwd_reduce(dout, x, nl, part)
    torch.cuda.synchronize()
    return part.cpu()


def compute():
    return {case.name: run_case(case, i).numpy() for i, case in enumerate(cases())}


if __name__ == "__main__":
    import numpy as np

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repo", default=os.path.dirname(TESTS), help="checkout whose built library is asked")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    table = compute()
    np.savez_compressed(args.out, **table)
    import multimodal_tta_amd

    print(f"{args.out}: {len(table)} cases, {sum(v.size for v in table.values())} values, {os.path.getsize(args.out)} bytes, "
          f"from the library of {os.path.dirname(multimodal_tta_amd.__file__)}")
