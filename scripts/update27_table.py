#!/usr/bin/env python
"""Per-layer table of the fused weight-update launches in a rocprofv3 kernel trace (CSV), one row per launch grid.

    python scripts/update27_table.py <dir>/run_kernel_trace.csv [other_trace.csv] > profiles/update27_stream_XXX.md

A grid (cg tiles [+ 1 bias column], cd tiles, sets) names a layer shape: Cg = 8 x cg tiles, Cd = 32 x cd tiles (the U-Net's
channel counts are multiples of 32, and only a convolution's launch carries the bias column, which makes its x odd).
Bytes per launch are the part that needs no plan: sets x weight elements x (12 read + 12 written + two bf16 images); the
slab reads (rn x 27 x CGp x CDp x 4 per set) come on top, so the TB/s column is a lower bound.  With two traces the second
is printed beside the first (before / after)."""
import csv
import sys
from collections import defaultdict


def load(path):
    rows, pre = defaultdict(lambda: [0, 0]), [0, 0]
    for r in csv.DictReader(open(path, newline="")):
        name, ns = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if "wgrad_update27_kernel" in name:
            k = (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))
            rows[k][0] += 1
            rows[k][1] += ns
        elif "slab_prereduce_kernel" in name:
            pre[0] += 1
            pre[1] += ns
    return rows, pre


def main(paths):
    tabs = [load(p) for p in paths]
    for p, (rows, pre) in zip(paths, tabs):
        print(f"`{p}`: {sum(v[0] for v in rows.values())} update launches, {sum(v[1] for v in rows.values()) / 1e6:.3f} ms; "
              f"slab_prereduce {pre[0]} launches, {pre[1] / 1e6:.3f} ms\n")
    two = len(tabs) > 1
    print("| grid (x, y, sets) | Cg x Cd | blocks | launches | us | MB (weights + images) | TB/s (lower bound) |"
          + (" us after | TB/s after | ms saved |" if two else ""))
    print("|---|---|---:|---:|---:|---:|---:|" + ("---:|---:|---:|" if two else ""))
    rows = tabs[0][0]
    for k, (n, ns) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        gx, gy, q = k
        cg, cd = 8 * (gx - gx % 2), 32 * gy
        mb = q * cg * cd * 27 * 28 / 1e6
        us = ns / n / 1e3
        line = f"| {gx}, {gy}, {q} | {cg} x {cd} | {gx * gy * q} | {n} | {us:.1f} | {mb:.1f} | {mb / us:.2f} |"
        if two:
            n2, ns2 = tabs[1][0].get(k, (0, 0))
            us2 = ns2 / n2 / 1e3 if n2 else float("nan")
            line += f" {us2:.1f} | {mb / us2:.2f} | {(ns - ns2) / 1e6:.2f} |"
        print(line)


if __name__ == "__main__":
    main(sys.argv[1:])
