#!/usr/bin/env python
"""Per-instantiation table of the two-stage channel reductions in rocprofv3 kernel traces (CSV).

    python scripts/norm_reduce_table.py <dir>/run_kernel_trace.csv [more traces ...]

One row per kernel instantiation whose name contains channel_reduce (both forms), and norm_bwd_apply8_kernel beside them as
the yardstick: launches, total ms, average microseconds.  A launch's grid does not name its tensor, so the bytes - and the
TB/s - of a shape come from timing that shape alone (profiles/norm_reduce_stream_*.md say how)."""
import csv
import sys
from collections import defaultdict


def load(path):
    rows = defaultdict(lambda: [0, 0])
    for r in csv.DictReader(open(path, newline="")):
        name = r["Kernel_Name"]
        if "channel_reduce" in name or "norm_bwd_apply8_kernel" in name:
            name = name.replace("void mmtta::", "").split("(")[0]
            rows[name][0] += 1
            rows[name][1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    return rows


def main(paths):
    for p in paths:
        rows = load(p)
        red = sum(v[1] for k, v in rows.items() if "channel_reduce" in k)
        print(f"`{p}`: reduce kernels {sum(v[0] for k, v in rows.items() if 'channel_reduce' in k)} launches, {red / 1e6:.3f} ms\n")
        print("| kernel | launches | total ms | avg us |")
        print("|---|---:|---:|---:|")
        for k, (n, ns) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
            print(f"| `{k}` | {n} | {ns / 1e6:.3f} | {ns / n / 1e3:.1f} |")
        print()


if __name__ == "__main__":
    main(sys.argv[1:])
