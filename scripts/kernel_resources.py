"""Per-kernel resource figures of the gfx950 code objects in built objects (no GPU needed).

    python scripts/kernel_resources.py DIR_OR_OBJ... [--json OUT]       # print / save the table
    python scripts/kernel_resources.py --diff OLD.json NEW.json          # figures that changed for kernels in both

Each object's offload bundle is unbundled with clang-offload-bundler and its AMDHSA metadata note read with llvm-readelf.
Figures: VGPR, AGPR, SGPR, LDS (group segment), scratch (private segment) and spill counts, keyed by mangled kernel name.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
KEYS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".group_segment_fixed_size": "lds",
        ".private_segment_fixed_size": "scratch", ".vgpr_spill_count": "vgpr_spill", ".sgpr_spill_count": "sgpr_spill"}


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def figures(obj: str) -> dict:
    """Figures of every gfx950 kernel in an object, or in a linked library (whose fatbin section holds one bundle per object)."""
    notes = ""
    with tempfile.TemporaryDirectory() as td:
        co, fb, one = os.path.join(td, "k.co"), os.path.join(td, "fatbin"), os.path.join(td, "bundle")
        if subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(td, "o")],
                          capture_output=True).returncode != 0:
            return {}                                 # host-only object (no device code)
        blob = open(fb, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)] or [0]
        for a, b in zip(starts, starts[1:] + [len(blob)]):
            with open(one, "wb") as fh:
                fh.write(blob[a:b])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", f"--input={one}",
                            f"--output={co}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
            notes += subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                    text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        if line.startswith("  - "):            # a kernel's record starts (keys of the record sit at column 4)
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    (\.[a-z_]+):\s+(\S+)$", line)
        if cur is None or not m:
            continue
        k, v = m.groups()
        if k in KEYS:
            cur[KEYS[k]] = int(v)
        elif k == ".name":
            out[v] = cur
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--json")
    ap.add_argument("--diff", nargs=2)
    a = ap.parse_args()
    if a.diff:
        old, new = (json.load(open(p)) for p in a.diff)
        common = sorted(set(old) & set(new))
        changed = [k for k in common if old[k] != new[k]]
        for k in changed:
            print(f"{k}\n  old {old[k]}\n  new {new[k]}")
        print(f"{len(common)} kernels in both, {len(changed)} changed; {len(set(old) - set(new))} only in old, "
              f"{len(set(new) - set(old))} only in new")
        return 1 if changed or set(old) - set(new) else 0
    objs = []
    for p in a.paths:
        objs += sorted(glob.glob(os.path.join(p, "*.o"))) if os.path.isdir(p) else [p]
    table = {}
    for o in objs:
        table.update(figures(o))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(table, fh, indent=0, sort_keys=True)
    for k in sorted(table):
        print(k, table[k])
    return 0


if __name__ == "__main__":
    sys.exit(main())
