"""Table of forward / input-gradient convolution plans (tests/golden/conv_plans.json, checked by tests/test_conv_plan.py).

``mmtta_conv_plan`` (csrc/conv_igemm.hip::geometry) reads descriptors and options, never tensor memory, so it can be asked
about any shape at any address without a GPU.  ``compute()`` asks it about every layer of ``make_wgrad_plans.layers()`` in
both orientations - forward, and input gradient with x / y swapped - under every combination of the axes in ``AXES`` and
records, per entry, the status code and the seven fields of mmtta_conv_plan_t.

    python tests/golden/make_conv_plans.py [--repo ROOT]      # writes tests/golden/conv_plans.json

``--repo`` names the checkout whose library is asked (default: this one).  The committed table was written from the commit
before the planner was split from the launch code; regenerate it only from a commit whose plans are the reference.

File format: ``layers`` (cin, cout, k, stride, transposed, [n, d, h, w]) without duplicates; ``results`` the distinct
[status, tiles, launches, ksplit, stats_rows, config, _pad, workspace bytes]; ``rows`` the distinct sequences of results over
the combinations in the order of ``combos()`` (the axes that matter to the fewest layers innermost), run-length encoded as
[result index, count, result index, count, ...]; ``table[2 * i + o]`` the row of layer i in orientation o (0 forward, 1 input
gradient); ``errors`` the argument errors by status code.
"""
import argparse
import ctypes as C
import importlib.util
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "conv_plans.json")

F32, BF16 = 0, 1          # include/mmtta.h dtype codes (checked against _lib in compute())
# every axis of the cross product, in the order the table stores it; the first four describe one call, the rest are
# process-wide options
AXES = {
    "dtype": (F32, BF16),                                 # desc.dtype
    "storage": ((F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)),      # (x, y) of the call
    "base_offset": (0, 4, 8),                             # bytes past a 64-byte boundary, both tensors
    "row_pad": (0, 1),                                    # 1: a voxel row one element longer, so no multiple of 4
    "volumes_in_flight": (1, 4, 24),                      # ops.tune_for_volumes_in_flight (the split-K knobs)
    "opt12": (0, 1, 128),                                 # MMTTA_OPT_CLASS_FUSED_MIN_WORKGROUPS (set after the tuning)
    "opt10": (0, 1),                                      # MMTTA_OPT_IGEMM_LEAN
    "opt9": (0, 1),                                       # MMTTA_OPT_EPILOGUE_VEC16
    "opt13": (0, 1, 2, 3),                                # MMTTA_OPT_THIN_MFMA
}
OPTION_KEYS = (9, 10, 12, 13)


def _wgrad_generator():
    spec = importlib.util.spec_from_file_location("make_wgrad_plans", os.path.join(HERE, "make_wgrad_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


WG = _wgrad_generator()
layers, tensor, out_dhw, rle, unrle = WG.layers, WG.tensor, WG.out_dhw, WG.rle, WG.unrle


def combos():
    return list(itertools.product(*AXES.values()))


def error_cases(_lib):
    """(name, desc, x, y): one argument error each."""
    D, T = _lib.ConvDesc, _lib.Tensor
    fwd, dgrad_t = _lib.CONV_FWD, _lib.CONVT_DGRAD

    def t(base, c, dhw, n=1):
        return tensor(_lib, base, n, c, dhw, F32, 0, 0)

    X, Y, e8 = 1 << 30, 1 << 32, (8, 8, 8)
    planar = T(X, 1, 32, 8, 8, 8, 32 * 512, 512, 64, 8, 1, F32, 0)        # NCDHW: sc != 1
    return [
        ("bad op", D(4, 3, 1, 32, 32, F32), t(X, 32, e8), t(Y, 32, e8)),
        ("ksize 5", D(fwd, 5, 1, 32, 32, F32), t(X, 32, e8), t(Y, 32, e8)),
        ("stride 3", D(fwd, 3, 3, 32, 32, F32), t(X, 32, (9, 9, 9)), t(Y, 32, (3, 3, 3))),
        ("1x1x1 with stride 2", D(fwd, 1, 2, 32, 32, F32), t(X, 32, e8), t(Y, 32, (4, 4, 4))),
        ("channel mismatch", D(fwd, 3, 1, 32, 32, F32), t(X, 16, e8), t(Y, 32, e8)),
        ("batch mismatch", D(fwd, 3, 1, 32, 32, F32), t(X, 32, e8, 2), t(Y, 32, e8, 1)),
        ("spatial mismatch", D(fwd, 3, 2, 32, 32, F32), t(X, 32, e8), t(Y, 32, e8)),
        ("odd extent for the transposed input gradient", D(dgrad_t, 3, 2, 32, 32, F32), t(X, 32, (8, 9, 8)), t(Y, 32, (4, 4, 4))),
        ("non-channels-last", D(fwd, 3, 1, 32, 32, F32), planar, t(Y, 32, e8)),
    ]


def options(ops):
    """The options this table varies, as they are now (mmtta_set_option returns the previous value)."""
    now = {}
    for key in list(ops.TUNE_AT_4) + list(OPTION_KEYS):
        now[key] = ops.set_option(key, 1)
        ops.set_option(key, now[key])
    return now


def compute():
    """{"layers", "results", "rows", "table", "errors"} from the library of the importable multimodal_tta_amd; options and tuning are
    left as they were found."""
    from multimodal_tta_amd import _lib, ops

    assert (_lib.F32, _lib.BF16) == (F32, BF16)
    lib, plan = _lib.load(), _lib.ConvPlan()
    pref = C.byref(plan)

    def ask(d, x, y):
        st = int(lib.mmtta_conv_plan(d, x, y, pref))
        if st:
            return (st, 0, 0, 0, 0, 0, 0, 0)
        return (0, plan.tiles, plan.launches, plan.ksplit, plan.stats_rows, plan.config, plan._pad, plan.workspace_bytes)

    lay = layers()
    ax = AXES
    per_call = list(itertools.product(ax["dtype"], ax["storage"], ax["base_offset"], ax["row_pad"]))
    keep, calls = [], []            # per (layer, orientation): [(desc, x, y)] in per_call order, as ctypes references
    for cin, cout, k, stride, transposed, (n, *dhw) in lay:
        fo, do = (_lib.CONVT_FWD, _lib.CONVT_DGRAD) if transposed else (_lib.CONV_FWD, _lib.CONV_DGRAD)
        for op in (fo, do):
            row = []
            for dtype, (sx, sy), off, pad in per_call:
                lo = tensor(_lib, 1 << 30, n, cin, dhw, sx if op == fo else sy, off, pad)
                hi = tensor(_lib, 1 << 40, n, cout, out_dhw(dhw, stride, transposed), sy if op == fo else sx, off, pad)
                x, y = (lo, hi) if op == fo else (hi, lo)
                dsc = _lib.ConvDesc(op, k, stride, cin, cout, dtype)
                keep.append((dsc, x, y))
                row.append((C.byref(dsc), C.byref(x), C.byref(y)))
            calls.append(row)
    per_opt = list(itertools.product(ax["volumes_in_flight"], ax["opt12"], ax["opt10"], ax["opt9"], ax["opt13"]))
    index, flat = {}, [[0] * (len(per_call) * len(per_opt)) for _ in calls]
    tuned_for, saved = ops._TUNED_FOR, options(ops)
    try:
        for j, (volumes, o12, o10, o9, o13) in enumerate(per_opt):      # options outside: one setting, every call
            for key, val in ops.tune_for_volumes_in_flight(volumes).items():
                ops.set_option(key, val)            # (whether or not the call above did: MMTTA_NO_AUTOTUNE, already tuned)
            for key, val in ((12, o12), (10, o10), (9, o9), (13, o13)):
                ops.set_option(key, val)
            for i, row in enumerate(calls):
                out = flat[i]
                for k, (d, x, y) in enumerate(row):
                    r = ask(d, x, y)
                    out[k * len(per_opt) + j] = index.setdefault(r, len(index))
        errors = []
        for name, d, x, y in error_cases(_lib):
            errors.append({"name": name, "status": ask(C.byref(d), C.byref(x), C.byref(y))[0]})
    finally:
        for key, val in saved.items():
            ops.set_option(key, val)
        ops._TUNED_FOR = tuned_for
    results = [list(r) for r in index]          # insertion order = index
    rows = {}
    table = [rows.setdefault(tuple(rle(f)), len(rows)) for f in flat]
    return {"layers": [list(c[:5]) + [list(c[5])] for c in lay], "results": results, "rows": [list(r) for r in rows], "table": table,
            "errors": errors}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repo", default=os.path.dirname(TESTS), help="checkout whose built library is asked")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    table = compute()
    with open(args.out, "w") as fh:
        json.dump(table, fh, separators=(",", ":"))
        fh.write("\n")
    cfgs = sorted({r[5] for r in table["results"] if r[0] == 0})
    print(f"{args.out}: {len(table['layers'])} layers x 2 orientations x {len(combos())} combinations, {len(table['results'])} "
          f"distinct results, configs {cfgs}, {os.path.getsize(args.out)} bytes")
