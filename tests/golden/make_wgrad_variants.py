"""Table of weight-gradient decisions (tests/golden/wgrad_variants.json, checked by tests/test_wgrad_variant_table.py).

The planner of the weight gradient (csrc/conv_wgrad.hip: wgeometry, then plan_wgrad for the variant of the route) reads
descriptors and options, never tensor memory, so it can be asked about any call at any address without a GPU.  ``compute()``
asks it about every layer of make_wgrad_plans.py ``layers()`` under the combinations of ``combos()`` and records per entry
the answer of mmtta_conv_wgrad_kernel (the route, or its negative status), the status and the four integers of
mmtta_conv_wgrad_plan_sets, mmtta_conv_wgrad_workspace_bytes_sets, mmtta_conv_wgrad_stages_raw and
mmtta_conv_wgrad_updates_in_epilogue.

    python tests/golden/make_wgrad_variants.py [--repo ROOT]      # writes tests/golden/wgrad_variants.json

``--repo`` names the checkout whose library is asked (default: this one).  The committed table was written from the commit
before the variant of a route moved into the weight gradient's plan; regenerate it only from a commit whose decisions are
the reference.  MMTTA_WGRAD_PAIR and MMTTA_FUSED_UPDATE are read from the environment when the library is loaded: the table
records their defaults only (neither variable set).

wgrad_plans.json crosses the volumes in flight, options 11 and 13, desc.dtype, the storage pairs, sets of one item, base
offsets and row pads.  This table adds what the variant reads - option 16, option 19, the norm-on-load of x, sets of two
items - and keeps every axis only where the planner can read it, by precision and class of layer:

  every layer      the volumes-in-flight tuning (slab counts), the four storage pairs, the parameter sets (none, one item,
                   two items per set: tiles and slabs are per set; a batch of one refuses sets of two), base offsets and row
                   pads (every alignment test).
  fp32 precision   nothing else: options 11, 13, 16 and 19 and the norm-on-load gate kernels of bf16 precision only.
  bf16 precision   option 11 (the transposed-read kernels: wtr_ok / q_ok and MMTTA_OPT_WGRAD_VECTOR_STAGING) on every layer;
    thin           (<= 4 channels on a side) option 13, which picks between the tiny, the small and the thin transposed-read
                   kernel; no variant: raw staging and the update in the epilogue exist on routes 7 and 8 alone.
    stride2        (27 taps at stride 2, Conv3d and ConvTranspose3d, more than 4 channels a side: route 8) option 16
                   (wgrad_raw_bits) and the norm-on-load (its identity test; LeakyReLU runs the instantiation without raw
                   kernels).
    stride1        (27 taps at stride 1, more than 4 channels a side: route 7) option 19 (wgrad_updates_in_epilogue) and the
                   norm-on-load (LeakyReLU again).
    one_tap        (1x1x1, more than 4 channels a side) nothing else.
  An option a class does not vary stays at the default of csrc/api.hip.

File format: ``layers`` (cin, cout, k, stride, transposed, [n, d, h, w]); ``results`` the distinct [kernel, plan status, nsl,
pre_chunks, CGp, CDp, workspace bytes, stages_raw, updates_in_epilogue]; ``rows`` the distinct rows - the results of one
section's calls (``call_axes`` order) under one combination of options - run-length encoded as [index, count, ...];
``table[i]`` = the sections of layer i in ``SECTIONS`` order (desc.dtype), each the rows over ``option_combos(layer, dtype)``,
run-length encoded as [row index, count, ...].  A row many option combinations and layers share is stored once.
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
OUT = os.path.join(HERE, "wgrad_variants.json")

F32, BF16 = 0, 1          # include/mmtta.h dtype codes (checked against _lib in compute())
P = 1 << 21               # a made-up address for the pointers nothing reads (norm parameters)
FIELDS = ("kernel", "plan status", "nsl", "pre_chunks", "CGp", "CDp", "workspace bytes", "stages_raw", "updates_in_epilogue")

# ---- the axes of one call
CALL_AXES = {
    "storage": ((F32, F32), (BF16, F32), (BF16, BF16), (F32, BF16)),      # (x, dy); the last is the pair the planner refuses for bf16 kernels
    "sets": (0, 1, 2),                                    # no parameter sets / sets of one item / of two items
    "base_offset": (0, 4, 8),                             # bytes past a 64-byte boundary, both tensors
    "row_pad": (0, 1),                                    # 1: a voxel row one element longer, so no multiple of 4
    "x_norm": ("none", "null", "mean_rstd", "scale_shift", "relu", "leaky"),
}
# ---- process-wide options, by precision and class of layer (docstring); the order is the order of the loops
OPTION_AXES = {
    "volumes_in_flight": (1, 4, 24),      # ops.tune_for_volumes_in_flight
    11: (0, 1), 13: (0, 1, 2, 3), 16: (0, 1, 2, 3), 19: (0, 1),
}
CLASS_OPTIONS = {
    "fp32": ("volumes_in_flight",),
    "thin": ("volumes_in_flight", 11, 13),
    "stride2": ("volumes_in_flight", 11, 16),
    "stride1": ("volumes_in_flight", 11, 19),
    "one_tap": ("volumes_in_flight", 11),
}
SECTIONS = (F32, BF16)


def _wgrad_plans():
    spec = importlib.util.spec_from_file_location("make_wgrad_plans", os.path.join(HERE, "make_wgrad_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


wp = _wgrad_plans()
layers, rle, unrle = wp.layers, wp.rle, wp.unrle


def layer_class(layer, dtype):
    cin, cout, k, stride, transposed, _ = layer
    if dtype == F32:
        return "fp32"
    if min(cin, cout) <= 4:
        return "thin"
    if k == 1:
        return "one_tap"
    return "stride2" if (stride == 2 or transposed) else "stride1"


def call_axes(layer, dtype):
    """{axis: values} of the per-call axes this section varies, in CALL_AXES order."""
    ax = dict(CALL_AXES)
    if layer_class(layer, dtype) not in ("stride1", "stride2"):
        ax["x_norm"] = ("none",)
    return ax


def option_combos(layer, dtype):
    """[{option: value}] of a section, in table order."""
    keys = CLASS_OPTIONS[layer_class(layer, dtype)]
    return [dict(zip(keys, combo)) for combo in itertools.product(*[OPTION_AXES[k] for k in keys])]


def combos(layer, dtype):
    """Every combination of a section's entries, options outermost: [({option: value}, {axis: value})] in table order."""
    ca = call_axes(layer, dtype)
    return [(o, dict(zip(ca, c))) for o in option_combos(layer, dtype) for c in itertools.product(*ca.values())]


def x_norm(_lib, kind):
    if kind == "none":
        return None
    return {"null": lambda: _lib.norm_on_load(),
            "mean_rstd": lambda: _lib.NormOnLoadAct(P, P, None, None, _lib.ACT_NONE, 0, None, None, 0.0, 0),
            "scale_shift": lambda: _lib.NormOnLoadAct(None, None, None, None, _lib.ACT_NONE, 0, P, P, 0.0, 0),
            "relu": lambda: _lib.norm_on_load(relu=True),
            "leaky": lambda: _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=0.1)}[kind]()


class Calls:
    """The ctypes arguments of a section's calls, built once: the same objects serve every option combination."""

    def __init__(self, _lib, layer, dtype):
        self.lib = _lib.load()
        cin, cout, k, stride, transposed, (n, *dhw) = layer
        self.plan = (C.c_int32 * 4)()
        self.sets = {0: None, 1: _lib.ParamSets(1, 1, 0, 0, 0, 0, 0, 0), 2: _lib.ParamSets(2, 1, 0, 0, 0, 0, 0, 0)}
        self.keep, self.calls = [], []
        ax = call_axes(layer, dtype)
        r = lambda o: None if o is None else C.byref(o)
        for combo in itertools.product(*ax.values()):
            a = dict(zip(ax, combo))
            sx, sy = a["storage"]
            desc = _lib.ConvDesc(_lib.CONVT_FWD if transposed else _lib.CONV_FWD, k, stride, cin, cout, dtype)
            x = wp.tensor(_lib, 1 << 30, n, cin, dhw, sx, a["base_offset"], a["row_pad"])
            dy = wp.tensor(_lib, 1 << 40, n, cout, wp.out_dhw(dhw, stride, transposed), sy, a["base_offset"], a["row_pad"])
            xn = x_norm(_lib, a["x_norm"])
            self.keep += [desc, x, dy, xn]
            self.calls.append((r(desc), r(x), r(xn), r(dy), r(self.sets[a["sets"]])))

    def ask(self):
        """One result per call, under the options as they are now."""
        lib, plan = self.lib, self.plan
        out = []
        for d, x, xn, dy, sets in self.calls:
            st = int(lib.mmtta_conv_wgrad_plan_sets(d, x, dy, sets, plan))
            out.append((int(lib.mmtta_conv_wgrad_kernel(d, x, dy)), st, *(plan if st == 0 else (0, 0, 0, 0)),
                        int(lib.mmtta_conv_wgrad_workspace_bytes_sets(d, x, dy, sets)), int(lib.mmtta_conv_wgrad_stages_raw(d, x, xn, dy)),
                        int(lib.mmtta_conv_wgrad_updates_in_epilogue(d, x, xn, dy, sets))))
        return out


def options(ops):
    """The options this table varies, as they are now (mmtta_set_option returns the previous value)."""
    now = {}
    for key in list(ops.TUNE_AT_4) + [k for k in OPTION_AXES if k != "volumes_in_flight"]:
        now[key] = ops.set_option(key, 1)
        ops.set_option(key, now[key])
    return now


def compute():
    """{"layers", "results", "rows", "table"} from the library of the importable multimodal_tta_amd; options and tuning are
    left as they were found."""
    from multimodal_tta_amd import _lib, ops

    assert (_lib.F32, _lib.BF16) == (F32, BF16)
    lay = layers()
    results, rows, table = {}, {}, []
    tuned_for, saved = ops._TUNED_FOR, options(ops)
    tuning = {}
    try:
        for v in OPTION_AXES["volumes_in_flight"]:
            tuning[v] = dict(ops.tune_for_volumes_in_flight(v))
        for layer in lay:
            row = []
            for dtype in SECTIONS:
                calls, flat = Calls(_lib, layer, dtype), []
                for combo in option_combos(layer, dtype):
                    for key, val in combo.items():
                        for k, v in (tuning[val].items() if key == "volumes_in_flight" else ((key, val),)):
                            ops.set_option(k, v)
                    one = tuple(rle([results.setdefault(r, len(results)) for r in calls.ask()]))
                    flat.append(rows.setdefault(one, len(rows)))
                for key, val in saved.items():
                    ops.set_option(key, val)
                row.append(rle(flat))
            table.append(row)
    finally:
        for key, val in saved.items():
            ops.set_option(key, val)
        ops._TUNED_FOR = tuned_for
    return {"layers": [list(c[:5]) + [list(c[5])] for c in lay], "results": [list(r) for r in results],
            "rows": [list(r) for r in rows], "table": table}


def section_results(table, section):
    """The results of a section over ``combos()``: its rows, expanded."""
    return [table["results"][i] for row in unrle(section) for i in unrle(table["rows"][row])]


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
    ok = [r for r in table["results"] if r[0] >= 0]
    entries = sum(len(section_results(table, sec)) for row in table["table"] for sec in row)
    print(f"{args.out}: {len(table['layers'])} layers, {entries} entries, {len(table['results'])} distinct results, "
          f"{len(table['rows'])} distinct rows, kernel ids {sorted({r[0] for r in ok})}, stages_raw {sorted({r[7] for r in ok})}, "
          f"updates_in_epilogue {sorted({r[8] for r in ok})}, {os.path.getsize(args.out)} bytes")
