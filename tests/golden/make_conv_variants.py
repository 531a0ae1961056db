"""Table of forward / input-gradient convolution decisions (tests/golden/conv_variants.json, checked by
tests/test_conv_variant_table.py).

The planner of a convolution run (csrc/conv_igemm.hip: geometry / plan_run) reads descriptors and options, never tensor
memory, so it can be asked about any call at any address without a GPU.  ``compute()`` asks it about every layer below, as a
forward call and as the input gradient, under the combinations of ``combos()``, and records per entry the status and the
bytes of mmtta_conv_plan, the answers of the six run-time queries (mmtta_conv_route, _stages_raw, _cls8_pipelined,
_cls8_lean_epilogue, _thin_lean, _thin_kernel) and mmtta_conv_head_loss_eligible.

    python tests/golden/make_conv_variants.py [--repo ROOT]      # writes tests/golden/conv_variants.json

``--repo`` names the checkout whose library is asked (default: this one).  The committed table was written from the commit
before the variant of a route moved into the run plan; regenerate it only from a commit whose decisions are the reference.

Layers: tests/conv_geometry.py CASES and CLS_FUSED_CASE, the two class-fused layers whose channel counts are no multiple
of 8 (36 produced channels; 40 -> 24), and every convolution of the registered models at 128^3 (make_wgrad_plans.py
model_layers(); batch 1 only: the planner works per item, the batch multiplies the tiles).

The full cross product of the axes is some 10^9 entries, so every axis is kept only where the planner can read it.  What a
layer's descriptor rules out (the functions named are those of csrc/conv_igemm.hip and csrc/conv_direct.hip):

  per call   `accumulate` is read by the thin routes alone (chan_lean_applicable, direct_kernel's head test): it varies
             on thin layers only (<= 4 channels on either side).  `stats` is read by those and by the gates of the 1x1x1
             routes (pointwise_small_applicable, pointwise_mfma_applicable): it varies on thin and on 1x1x1 layers only.
             A base offset and a row pad each break every alignment test the other does: (0, 0), (8, 0), (0, 1); thin
             layers add a pad of 4 elements, which keeps fp32 items and breaks bf16 ones (direct_variant 3 against 5).
  options    fp32 precision (desc.dtype): the volumes-in-flight tuning alone.  Every other option below gates a kernel of
                 bf16 precision (use_bf16 / cfg.bf, direct_variant, chan_lean_applicable, direct_upconv8_lean).
             bf16 precision, by class of layer:
             thin layers: the tuning, 13 and 18 (direct_variant, the lean predicates); no option of the implicit GEMM is
                 read on routes 6 / 13, and their operands are fp32 operands on any other route.
             stride-2 transposed forms (ConvTranspose3d forward, input gradient of a stride-2 Conv3d): the tuning, 12 and 9
                 (the class-fused gate) and 16; 20 where the gate can open (12 below 2^20 - no layer here has that many
                 workgroups - and 9 set) and 16 has bit 0, 21 where 20 is set as well: the pipelined kernel is a raw
                 call of route 15, the lean epilogue a pipelined one.
             3x3x3 stride-1 32 -> 32: the tuning, 6, 9 and 14 (igemm_reuse_applicable) and 16.
             every other layer: the tuning and 16.
  Options a class does not vary stay at the defaults of csrc/api.hip, but option 10 = 0 on the case of
  tests/conv_geometry.py that asks for it (`lean=0`: the 8 x 8 x 8 bf16 tile, route 7).
  Of the tuning only keys 2 - 5 are set: key 12 is an axis of its own.

File format: ``layers`` (cin, cout, k, stride, transposed, [n, d, h, w]) without duplicates; ``plans`` the distinct
[plan status, plan bytes (hex)]; ``decisions`` the distinct [route, stages_raw, cls8_pipelined, cls8_lean_epilogue, thin_lean,
thin_kernel, head_loss_eligible]; ``rows`` the distinct rows - the plans, or the decisions, of one section's calls
(``call_axes`` order) under one combination of options - run-length encoded as [index, count, index, count, ...];
``table[i]`` = the sections of layer i in ``SECTIONS`` order (orientation, desc.dtype), each a pair [plan rows, decision rows]
over ``option_combos(layer, orientation, dtype)``, run-length encoded as [row index, count, ...].  A row many option
combinations and layers share is stored once.
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
OUT = os.path.join(HERE, "conv_variants.json")

F32, BF16 = 0, 1          # include/mmtta.h dtype codes (checked against _lib in compute())
OWNS_PAD = 1              # MMTTA_TENSOR_OWNS_PAD: the <= 4-channel tensors own the pad lanes of their rows, as the models' do
QUERIES = ("mmtta_conv_route", "mmtta_conv_stages_raw", "mmtta_conv_cls8_pipelined", "mmtta_conv_cls8_lean_epilogue",
           "mmtta_conv_thin_lean", "mmtta_conv_thin_kernel")
P = 1 << 21               # a made-up address for the pointers nothing reads (statistics rows, norm parameters)

# ---- the axes of one call
CALL_AXES = {
    "storage": ((F32, F32, F32), (BF16, BF16, BF16), (BF16, F32, F32)),    # (x, y, add); the mixed pair is the thin up-convolution's
    "x_norm": ("none", "null", "mean_rstd", "scale_shift", "relu", "leaky"),
    "add": ("none", "plain", "leaky"),
    "layout": ((0, 0), (8, 0), (0, 1)),                                   # (base offset in bytes, elements of row pad), all tensors
    "stats": (0, 1),
    "accumulate": (0, 1),
}
# ---- process-wide options, by class of layer (docstring); the order is the order of the loops
OPTION_AXES = {
    "volumes_in_flight": (1, 4, 24),      # ops.tune_for_volumes_in_flight, keys 2 - 5
    6: (0, 1), 9: (0, 1), 12: (1, 128, 1 << 20), 13: (0, 2), 14: (0, 1), 16: (0, 1, 2, 3), 18: (0, 1, 2, 3), 20: (0, 1), 21: (0, 1),
}
CLASS_OPTIONS = {
    "fp32": ("volumes_in_flight",),
    "thin": ("volumes_in_flight", 13, 18),
    "classes": ("volumes_in_flight", 12, 9, 16, 20, 21),      # (20 and 21 where they can be read: option_combos)
    "reuse": ("volumes_in_flight", 6, 9, 14, 16),
    "igemm": ("volumes_in_flight", 16),
}
OPTION_KEYS = (2, 3, 4, 5, 10) + tuple(k for k in OPTION_AXES if k != "volumes_in_flight")
SECTIONS = (("fwd", F32), ("fwd", BF16), ("dgrad", F32), ("dgrad", BF16))
THIN_LAYOUTS = CALL_AXES["layout"] + ((0, 4),)
MODEL_BATCH = 1


def _wgrad_generator():
    spec = importlib.util.spec_from_file_location("make_wgrad_plans", os.path.join(HERE, "make_wgrad_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def layers():
    sys.path.insert(0, TESTS)
    try:
        import conv_geometry as cg
    finally:
        sys.path.remove(TESTS)
    out = [(c.cin, c.cout, c.k, c.stride, c.transposed, tuple(c.shape)) for c in list(cg.CASES) + [cg.CLS_FUSED_CASE]]
    # class-fused layers whose rows are groups of 4 channels, not 8 (tests/test_cls8_lean_epilogue_host.py)
    out += [(128, 36, 3, 2, True, (2, 8, 8, 8)), (40, 24, 3, 2, True, (2, 8, 8, 8))]
    for case in _wgrad_generator().model_layers():
        if case[5][0] == MODEL_BATCH:
            out.append(tuple(case[:5]) + (tuple(case[5]),))
    uniq = []
    for case in out:
        if case not in uniq:                # the same layer from two lists is the same input: one entry
            uniq.append(case)
    return uniq


def layer_class(layer, orientation):
    cin, cout, k, stride, transposed, _ = layer
    if min(cin, cout) <= 4:
        return "thin"
    if k == 3 and stride == 2 and (transposed == (orientation == "fwd")):
        return "classes"
    if k == 3 and stride == 1 and cin == 32 and cout == 32:
        return "reuse"
    return "igemm"


def fixed_options(layer):
    """Options a layer runs under throughout: what its case of tests/conv_geometry.py asks for."""
    sys.path.insert(0, TESTS)
    try:
        import conv_geometry as cg
    finally:
        sys.path.remove(TESTS)
    wide = [(c.cin, c.cout, c.k, c.stride, c.transposed, tuple(c.shape)) for c in cg.CASES if not c.lean]
    return {10: 0} if tuple(layer[:5]) + (tuple(layer[5]),) in wide else {}


def call_axes(layer, orientation):
    """{axis: values} of the per-call axes this layer varies, in CALL_AXES order."""
    thin, k = layer_class(layer, orientation) == "thin", layer[2]
    ax = dict(CALL_AXES)
    if thin:
        ax["layout"] = THIN_LAYOUTS
    else:
        ax["accumulate"] = (0,)
        if k != 1:
            ax["stats"] = (0,)
    return ax


def option_combos(layer, orientation, dtype):
    """[{option: value}] of a section, in table order."""
    cls = "fp32" if dtype == F32 else layer_class(layer, orientation)
    keys = CLASS_OPTIONS[cls]
    out = []
    for combo in itertools.product(*[OPTION_AXES[k] for k in keys]):
        o = dict(zip(keys, combo))
        if cls == "classes":
            raw = o[12] < (1 << 20) and o[9] and (o[16] & 1)
            if (o[20] == 0 and not raw) or (o[21] == 0 and not (raw and o[20])):
                continue                    # an option nothing can read stays at its default
        out.append(o)
    return out


def combos(layer, orientation, dtype):
    """Every combination of a section's entries, options outermost: [({option: value}, {axis: value})] in table order."""
    ca = call_axes(layer, orientation)
    return [(o, dict(zip(ca, c))) for o in option_combos(layer, orientation, dtype) for c in itertools.product(*ca.values())]


def out_dhw(dhw, stride, transposed):
    return tuple(2 * v if transposed else (v if stride == 1 else (v + 1) // 2) for v in dhw)


def tensor(_lib, base, n, c, dhw, dtype, layout):
    offset, row_pad = layout
    d, h, w = dhw
    sw = ((c + 3) // 4 * 4 if (dtype == F32 or c <= 4) else (c + 7) // 8 * 8) + row_pad
    return _lib.Tensor(base + offset, n, c, d, h, w, d * h * w * sw, 1, h * w * sw, w * sw, sw, dtype, OWNS_PAD if c <= 4 else 0)


def x_norm(_lib, kind):
    if kind == "none":
        return None
    return {"null": lambda: _lib.norm_on_load(),
            "mean_rstd": lambda: _lib.NormOnLoadAct(P, P, None, None, _lib.ACT_NONE, 0, None, None, 0.0, 0),
            "scale_shift": lambda: _lib.NormOnLoadAct(None, None, None, None, _lib.ACT_NONE, 0, P, P, 0.0, 0),
            "relu": lambda: _lib.norm_on_load(relu=True),
            "leaky": lambda: _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=0.1)}[kind]()


class Calls:
    """The ctypes arguments of a layer's calls, built once: the same objects serve every option combination."""

    def __init__(self, _lib, layer, orientation, dtype):
        self._lib, self.lib = _lib, _lib.load()
        cin, cout, k, stride, transposed, (n, *dhw) = layer
        fo, do = (_lib.CONVT_FWD, _lib.CONVT_DGRAD) if transposed else (_lib.CONV_FWD, _lib.CONV_DGRAD)
        self.keep, self.calls = [], []
        fns = [getattr(self.lib, q) for q in QUERIES]
        ax = call_axes(layer, orientation)
        for combo in itertools.product(*ax.values()):
            a = dict(zip(ax, combo))
            sx, sy, sa = a["storage"]
            lo = (cin, tuple(dhw)), (cout, out_dhw(dhw, stride, transposed))
            (xc, xs), (yc, ys) = lo if orientation == "fwd" else lo[::-1]
            desc = _lib.ConvDesc(fo if orientation == "fwd" else do, k, stride, cin, cout, dtype)
            x = tensor(_lib, 1 << 30, n, xc, xs, sx, a["layout"])
            y = tensor(_lib, 1 << 40, n, yc, ys, sy, a["layout"])
            dz = tensor(_lib, 1 << 42, n, yc, ys, F32, (0, 0))          # the loss gradient of the head pair: dense, owns its pad
            xn = x_norm(_lib, a["x_norm"])
            epi = None
            if a["add"] != "none":
                add = tensor(_lib, 1 << 41, n, yc, ys, sa, a["layout"])
                epi = _lib.ConvEpilogue(C.pointer(add), x_norm(_lib, "leaky" if a["add"] == "leaky" else "null"))
                self.keep.append(add)
            self.keep += [desc, x, y, dz, xn, epi]
            r = lambda o: None if o is None else C.byref(o)
            args = (r(desc), r(x), r(xn), r(epi), r(y), a["accumulate"], P if a["stats"] else None)
            self.calls.append((fns, args, (r(desc), r(x), r(y)), (r(desc), r(x), r(xn), r(epi), r(y), r(dz), 0, 1)))
        self.plan = _lib.ConvPlan()

    def ask(self):
        """One result per call, under the options as they are now."""
        lib, plan, pref = self.lib, self.plan, C.byref(self.plan)
        out = []
        for fns, args, pargs, hargs in self.calls:
            C.memset(pref, 0, C.sizeof(plan))
            st = int(lib.mmtta_conv_plan(*pargs, pref))
            out.append((st, bytes(plan).hex() if st == 0 else "", *[int(fn(*args)) for fn in fns],
                        int(lib.mmtta_conv_head_loss_eligible(*hargs))))
        return out


def options(ops):
    """The options this table varies, as they are now (mmtta_set_option returns the previous value)."""
    now = {}
    for key in OPTION_KEYS:
        now[key] = ops.set_option(key, 1)
        ops.set_option(key, now[key])
    return now


def compute():
    """{"layers", "plans", "decisions", "rows", "table"} from the library of the importable multimodal_tta_amd; options and tuning are left as
    they were found."""
    from multimodal_tta_amd import _lib, ops

    assert (_lib.F32, _lib.BF16, _lib.TENSOR_OWNS_PAD) == (F32, BF16, OWNS_PAD)
    lay = layers()
    plans, decisions, rows, table = {}, {}, {}, []
    tuned_for, saved = ops._TUNED_FOR, options(ops)
    tuning = {}
    try:
        for v in OPTION_AXES["volumes_in_flight"]:
            tuning[v] = {k: val for k, val in ops.tune_for_volumes_in_flight(v).items() if k in (2, 3, 4, 5)}
        for key, val in saved.items():
            ops.set_option(key, val)
        for layer in lay:
            row = []
            for orientation, dtype in SECTIONS:
                calls, flat = Calls(_lib, layer, orientation, dtype), ([], [])
                for key, val in fixed_options(layer).items():
                    ops.set_option(key, val)
                for combo in option_combos(layer, orientation, dtype):
                    for key, val in combo.items():
                        for k, v in (tuning[val].items() if key == "volumes_in_flight" else ((key, val),)):
                            ops.set_option(k, v)
                    got = calls.ask()
                    for part, seen, lo, hi in ((0, plans, 0, 2), (1, decisions, 2, None)):
                        one = tuple(rle([seen.setdefault(r[lo:hi], len(seen)) for r in got]))
                        flat[part].append(rows.setdefault(one, len(rows)))
                for key, val in saved.items():
                    ops.set_option(key, val)
                row.append([rle(flat[0]), rle(flat[1])])
            table.append(row)
    finally:
        for key, val in saved.items():
            ops.set_option(key, val)
        ops._TUNED_FOR = tuned_for
    return {"layers": [list(c[:5]) + [list(c[5])] for c in lay], "plans": [list(r) for r in plans], "decisions": [list(r) for r in decisions],
            "rows": [list(r) for r in rows], "table": table}


def rle(seq):
    out = []
    for v in seq:
        if out and out[-2] == v:
            out[-1] += 1
        else:
            out += [v, 1]
    return out


def unrle(runs):
    return [v for v, cnt in zip(runs[0::2], runs[1::2]) for _ in range(cnt)]


def section_results(table, section):
    """[plan + decision] of a section over ``combos()``: its rows, expanded."""
    plan, dec = ([i for row in unrle(runs) for i in unrle(table["rows"][row])] for runs in section)
    return [table["plans"][p] + table["decisions"][d] for p, d in zip(plan, dec)]


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
    ok = [r for r in table["decisions"] if r[0] >= 0]
    entries = sum(len(section_results(table, sec)) for row in table["table"] for sec in row)
    print(f"{args.out}: {len(table['layers'])} layers, {entries} entries, {len(table['plans'])} distinct plans, "
          f"{len(table['decisions'])} distinct decisions, {len(table['rows'])} distinct rows, routes {sorted({r[0] for r in ok})}, "
          f"thin kernels {sorted({r[5] for r in ok})}, {os.path.getsize(args.out)} bytes")
