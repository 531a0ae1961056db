"""Table of weight-gradient plans (tests/golden/wgrad_plans.json, checked by tests/test_wgrad_plan.py).

The planner of the weight gradient (csrc/conv_wgrad.hip::wgeometry) reads descriptors and options, never tensor memory, so
it can be asked about any shape at any address without a GPU.  ``compute()`` asks it about every layer below under every
combination of the axes in ``AXES`` and records, per entry, the status code, the kernel id (mmtta_conv_wgrad_kernel), the
four integers of mmtta_conv_wgrad_plan_sets and mmtta_conv_wgrad_workspace_bytes_sets.

    python tests/golden/make_wgrad_plans.py [--repo ROOT]      # writes tests/golden/wgrad_plans.json

``--repo`` names the checkout whose library is asked (default: this one).  The committed table was written from the commit
before the planner was split from the launch code; regenerate it only from a commit whose plans are the reference.

File format: ``layers`` (cin, cout, k, stride, transposed, [n, d, h, w]) without duplicates; ``results`` the distinct
[status, kernel id, nsl, pre_chunks, CGp, CDp, workspace bytes]; ``table[i]`` the results of layer i over the combinations
in the order of ``combos()``, run-length encoded as [result index, count, result index, count, ...]; ``errors`` the
argument errors by status code.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "wgrad_plans.json")

F32, BF16 = 0, 1          # include/mmtta.h dtype codes (checked against _lib in compute())
# every axis of the cross product; the first three are process-wide options, the rest describe one call
AXES = {
    "volumes_in_flight": (1, 4, 24),                      # ops.tune_for_volumes_in_flight
    "opt11": (0, 1),                                      # MMTTA_OPT_WGRAD_VECTOR_STAGING
    "opt13": (0, 1, 2, 3),                                # MMTTA_OPT_THIN_MFMA
    "dtype": (F32, BF16),                                 # desc.dtype
    "storage": ((F32, F32), (BF16, F32), (BF16, BF16), (F32, BF16)),      # (x, dy); the last is the pair the planner refuses for bf16 kernels
    "sets": (0, 1),                                       # no parameter sets / sets of one item each
    "base_offset": (0, 4, 8),                             # bytes past a 64-byte boundary, both tensors
    "row_pad": (0, 1),                                    # 1: a voxel row one element longer, so no multiple of 4
}
MODEL_EDGE, MODEL_BATCHES = 128, (1, 8)


def combos():
    return list(itertools.product(*AXES.values()))


def model_layers():
    """Every convolution of the registered models at 128^3: shapes from a forward of the torch oracle on the meta device."""
    import torch

    import oracle
    from multimodal_tta_amd import registry
    from multimodal_tta_amd.config import compose

    seen = []

    def hook(mod, inp, out):
        seen.append((mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride[0],
                     isinstance(mod, torch.nn.ConvTranspose3d), tuple(inp[0].shape[2:])))

    for name in registry.MODELS.list_all():
        cfg = compose(overrides=["task=brats", f"model={name}"])["model"]
        cls = oracle.UNet if cfg["name"] == "unet" else oracle.MultimodalUNetDeepFusion
        with torch.device("meta"):
            net = cls(cfg)
        for mod in net.modules():
            if isinstance(mod, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
                mod.register_forward_hook(hook)
        net(torch.empty(1, cfg["in_channels"], MODEL_EDGE, MODEL_EDGE, MODEL_EDGE, device="meta"))
    return [(ci, co, k, s, t, (n,) + sp) for (ci, co, k, s, t, sp) in seen for n in MODEL_BATCHES]


def layers():
    sys.path.insert(0, TESTS)
    try:
        from test_hip_conv import BF16_CASES, CASES, THIN_TR_CASES, TR_CASES
    finally:
        sys.path.remove(TESTS)
    out = []
    for case in list(CASES) + list(BF16_CASES) + list(TR_CASES) + list(THIN_TR_CASES) + model_layers():
        case = tuple(case[:5]) + (tuple(case[5]),)
        if case not in out:                 # the same layer from two lists is the same input: one entry
            out.append(case)
    return out


def tensor(_lib, base, n, c, dhw, dtype, offset, row_pad):
    d, h, w = dhw
    sw = ((c + 3) // 4 * 4 if (dtype == F32 or c <= 4) else (c + 7) // 8 * 8) + row_pad
    return _lib.Tensor(base + offset, n, c, d, h, w, d * h * w * sw, 1, h * w * sw, w * sw, sw, dtype, 0)


def out_dhw(dhw, stride, transposed):
    return tuple(2 * v if transposed else (v if stride == 1 else (v + 1) // 2) for v in dhw)


class Asker:
    def __init__(self, _lib):
        self._lib, self.lib = _lib, _lib.load()
        self.plan = (C.c_int32 * 4)()
        self.sets = _lib.ParamSets(1, 1, 0, 0, 0, 0, 0, 0)

    def ask(self, desc, tx, ty, sets):
        lib, sref = self.lib, (C.byref(self.sets) if sets else None)
        d, x, y = C.byref(desc), C.byref(tx), C.byref(ty)
        st = int(lib.mmtta_conv_wgrad_plan_sets(d, x, y, sref, self.plan))
        plan = list(self.plan) if st == 0 else [0, 0, 0, 0]
        return (st, int(lib.mmtta_conv_wgrad_kernel(d, x, y)), *plan, int(lib.mmtta_conv_wgrad_workspace_bytes_sets(d, x, y, sref)))


def error_cases(_lib):
    """(name, desc, x, dy): one argument error each."""
    D = _lib.ConvDesc
    fwd, dgrad, fwd_t = _lib.CONV_FWD, _lib.CONV_DGRAD, _lib.CONVT_FWD

    def t(base, c, dhw):
        return tensor(_lib, base, 1, c, dhw, F32, 0, 0)

    X, Y = 1 << 30, 1 << 32
    return [
        ("wrong op", D(dgrad, 3, 1, 32, 32, F32), t(X, 32, (8, 8, 8)), t(Y, 32, (8, 8, 8))),
        ("ksize 5", D(fwd, 5, 1, 32, 32, F32), t(X, 32, (8, 8, 8)), t(Y, 32, (8, 8, 8))),
        ("stride 3", D(fwd, 3, 3, 32, 32, F32), t(X, 32, (9, 9, 9)), t(Y, 32, (3, 3, 3))),
        ("channel mismatch", D(fwd, 3, 1, 32, 32, F32), t(X, 16, (8, 8, 8)), t(Y, 32, (8, 8, 8))),
        ("spatial mismatch", D(fwd, 3, 2, 32, 32, F32), t(X, 32, (8, 8, 8)), t(Y, 32, (8, 8, 8))),
        ("odd fine extent of a transposed convolution", D(fwd_t, 3, 2, 32, 32, F32), t(X, 32, (4, 4, 4)), t(Y, 32, (8, 9, 8))),
    ]


def options(ops):
    """The options this table varies, as they are now (mmtta_set_option returns the previous value)."""
    now = {}
    for key in list(ops.TUNE_AT_4) + [11, 13]:
        now[key] = ops.set_option(key, 1)
        ops.set_option(key, now[key])
    return now


def compute():
    """{"layers", "results", "table", "errors"} from the library of the importable multimodal_tta_amd; options and tuning are
    left as they were found."""
    from multimodal_tta_amd import _lib, ops

    assert (_lib.F32, _lib.BF16) == (F32, BF16)
    ask = Asker(_lib)
    lay = layers()
    ax = AXES
    per_call = list(itertools.product(ax["dtype"], ax["storage"], ax["sets"], ax["base_offset"], ax["row_pad"]))
    calls = []                      # per layer: [(desc, x, dy, sets)] in per_call order
    for cin, cout, k, stride, transposed, (n, *dhw) in lay:
        op = _lib.CONVT_FWD if transposed else _lib.CONV_FWD
        row = []
        for dtype, (sx, sy), sets, off, pad in per_call:
            row.append((_lib.ConvDesc(op, k, stride, cin, cout, dtype), tensor(_lib, 1 << 30, n, cin, dhw, sx, off, pad),
                        tensor(_lib, 1 << 40, n, cout, out_dhw(dhw, stride, transposed), sy, off, pad), sets))
        calls.append(row)
    results, index, flat = [], {}, [[] for _ in lay]
    tuned_for, saved = ops._TUNED_FOR, options(ops)
    try:
        for volumes in ax["volumes_in_flight"]:
            for key, val in ops.tune_for_volumes_in_flight(volumes).items():
                ops.set_option(key, val)            # (whether or not the call above did: MMTTA_NO_AUTOTUNE, already tuned)
            for o11 in ax["opt11"]:
                ops.set_option(11, o11)
                for o13 in ax["opt13"]:
                    ops.set_option(13, o13)
                    for i, row in enumerate(calls):
                        for call in row:
                            r = ask.ask(*call)
                            flat[i].append(index.setdefault(r, len(index)))
        errors = [{"name": name, "status": ask.ask(d, x, y, 0)[0]} for name, d, x, y in error_cases(_lib)]
    finally:
        for key, val in saved.items():
            ops.set_option(key, val)
        ops._TUNED_FOR = tuned_for
    results = [list(r) for r in index]          # insertion order = index
    return {"layers": [list(c[:5]) + [list(c[5])] for c in lay], "results": results, "table": [rle(f) for f in flat], "errors": errors}


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
    kids = sorted({r[1] for r in table["results"] if r[0] == 0})
    print(f"{args.out}: {len(table['layers'])} layers x {len(combos())} combinations, {len(table['results'])} distinct results, "
          f"kernel ids {kids}, {os.path.getsize(args.out)} bytes")
