"""The decisions of a forward / input-gradient convolution run (csrc/conv_igemm.hip::plan_run: the route, and the variant of the
route - raw staging, the pipelined class-fused kernel, its lean epilogue, the thin kernels of routes 6 and 13 and their lean
forms, the head convolution with the loss in its epilogue) against the recorded table tests/golden/conv_variants.json -
host-only, nothing is launched.

The table was written by tests/golden/make_conv_variants.py from the commit before the variant moved into the run plan: the
cases of tests/conv_geometry.py, two class-fused layers whose channel counts are no multiple of 8 and every convolution of the
registered models at 128^3, forward and input gradient, crossed with desc.dtype, the operands' storage types, the norm-on-load
of x, the fused add, statistics rows, accumulate, base addresses, ragged row strides, the options that pick a variant and the
tuning for 1 / 4 / 24 volumes in flight (the generator's docstring says which axis a layer varies).  Equality is exact, entry
by entry."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUTES = set(range(19))                  # 0 - 5, 7 - 12, 14: implicit-GEMM tiles; 6, 13, 15 - 18: the other kernels
THIN_KERNELS = set(range(1, 14))         # THIN_* of csrc/common.h
# [plan status, plan bytes, route, stages_raw, cls8_pipelined, cls8_lean_epilogue, thin_lean, thin_kernel, head_loss_eligible]
FIELDS = ("plan status", "plan bytes", "route", "stages_raw", "cls8_pipelined", "cls8_lean_epilogue", "thin_lean", "thin_kernel",
          "head_loss_eligible")


def _generator():
    spec = importlib.util.spec_from_file_location("make_conv_variants", os.path.join(GOLDEN, "make_conv_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_variants_equal_the_recorded_table():
    from multimodal_tta_amd import ops

    gen = _generator()
    path = os.path.join(GOLDEN, "conv_variants.json")
    with open(path) as fh:
        want = json.load(fh)
    assert os.path.getsize(path) < (1 << 20), "the project keeps committed files under 1 MiB"
    # a table that silently lost a route, a thin kernel or a whole query fails here
    ok = [r for r in want["decisions"] if r[0] >= 0]
    assert {r[0] for r in ok} == ROUTES
    assert {r[5] for r in ok if r[5] > 0} == THIN_KERNELS
    assert any(r[5] < 0 for r in ok), "a thin kernel's refusal on a call whose route is planned"
    for col, name in enumerate(FIELDS[2:]):
        assert any(r[col] > 0 for r in ok), f"{name} answers non-zero nowhere"
    assert {r[4] for r in ok} == {0, 1, 2}
    assert all(p[0] == 0 for p in want["plans"])

    before, tuned_for = gen.options(ops), ops._TUNED_FOR
    got = gen.compute()
    assert gen.options(ops) == before and ops._TUNED_FOR == tuned_for, "compute() must leave the options and the tuning as they were"

    assert got["layers"] == want["layers"], "the layer list changed: regenerate the table from the reference commit"
    for layer, g_row, w_row in zip(want["layers"], got["table"], want["table"]):
        assert len(g_row) == len(w_row) == len(gen.SECTIONS)
        for (orientation, dtype), g_sec, w_sec in zip(gen.SECTIONS, g_row, w_row):
            if g_sec == w_sec and all(got[k] == want[k] for k in ("rows", "plans", "decisions")):
                continue                    # (the same rows over the same plans and decisions: every entry is equal)
            g, w = gen.section_results(got, g_sec), gen.section_results(want, w_sec)
            combos = gen.combos(layer, orientation, dtype)
            assert len(g) == len(w) == len(combos)
            for (opts, call), gr, wr in zip(combos, g, w):
                assert gr == wr, f"layer {layer} {orientation} dtype {dtype}, options {opts}, call {call}: {FIELDS} = {gr}, recorded {wr}"
