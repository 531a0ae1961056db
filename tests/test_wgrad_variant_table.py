"""The decisions of a weight gradient (csrc/conv_wgrad.hip::plan_wgrad: the route and its reduction plan, and the variant of the
route - raw staging, the optimizer step in the main kernel's epilogue) against the recorded table
tests/golden/wgrad_variants.json - host-only, nothing is launched.

The table was written by tests/golden/make_wgrad_variants.py from the commit before the variant moved into the plan: the
layers of tests/golden/make_wgrad_plans.py, crossed with desc.dtype, the operands' storage types, parameter sets of one and of
two items, base addresses, ragged row strides, the norm-on-load of x, options 11, 13, 16 and 19 and the tuning for 1 / 4 / 24
volumes in flight (the generator's docstring says which axis a layer varies).  Equality is exact, entry by entry."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUTES = {0, 1, 2, 3, 6, 7, 8, 9, 10}      # WRoute of csrc/conv_wgrad.hip (4 and 5 are retired)
KERNEL, STAGES_RAW, UPDATES = 0, 7, 8      # columns of a result (the generator's FIELDS)


def _generator():
    spec = importlib.util.spec_from_file_location("make_wgrad_variants", os.path.join(GOLDEN, "make_wgrad_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _leaky_twins(gen, table):
    """(column, answer of the LeakyReLU call, answer of its twin with a plain descriptor) wherever the twin answers non-zero."""
    out = []
    for layer, row in zip(table["layers"], table["table"]):
        for dtype, sec in zip(gen.SECTIONS, row):
            if "leaky" not in gen.call_axes(layer, dtype)["x_norm"]:
                continue
            by_call = {}
            for (opts, call), res in zip(gen.combos(layer, dtype), gen.section_results(table, sec)):
                rest = (tuple(opts.items()), tuple((k, v) for k, v in call.items() if k != "x_norm"))
                by_call.setdefault(rest, {})[call["x_norm"]] = res
            for kinds in by_call.values():
                out += [(col, kinds["leaky"][col], kinds["null"][col]) for col in (STAGES_RAW, UPDATES) if kinds["null"][col] > 0]
    return out


def test_wgrad_variants_equal_the_recorded_table():
    from multimodal_tta_amd import ops

    gen = _generator()
    path = os.path.join(GOLDEN, "wgrad_variants.json")
    with open(path) as fh:
        want = json.load(fh)
    assert os.path.getsize(path) < (1 << 20), "the project keeps committed files under 1 MiB"
    # a table that silently lost a route, a variant or the LeakyReLU exception fails here
    ok = [r for r in want["results"] if r[KERNEL] >= 0]
    assert {r[KERNEL] for r in ok} == ROUTES
    assert {r[STAGES_RAW] for r in ok} == {0, 2, 3}
    assert {0, 1} <= {r[UPDATES] for r in ok}
    twins = _leaky_twins(gen, want)
    assert {col for col, _, _ in twins} == {STAGES_RAW, UPDATES}, "a LeakyReLU call next to a twin that answers non-zero, per query"
    assert all(leaky == 0 for _, leaky, _ in twins)

    before, tuned_for = gen.options(ops), ops._TUNED_FOR
    got = gen.compute()
    assert gen.options(ops) == before and ops._TUNED_FOR == tuned_for, "compute() must leave the options and the tuning as they were"

    assert got["layers"] == want["layers"], "the layer list changed: regenerate the table from the reference commit"
    for layer, g_row, w_row in zip(want["layers"], got["table"], want["table"]):
        assert len(g_row) == len(w_row) == len(gen.SECTIONS)
        for dtype, g_sec, w_sec in zip(gen.SECTIONS, g_row, w_row):
            if g_sec == w_sec and all(got[k] == want[k] for k in ("rows", "results")):
                continue                    # (the same rows over the same results: every entry is equal)
            g, w = gen.section_results(got, g_sec), gen.section_results(want, w_sec)
            combos = gen.combos(layer, dtype)
            assert len(g) == len(w) == len(combos)
            for (opts, call), gr, wr in zip(combos, g, w):
                assert gr == wr, f"layer {layer} dtype {dtype}, options {opts}, call {call}: {gen.FIELDS} = {gr}, recorded {wr}"
