"""The weight gradient's planner (csrc/conv_wgrad.hip::wgeometry: route = kernel id, slabs, pre-reduce chunks, padded channel
counts, workspace bytes, status codes) against the recorded table tests/golden/wgrad_plans.json - host-only, no GPU.

The table was written by tests/golden/make_wgrad_plans.py from the commit before the planner was split from the launch code
(route enum, one slab planner, one bias-source decision): every parity case of tests/test_hip_conv.py and every convolution
of the registered models at 128^3 (batch 1 and 8), crossed with desc.dtype, the operands' storage types, parameter sets, base
addresses, a ragged row stride, options 11 and 13 and the tuning for 1 / 4 / 24 volumes in flight; plus the argument errors
by status code.  Equality is exact, entry by entry."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIVE_IDS = {0, 1, 2, 3, 6, 7, 8, 9, 10}        # ids 4 / 5 are retired


def _generator():
    spec = importlib.util.spec_from_file_location("make_wgrad_plans", os.path.join(GOLDEN, "make_wgrad_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wgrad_plans_equal_the_recorded_table():
    from multimodal_tta_amd import ops

    gen = _generator()
    with open(os.path.join(GOLDEN, "wgrad_plans.json")) as fh:
        want = json.load(fh)
    assert os.path.getsize(os.path.join(GOLDEN, "wgrad_plans.json")) < (1 << 20), "the project keeps committed files under 1 MiB"
    # a table that silently lost a route fails here
    assert {r[1] for r in want["results"] if r[0] == 0} == LIVE_IDS

    before, tuned_for = gen.options(ops), ops._TUNED_FOR
    got = gen.compute()
    assert gen.options(ops) == before and ops._TUNED_FOR == tuned_for, "compute() must leave the options and the tuning as they were"

    assert got["layers"] == want["layers"], "the layer list changed: regenerate the table from the reference commit"
    assert got["errors"] == want["errors"]
    assert [e["name"] for e in want["errors"]] == ["wrong op", "ksize 5", "stride 3", "channel mismatch", "spatial mismatch",
                                                   "odd fine extent of a transposed convolution"]
    assert all(e["status"] != 0 for e in want["errors"])
    combos = gen.combos()
    for layer, g_runs, w_runs in zip(want["layers"], got["table"], want["table"]):
        g, w = gen.unrle(g_runs), gen.unrle(w_runs)
        assert len(g) == len(w) == len(combos)
        for combo, gi, wi in zip(combos, g, w):
            assert got["results"][gi] == want["results"][wi], \
                f"layer {layer}, {dict(zip(gen.AXES, combo))}: [status, kernel, nsl, pre_chunks, CGp, CDp, workspace bytes] = " \
                f"{got['results'][gi]}, recorded {want['results'][wi]}"
