"""The planner of the forward / input-gradient convolution (csrc/conv_igemm.hip::geometry, as mmtta_conv_plan reports it: tiles,
launches, ksplit, statistics rows, config = route of the shape, workspace bytes, status codes) against the recorded table
tests/golden/conv_plans.json - host-only, no GPU.

The table was written by tests/golden/make_conv_plans.py from the commit before the planner was split from the launch code
(route enum, one planner for plan and run): every parity case of tests/test_hip_conv.py and every convolution of the
registered models at 128^3 (batch 1 and 8), forward and input gradient, crossed with desc.dtype, the operands' storage types,
base addresses, a ragged row stride, options 9, 10, 12 and 13 and the tuning for 1 / 4 / 24 volumes in flight; plus the
argument errors by status code.  Equality is exact, entry by entry."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = "[status, tiles, launches, ksplit, stats_rows, config, _pad, workspace bytes]"


def _generator():
    spec = importlib.util.spec_from_file_location("make_conv_plans", os.path.join(GOLDEN, "make_conv_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_plans_equal_the_recorded_table():
    from multimodal_tta_amd import ops

    gen = _generator()
    with open(os.path.join(GOLDEN, "conv_plans.json")) as fh:
        want = json.load(fh)
    assert os.path.getsize(os.path.join(GOLDEN, "conv_plans.json")) < (1 << 20), "the project keeps committed files under 1 MiB"
    # a table that silently lost a route fails here
    assert {r[5] for r in want["results"] if r[0] == 0} == set(range(16))

    before, tuned_for = gen.options(ops), ops._TUNED_FOR
    got = gen.compute()
    assert gen.options(ops) == before and ops._TUNED_FOR == tuned_for, "compute() must leave the options and the tuning as they were"

    assert got["layers"] == want["layers"], "the layer list changed: regenerate the table from the reference commit"
    assert got["errors"] == want["errors"]
    assert [e["name"] for e in want["errors"]] == ["bad op", "ksize 5", "stride 3", "1x1x1 with stride 2", "channel mismatch",
                                                   "batch mismatch", "spatial mismatch",
                                                   "odd extent for the transposed input gradient", "non-channels-last"]
    assert all(e["status"] != 0 for e in want["errors"])
    combos = gen.combos()
    assert len(got["table"]) == len(want["table"]) == 2 * len(want["layers"])
    for i, (gr, wr) in enumerate(zip(got["table"], want["table"])):
        g, w = gen.unrle(got["rows"][gr]), gen.unrle(want["rows"][wr])
        assert len(g) == len(w) == len(combos)
        for combo, gi, wi in zip(combos, g, w):
            assert got["results"][gi] == want["results"][wi], \
                f"layer {want['layers'][i // 2]} ({'input gradient' if i % 2 else 'forward'}), {dict(zip(gen.AXES, combo))}: " \
                f"{FIELDS} = {got['results'][gi]}, recorded {want['results'][wi]}"
