"""What the adaptation plugins' constructors accept and refuse, against the recorded table tests/golden/tta_refusals.json -
host-only, nothing is launched.

The table was written by tests/golden/make_tta_refusals.py from the commit before the range, type, seed and moddrop checks of
the plugins moved into shared helpers: every plugin from its defaults, with every key of its ``method.<block>`` mapping at
every probe value of the generator (below and above every range, range ends, bools, NaN, infinities, wrong types) and with
``method.moddrop.enabled: true``.  An accepted construction is recorded with the plugin's ``records`` tuple, a refused one
with the exception's type and message.  Equality is exact: a message that differs is a bug in the code, not in the table."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_tta_refusals", os.path.join(GOLDEN, "make_tta_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_constructor_outcomes_equal_the_recorded_table():
    gen = _generator()
    path = os.path.join(GOLDEN, "tta_refusals.json")
    with open(path) as fh:
        want = json.load(fh)
    assert os.path.getsize(path) < (1 << 20), "the project keeps committed files under 1 MiB"
    # a table that lost its refusals, a plugin or a kind of probe fails here
    assert want["probes"] == list(gen.PROBES) and {"nan", "true", "'x'", "-1e9", "1e9"} <= set(want["probes"])
    assert sorted(want["table"]) == sorted(gen.BLOCKS)
    kinds = {(o[0], o[1]) if o[0] == "raises" else ("ok",) for o in want["outcomes"]}
    assert {("ok",), ("raises", "ValueError"), ("raises", "NotImplementedError")} <= kinds
    refusing = sorted(p for p, row in want["table"].items() if want["outcomes"][row["moddrop"]][0] == "raises")
    assert refusing == sorted(["memo_tta", "cotta_tta", "petal_tta", "deyo_tta", "innorm_tta", "biasfield_tta", "modcons_tta",
                               "window_tta"]), "the plugins that refuse modality dropout"

    got = gen.compute()
    for plugin, w_row in want["table"].items():
        g_row = got["table"][plugin]
        for what in ("default", "moddrop"):
            g, w = got["outcomes"][g_row[what]], want["outcomes"][w_row[what]]
            assert g == w, f"{plugin}, {what}: {g}, recorded {w}"
        assert list(g_row["keys"]) == list(w_row["keys"])
        for key, w_idx in w_row["keys"].items():
            for probe, gi, wi in zip(want["probes"], g_row["keys"][key], w_idx):
                g, w = got["outcomes"][gi], want["outcomes"][wi]
                assert g == w, f"{plugin}: method.{gen.BLOCKS[plugin][0]}.{key} = {probe}: {g}, recorded {w}"
