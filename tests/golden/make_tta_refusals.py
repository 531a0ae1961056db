"""Table of what the adaptation plugins' constructors accept and refuse (tests/golden/tta_refusals.json, checked by
tests/test_tta_refusals_host.py).

A plugin reads its ``method.<block>`` mapping in its constructor, on the host, and refuses a value with an exception whose
type and text other tests and callers match on.  ``compute()`` constructs every registered plugin

  * from its base config (``BLOCKS``: the block's required keys, nothing else) - the defaults;
  * with every key of ``BLOCKS`` set, one at a time, to every value of ``PROBES``: numbers below and above every range of the
    package, the range ends, bools, NaN and the infinities, and values of a wrong type;
  * with ``method.moddrop.enabled: true``;

and records per construction either ``["ok", records]`` - the plugin's ``records`` tuple, dtypes by name - or
``["raises", exception type, message]``, the probed value in the message written as ``{v}`` (``outcome``).

    python tests/golden/make_tta_refusals.py [--repo ROOT]      # writes tests/golden/tta_refusals.json

``--repo`` names the checkout whose package is asked (default: this one).  The committed table was written from the commit
before the checks moved into shared helpers; regenerate it only from a commit whose messages are the reference.

File format: ``outcomes`` the distinct outcomes; ``table`` = {plugin: {"default": i, "moddrop": i, "keys": {key: [i per probe,
``PROBES`` order]}}} with i an index into ``outcomes``.
"""
import argparse
import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "tta_refusals.json")

NAN, INF = float("nan"), float("inf")
# name -> value; the name is what the messages of a failing test show
PROBES = {
    "-inf": -INF, "-1e9": -1e9, "-2": -2, "-1.0": -1.0, "-1e-3": -1e-3, "0": 0, "0.0": 0.0, "1e-30": 1e-30, "1e-7": 1e-7,
    "1e-3": 1e-3, "0.5": 0.5, "1": 1, "1.0": 1.0, "1.5": 1.5, "2": 2, "3": 3, "4": 4, "4.5": 4.5, "6": 6, "16": 16, "16.5": 16.5,
    "17": 17, "18": 18, "26": 26, "64": 64, "65": 65, "1e9": 1e9, "2^64 - 1": (1 << 64) - 1, "2^64": 1 << 64, "inf": INF,
    "nan": NAN, "true": True, "false": False, "'x'": "x", "'min'": "min", "'1'": "1", "[]": [], "[1]": [1], "[2, 2, 2]": [2, 2, 2],
    "[1.0, nan, 0.0]": [1.0, NAN, 0.0], "[true, 0, 0]": [True, 0, 0],
    "[[0], [1]]": [[0], [1]], "['d']": ["d"], "{}": {}, "{'k': [1]}": {"k": [1]},
}

INTENSITY = ("intensity", "intensity.copies", "intensity.scale", "intensity.noise_std", "intensity.per_channel", "intensity.seed")
AFFINE = ("affine", "affine.views", "affine.rotate", "affine.scale", "affine.seed")
# plugin -> (block name, the block's required keys, the keys probed)
BLOCKS = {
    "entmin_tta": (None, {}, ()),
    "seg_supervised_step": (None, {}, ()),
    "sar_tta": ("sar", {}, ("e_margin", "rho")),
    "memo_tta": ("memo", {}, ("mirror_axes", "ensemble", "rot90", "rot90.k") + INTENSITY),
    "cotta_tta": ("cotta", {}, ("mirror_axes", "rot90", "alpha", "restore_p", "seed") + INTENSITY + AFFINE),
    "petal_tta": ("petal", {}, ("mirror_axes", "rot90", "alpha", "restore_p", "seed", "quantile")),
    "eata_tta": ("eata", {}, ("e_margin", "fisher_alpha", "fisher.volumes")),
    "deyo_tta": ("deyo", {}, ("e_margin", "e_margin0", "plpd_threshold", "patches", "seed")),
    "lame_tta": ("lame", {}, ("iterations", "weight", "sigma", "connectivity")),
    "crf_tta": ("crf", {}, ("weight", "sigma", "connectivity", "form")),
    "bnm_tta": ("bnm", {}, ("weight", "entropy_weight", "block", "eps")),
    "innorm_tta": ("innorm", {}, ("lr", "gamma", "bound.log_scale", "bound.shift", "bound.log_gamma")),
    "biasfield_tta": ("biasfield", {}, ("lr", "order", "anchor", "l2", "bound.gain", "bound.field")),
    "modcons_tta": ("modcons", {}, ("subsets", "weight", "entropy_weight", "detach")),
    "window_tta": ("window", {"roi": [8, 8, 8]}, ("roi", "overlap", "mode", "sigma_scale", "floor", "pad_value")),
}


def config(plugin, key=None, value=None, moddrop=False):
    """The root config of one construction."""
    block, required, _ = BLOCKS[plugin]
    method = {}
    if block is not None:
        node = method[block] = copy.deepcopy(required)
        if key is not None:
            parts = key.split(".")
            for p in parts[:-1]:
                node = node.setdefault(p, {})
            node[parts[-1]] = copy.deepcopy(value)
    if moddrop:
        method["moddrop"] = {"enabled": True, "p": 0.25}
    return {"method": method}


def outcome(plugin, cfg, value=None):
    """One construction.  A refusal's message is stored with the probed value's repr behind the first " = " written as
    ``{v}`` (most messages open "<key> = <value>: expected ..."), so that the probes of a key share a few outcomes: the
    comparison stays exact, the value being known."""
    from multimodal_tta_amd.registry import get_plugin

    try:
        plug = get_plugin(plugin)(cfg)
    except Exception as exc:          # (whatever the constructor raises is what a caller meets)
        return ["raises", type(exc).__name__, str(exc).replace(f" = {value!r}:", " = {v}:", 1)]
    return ["ok", [[k, buf, str(dt)] for k, buf, dt in plug.records]]


def compute():
    """{"probes", "outcomes", "table"} from the importable multimodal_tta_amd."""
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    from multimodal_tta_amd.tta import EntropyMinimizationTTA

    methods = [p for p in list_plugins() if issubclass(get_plugin(p), EntropyMinimizationTTA)]
    assert sorted(BLOCKS) == sorted(methods), "an adaptation plugin without a row in BLOCKS (or a row without a plugin)"
    outcomes, table = {}, {}

    def index(o):
        return outcomes.setdefault(json.dumps(o), len(outcomes))

    for plugin, (_, _, keys) in BLOCKS.items():
        table[plugin] = {"default": index(outcome(plugin, config(plugin))),
                         "moddrop": index(outcome(plugin, config(plugin, moddrop=True))),
                         "keys": {key: [index(outcome(plugin, config(plugin, key, v), v)) for v in PROBES.values()] for key in keys}}
    return {"probes": list(PROBES), "outcomes": [json.loads(o) for o in outcomes], "table": table}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repo", default=os.path.dirname(TESTS), help="checkout whose package is asked")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    table = compute()
    with open(args.out, "w") as fh:          # one outcome, one key per line
        dump = lambda o: json.dumps(o, separators=(",", ":"))
        fh.write('{"probes":' + dump(table["probes"]) + ',\n"outcomes":[\n' + ",\n".join(dump(o) for o in table["outcomes"]) + '],\n"table":{\n')
        fh.write(",\n".join(f'{dump(p)}:{{"default":{r["default"]},"moddrop":{r["moddrop"]},"keys":{{\n'
                             + ",\n".join(f" {dump(k)}:{dump(v)}" for k, v in r["keys"].items()) + "}}"
                             for p, r in table["table"].items()) + "}}\n")
    entries = sum(2 + len(PROBES) * len(row["keys"]) for row in table["table"].values())
    refused = sum(1 for o in table["outcomes"] if o[0] == "raises")
    print(f"{args.out}: {len(table['table'])} plugins, {entries} constructions, {len(table['outcomes'])} distinct outcomes "
          f"({refused} refusals), {os.path.getsize(args.out)} bytes")
