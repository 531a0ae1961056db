"""The case table of tests/pointwise_classes.py without a GPU: every case reaches the dispatch class it names
(mmtta_pointwise_route on made-up addresses), the table covers the reachable classes exactly, and the conditions that keep the
GPU comparisons of tests/test_hip_pointwise_classes.py honest hold for the chosen shapes and seeds."""
import ctypes as C

import numpy as np
import pytest

import pointwise_classes as pc
from multimodal_tta_amd import _lib, ops

ROUTES = {c.name: pc.host_route(c) for c in pc.CASES}
SUM_OPS = ("stats", "bwd_reduce", "stats_chain", "bwd_chain")


def _long_sums(case, route):
    """(item, channel) totals whose bound passes 0.25: 256 voxel lanes (C <= 4) over >= 16 400 voxels.  These are held row
    by row, where the bound stays below 0.02."""
    return route["nvl"] == 256 and case.shape[2] * case.shape[3] * case.shape[4] >= 16400


def test_route_struct_matches_the_header():
    assert C.sizeof(_lib.PointwiseRoute) == 96        # 3 x int64 + 18 x int32
    assert len(_lib.PW_OPS) == 8 and len(_lib.PW_FAMILIES) == 9


@pytest.mark.parametrize("case", pc.CASES, ids=[c.name for c in pc.CASES])
def test_case_reaches_its_class(case):
    pc.check_route(case, ROUTES[case.name])


def _by_prefix(prefix):
    (name,) = [n for n in ROUTES if n.startswith(prefix)]
    return ROUTES[name]


def test_route_query_reports_the_launch_geometry():
    r = ROUTES["stats_rpb2_c4_f_none"]
    assert (r["rows_per_n"], r["rows_per_block"], r["grid_x"], r["grid_y"], r["vox_per_row"]) == (513, 2, 257, 2, 32)
    assert (r["cpl"], r["nvl"], r["trips"], r["it"]) == (1, 256, 1, 1)
    r = ROUTES["stats_old_c1028_f_none"]
    assert (r["cpl"], r["nvl"], r["trips"], r["cb_passes"], r["grid_x"]) == (256, 1, 32, 2, 1)
    r = _by_prefix("combine8_it4_f_one_")
    assert (r["vec"], r["it"], r["cpl"], r["nvl"], r["grid_x"], r["grid_y"]) == (8, 4, 256, 1, 1024, 1)
    r = ROUTES["second_trip_up_bwd"]
    assert r["work_items"] == 3 * 112 ** 3 > r["grid_x"] * 256 and r["second_trip"] == 1
    r = _by_prefix("small_ff_c512_v30_")
    assert (r["grid_x"], r["grid_y"], r["it"], r["trips"]) == (16, 2, 2, 2)


def test_route_query_rejects_what_the_entry_points_reject():
    t = pc.host_desc((1, 8, 2, 2, 2), pc.TIGHT, False, 0)
    t16 = pc.host_desc((1, 8, 2, 2, 2), pc.TIGHT, True, 1)
    other = pc.host_desc((1, 8, 2, 2, 3), pc.TIGHT, False, 2)
    for op, operands in (("combine", [t, other]), ("combine", [t, t16]), ("combine", [t]), ("upsample_fwd", [t, t]),
                         ("lincomb", [t16, t, t]), ("lincomb", [t]), ("norm_bwd_small", [t, t, t]), ("channel_stats", [t, t])):
        with pytest.raises(_lib.MmttaError):
            ops.pointwise_route(op, operands)
    nl = _lib.norm_on_load(act=7)
    nl.mean = nl.rstd = pc.FAKE
    with pytest.raises(_lib.MmttaError):
        ops.pointwise_route("norm_bwd_reduce", [t, t], nl)


# ----------------------------------------------------------------------------- coverage
def test_table_covers_the_reachable_instantiations_exactly():
    got = {}
    for c in pc.CASES:
        got.setdefault(pc.klass(ROUTES[c.name]), []).append(c.name)
    missing, drifted = sorted(pc.REACHABLE - set(got)), {k: v for k, v in got.items() if k not in pc.REACHABLE}
    assert not missing, f"instantiations no case reaches: {missing}"
    assert not drifted, f"cases outside the list of reachable instantiations: {drifted}"


def test_table_covers_the_launch_geometry_classes():
    routes = ROUTES.values()
    assert {r["rows_per_block"] for r in routes if r["family"] == "reduce_stream"} == pc.REACHABLE_ROWS_PER_BLOCK
    assert {(r["family"], r["cb_passes"]) for r in routes if r["family"] in ("reduce", "reduce_stream")} == pc.REACHABLE_CB
    # the last workgroup of an item walks fewer rows than the others
    assert any(r["rows_per_block"] == k and r["rows_per_n"] % k for k in (2, 4) for r in routes)
    assert {(r["family"], r["mode"], r["second_trip"]) for r in routes
            if r["family"] in ("elementwise", "lincomb", "upsample_fwd", "upsample_bwd")} == pc.REACHABLE_SECOND_TRIP
    # more and fewer than 64 partial rows per item through the finalize kernels (the wave's second trip)
    for op in ("stats_chain", "bwd_chain"):
        rows = [ROUTES[c.name]["rows_per_n"] for c in pc.cases_of(op)]
        assert min(rows) < 64 < max(rows), (op, rows)
    # the streamed tail: a row shorter than the others, and items that are one short row
    assert any(r["family"] == "reduce_stream" and r["rows_per_n"] == 1 for r in routes)
    for c in pc.CASES:
        r = ROUTES[c.name]
        if r["family"] in ("elementwise", "lincomb", "upsample_fwd", "upsample_bwd") and not r["second_trip"]:
            assert r["work_items"] <= 1e5, f"{c.name}: only the second-trip cases may be large"


def test_every_family_meets_every_activation():
    seen = {}
    for c in pc.CASES:
        r = ROUTES[c.name]
        if r["family"] in pc.LEAKY_FAMILIES and (r["family"] != "reduce" or r["mode"] == 1) and (r["family"] != "reduce_stream" or r["mode"] == 1):
            seen.setdefault((r["family"], r["mode"]), set()).add(c.act)
            assert r["leaky"] == int(c.act == "leaky" or (bool(c.kw.get("two")) and c.kw.get("act_b") == "leaky"))
        else:
            assert r["leaky"] == 0
    lacking = {k: v for k, v in seen.items() if v != {"none", "relu", "leaky"}}
    assert not lacking and len(seen) == 7, (lacking, sorted(seen))


# ----------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("case", pc.cases_of(*SUM_OPS), ids=[c.name for c in pc.cases_of(*SUM_OPS)])
def test_sum_bounds_catch_one_dropped_voxel(case):
    o, route = pc.make(case), ROUTES[case.name]
    x = o["x"] if "x" in o else o["dout"]
    assert np.abs(x).min() >= 0.5
    ref = pc.ref_sums(case, o, route)
    near = ref.pop("near", None)
    for name in ("s0",) if near is None or not near.any() else ():
        assert ref[name][1].max() < 0.25, f"{case.name}: row bound {ref[name][1].max():.3f}"
        total = ref[name][1].sum(1).max()
        assert total < 0.25 or _long_sums(case, route), f"{case.name}: (item, channel) bound {total:.3f}"
    if case.act == "none":
        # the reference without one voxel (the last of an item: the short row's) differs by more than any bound allows
        dropped = {k: v.copy() for k, v in o.items() if isinstance(v, np.ndarray)}
        (dropped["x"] if "x" in o else dropped["dout"])[-1, -1, -1, -1, :] = 0.0
        ref2 = pc.ref_sums(case, dropped, route)
        gap = np.abs(ref2["s0"][0] - ref["s0"][0])[-1, -1]
        assert (gap > ref["s0"][1][-1, -1]).all()
        assert (gap > ref["s0"][1].sum(1)[-1]).all() or _long_sums(case, route)


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.act != "none"], ids=[c.name for c in pc.CASES if c.act != "none"])
def test_few_elements_sit_on_the_kink(case):
    share = pc.near_share(case, pc.make(case))
    assert share <= pc.NEAR_CAP, f"{case.name}: {share:.2e} of the elements have |z| < {pc.Z_NEAR}"


def test_offset_mean_cases_prove_something():
    cases = [c for c in pc.cases_of("stats_chain") if c.kw.get("offset")]
    assert sorted(c.kw["kind"] for c in cases) == ["BATCH", "GROUP", "INSTANCE"]
    for case in cases:
        o = pc.make(case)
        x = o["x"]
        ratio = np.abs(x.mean((1, 2, 3))) / x.std((1, 2, 3))
        assert 28.0 < ratio.min() and ratio.max() < 32.0, (ratio.min(), ratio.max())
        rel = pc.ref_stats_chain(case, o, ROUTES[case.name])["_rstd_rel"]
        assert rel < 0.05, f"{case.name}: derived relative bound of rstd {rel:.3f}"
