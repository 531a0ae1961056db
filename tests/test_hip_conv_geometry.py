"""Parity of the implicit-GEMM convolutions and the weight gradients at every launch geometry the tuner sets, against an
exact-operand float64 reference (helpers and the case table: tests/conv_geometry.py).

The geometry axis.  Options 2 - 5 (split-K below / target, weight-gradient workgroups / thin slabs; option 12 rides along)
decide whether a workgroup runs the whole K loop or a slice of it, whether the epilogue runs in the main kernel or in
splitk_finalize_kernel, and how many tiles a weight-gradient slab loops over.  Every case runs under `inflight1`,
`inflight4`, `inflight24` (the return values of ops.tune_for_volumes_in_flight), `unsplit` (1 / 1 / 1 / 1) and `deep` (split
forced, the target searched per call so that 1 < ksplit < ceil(K / 32); 4 / 4 for the weight gradient).  Before launching,
each test asks mmtta_conv_plan / mmtta_conv_wgrad_plan_sets what it will get and asserts the class it is there for; the
classes rest on ksplit, config and K only (a stage is at most 32 channels deep).  The closing tests assert that every
implicit-GEMM config id is run unsplit with >= 2 stages, split with >= 2 stages per split and split with one stage per split,
and that route 15 runs under inflight24.  The same table is evaluated on the CPU by the two tests without the `gpu` mark.

The reference.  float64 torch F.conv3d / F.conv_transpose3d + autograd on the CPU.  For bf16 operands x, the weights, gy, the
residual operand and the accumulate prefill are bf16-representable (bf16 x bf16 products are exact in fp32), so the only
difference left is the fp32 accumulation order, and bf16 and fp32 kernels are held to the same bound:

    fp32-stored results    |got - ref| <= 2e-4 * max|ref| + 1e-5                   (tests/test_hip_conv.py's fp32 bound)
    bf16-stored results    |got - ref| <= 2^-8 * |ref| + 2e-4 * max|ref| + 1e-5    element by element

No case needed more than that, so the a-priori bound terms * 2^-24 * sum|products| is not evaluated.  No check here uses the
1.5e-2 bf16-operand bound.  Statistics rows are summed and compared with the float64 sums under test_hip_conv.py's bounds.

Norm-on-load.  The kernels compute relu(fmaf(x, scale, shift)) in fp32 and, for bf16 operands, round that to bf16.  The
descriptors here carry precombined scale / shift, the bf16-operand checks read a bf16-stored x, and the reference operand
is the same fused multiply-add evaluated in float64 and rounded to fp32, then to bf16.  The cap of operand elements allowed
to sit one bf16 ulp off is 1 in 1000: the CPU test measures, per case, the share that differs between this and the
two-rounding torch.addcmul transform and asserts it is inside the cap (observed: 0 for every case).  The exact bound applies
to every element.

MMTTA_OPT_IGEMM_PIPELINE (6) is crossed with the bf16 stride-1 3x3x3 cases under `unsplit` and `deep`, MMTTA_OPT_EPILOGUE_VEC16
(9) with every epilogue form under `unsplit`: bit-for-bit equal outputs (the statistics of option 9 within summation order).

Observed worst err / bound on an MI355X (recorded values, not limits): see DESIGN.md, "Parity rules".
"""
import ctypes as C

import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl, cl_bf16

GPU = pytest.mark.gpu
SEEN = set()            # (config, class) of every implicit-GEMM launch the GPU tests made
SEEN_WGRAD = set()      # (operand type, class) of every weight-gradient launch
RAN = set()             # (case, operand type, geometry) whose GPU test ran


def _params():
    return [pytest.param(c, dt, geo, id=f"{c.name}-{dt}-{geo}") for c in cg.CASES for dt in cg.DTYPES for geo in cg.GEOMETRIES]


def _storages(dtype):
    return (False, True) if dtype == "bf16" else (False,)


def _plan_table(cases=None):
    """Every call of the module, host-only: {(case, dtype, geo, orientation, stored_bf16): (values, ksplit, config, class)},
    with the class assertions of the forced geometries."""
    table = {}
    for c in (cases or cg.CASES):
        for dtype in cg.DTYPES:
            for geo in cg.GEOMETRIES:
                for orientation in ("fwd", "dgrad"):
                    for stored in (_storages(dtype) if orientation == "fwd" else (False,)):
                        vals, ksplit, config, cls = cg.planned(c, dtype, geo, orientation, stored)
                        if vals is not None:
                            cg.assert_planned_class(c, dtype, geo, orientation, ksplit, cg.reduction_depth(c, orientation))
                        table[(c.name, dtype, geo, orientation, stored)] = (vals, ksplit, config, cls)
    return table


def _wgrad_classes(c, dtype, geo):
    """{x storage: (plan, class)} with the assertions of the forced geometries."""
    out = {}
    with cg.pinned(cg.case_options(c)), cg.pinned(cg.geometry_values(geo)):
        for x_bf16 in _storages(dtype):
            plan = cg.ask_wgrad_plan(c, dtype, x_bf16)
            if geo == "unsplit" and c.k == 3:
                assert plan[0] == 1, f"{c.name} {dtype}: unsplit weight gradient planned {plan[0]} slabs"
            if geo == "deep" and c.k == 3:
                assert plan[0] <= 4, f"{c.name} {dtype}: deep weight gradient planned {plan[0]} slabs"
            out[x_bf16] = (plan, cg.wgrad_class(c, geo, plan))
    return out


def _assert_complete(seen, seen_wgrad):
    missing = [(cfg, cls) for cfg in cg.IGEMM_CONFIGS for cls in cg.CLASSES if (cfg, cls) not in seen]
    assert not missing, f"(config, class) pairs no case reaches: {missing}"
    assert (cg.CLS_FUSED, "fused") in seen, "route 15 (class-fused) is not run"
    for dtype in cg.DTYPES:
        for cls in ("one-slab", "multi-tile", "prereduce"):
            assert (dtype, cls) in seen_wgrad, f"no {dtype} weight gradient of class {cls}"


# ----------------------------------------------------------------------------- without a GPU
def test_case_table_reaches_every_config_and_class_on_the_cpu():
    """The plan assertions and the coverage set of the whole case table, from the host-only planners."""
    before = cg.current_options(cg.GEOMETRY_KEYS + (6, 9, 10))
    from multimodal_tta_amd import ops
    tuned_for = ops._TUNED_FOR
    table = _plan_table()
    seen = {(config, cls) for (_, _, config, cls) in table.values() if cls is not None}
    seen_wgrad = set()
    for c in cg.CASES:
        for dtype in cg.DTYPES:
            for geo in cg.GEOMETRIES:
                seen_wgrad |= {(dtype, cls) for (_, cls) in _wgrad_classes(c, dtype, geo).values() if cls}
    fused = [cg.planned(cg.CLS_FUSED_CASE, "bf16", "inflight24", "fwd", stored) for stored in (False, True)]
    assert all(p[2] == cg.CLS_FUSED and p[1] == 1 for p in fused), f"class-fused case plans {fused}"
    seen.add((cg.CLS_FUSED, "fused"))
    _assert_complete(seen, seen_wgrad)
    # the cases the issue names: a short last split per operand type, the partly idle last column group, > 32 slabs
    for dtype in cg.DTYPES:
        assert table[("s1_160_64", dtype, "deep", "fwd", False)][1] == 3      # 10 / 5 stages in splits of 4 / 2
        assert table[("s1_128_136", dtype, "deep", "fwd", False)][1] == 3     # 136 produced channels; 16 / 8 stages in splits of 6 / 3
        with cg.pinned(cg.geometry_values("inflight1")):
            assert cg.ask_wgrad_plan(cg.CASES_BY_NAME["s1_32_32_slabs"], dtype)[1] > 0
    # every config meets odd extents and two batch items
    for want, holds in (("odd extents", lambda c: any(v % 2 for v in c.shape[1:])), ("batch 2", lambda c: c.shape[0] == 2)):
        got = {config for (name, *_), (vals, _, config, cls) in table.items() if vals is not None and holds(cg.CASES_BY_NAME[name])}
        lacking = [cfg for cfg in cg.IGEMM_CONFIGS if cfg not in got]
        assert not lacking, f"{want}: configs {lacking}"
    assert cg.current_options(cg.GEOMETRY_KEYS + (6, 9, 10)) == before and ops._TUNED_FOR == tuned_for


def test_norm_on_load_operands_stay_inside_the_cap():
    """At most 1 in 1000 elements of a bf16 norm-on-load operand may depend on how the fp32 transform is rounded."""
    for c in cg.CASES + [cg.CLS_FUSED_CASE]:
        share = cg.nl_operand_mismatch(c)
        assert share <= 1e-3, f"{c.name}: {share:.2e} of the operand elements differ"


# ----------------------------------------------------------------------------- on the GPU
def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous().cpu()


def _nl(mu, sc, sh):
    from multimodal_tta_amd import ops
    sc = sc.cuda()
    return ops.NL(mu.cuda(), sc, relu=True, scale=sc, shift=sh.cuda())          # (the kernels read the precombined pair)


def _make_op(c, dtype):
    from multimodal_tta_amd import ops
    op = ops.ConvOp(c.cin, c.cout, c.k, c.stride, c.transposed, "cuda", dtype=ops.BF16 if dtype == "bf16" else ops.F32)
    op.pack(cg.operands(c, dtype).w.cuda().contiguous())
    return op


def _new_y(c, stored_bf16):
    from multimodal_tta_amd import ops
    n = c.shape[0]
    if stored_bf16:
        return ops.new_cl(n, *cg.out_dhw(c), c.cout, "cuda", ldc=ops.row_pad(c.cout, torch.bfloat16), dtype=torch.bfloat16)
    return ops.new_cl(n, *cg.out_dhw(c), c.cout, "cuda")


def _checked_plan(op, desc, x, y, want, what):
    p = op.plan(desc, x, y)
    assert (int(p.ksplit), int(p.config)) == want, f"{what}: the launch plans {(int(p.ksplit), int(p.config))}, the table {want}"


def _forward_set(c, dtype, geo, op, stored, plan, outs):
    """Every forward form at one storage type, under the geometry of the forward call."""
    o, r = cg.operands(c, dtype), cg.reference(c, dtype)
    vals, ksplit, config, cls = plan
    tag = "bf16-stored" if stored else "fp32-stored"
    put = cl_bf16 if stored else cl
    bias = o.b.cuda()
    with cg.pinned(vals):
        x_cl, y = put(o.x), _new_y(c, stored)
        _checked_plan(op, op.d_fwd, x_cl, y, (ksplit, config), f"{c.name} {dtype} {geo} forward {tag}")
        stats = torch.full((op.stats_rows(x_cl, y), 2, c.cout), float("nan"), device="cuda")
        op.forward(x_cl, None, bias, y, stats=stats)
        outs[f"forward + bias, {tag}"] = (y, r.y, stored, stats)
        ya = put(o.y0)
        op.forward(x_cl, None, bias, ya, accumulate=True)
        outs[f"forward accumulate, {tag}"] = (ya, o.y0.double() + r.y, stored, None)
        # norm-on-load of x (bf16 operands: of a bf16-stored x) + a fused residual add under its own ReLU norm-on-load
        if stored or dtype == "fp32":
            y2 = _new_y(c, stored)
            stats2 = torch.full((op.stats_rows(x_cl, y2), 2, c.cout), float("nan"), device="cuda")
            op.forward(x_cl, _nl(o.mu, o.sc, o.sh), bias, y2, stats=stats2, add=put(o.res), add_nl=_nl(o.rmu, o.rsc, o.rsh))
            outs[f"forward norm-on-load + residual add, {tag}"] = (y2, r.y_nl + r.rin, stored, stats2)
    torch.cuda.synchronize()
    return config, cls


def _dgrad_set(c, dtype, geo, op, plan, outs):
    o, r = cg.operands(c, dtype), cg.reference(c, dtype)
    vals, ksplit, config, cls = plan
    n, d, h, w = c.shape
    from multimodal_tta_amd import ops
    with cg.pinned(vals):
        gy_cl, dx = cl(o.gy), ops.new_cl(n, d, h, w, c.cin, "cuda")
        _checked_plan(op, op.d_dgrad, gy_cl, dx, (ksplit, config), f"{c.name} {dtype} {geo} input gradient")
        op.dgrad(gy_cl, dx)
        outs["input gradient"] = (dx, r.dx, False, None)
        dxa = cl(o.dx0)
        op.dgrad(gy_cl, dxa, accumulate=True)
        outs["input gradient accumulate"] = (dxa, o.dx0.double() + r.dx, False, None)
    torch.cuda.synchronize()
    return config, cls


def _wgrad_set(c, dtype, geo, op, outs):
    o, r = cg.operands(c, dtype), cg.reference(c, dtype)
    classes = _wgrad_classes(c, dtype, geo)
    gy_cl = cl(o.gy)
    nl_bf16 = dtype == "bf16"                     # the norm-on-load check of bf16 operands reads a bf16-stored x
    with cg.pinned(cg.geometry_values(geo)):
        x_cl = cl(o.x)
        got = op.wgrad_plan(x_cl, gy_cl)
        assert [got["nsl"], got["pre_chunks"]] == classes[False][0][:2], f"{c.name} {dtype} {geo}: weight-gradient plan {got}"
        dw, db = torch.empty(cg.weight_shape(c), device="cuda"), torch.empty(c.cout, device="cuda")
        op.wgrad(x_cl, None, gy_cl, dw, db)
        outs["weight gradient"] = (dw, r.dw, False, None)
        outs["bias gradient"] = (db, r.db, False, None)
        dwa, dba = o.dw0.cuda(), o.db0.cuda()
        op.wgrad(x_cl, None, gy_cl, dwa, dba, accumulate=True)
        outs["weight gradient accumulate"] = (dwa, o.dw0.double() + r.dw, False, None)
        outs["bias gradient accumulate"] = (dba, o.db0.double() + r.db, False, None)
        xs = cl_bf16(o.x) if nl_bf16 else x_cl
        got = op.wgrad_plan(xs, gy_cl)
        assert [got["nsl"], got["pre_chunks"]] == classes[nl_bf16][0][:2], f"{c.name} {dtype} {geo}: weight-gradient plan {got}"
        dwn = torch.empty(cg.weight_shape(c), device="cuda")
        op.wgrad(xs, _nl(o.mu, o.sc, o.sh), gy_cl, dwn, None)
        outs["weight gradient, norm-on-load of x"] = (dwn, r.dw_nl, False, None)
    torch.cuda.synchronize()
    return {(dtype, cls) for (_, cls) in classes.values() if cls}


def _launch_all(c, dtype, geo, table, extra=None):
    """Every check of one case under one geometry: {name: (result, float64 reference, bf16-stored, statistics rows)}, the
    (config, class) pairs of its implicit-GEMM launches and the classes of its weight-gradient launches."""
    outs, seen, seen_wgrad = {}, set(), set()
    with cg.pinned({**cg.case_options(c), **(extra or {})}):
        op = _make_op(c, dtype)
        for stored in _storages(dtype):
            plan = table[(c.name, dtype, geo, "fwd", stored)]
            if plan[0] is not None:
                seen.add(_forward_set(c, dtype, geo, op, stored, plan, outs))
        plan = table[(c.name, dtype, geo, "dgrad", False)]
        if plan[0] is not None:
            seen.add(_dgrad_set(c, dtype, geo, op, plan, outs))
        seen_wgrad = _wgrad_set(c, dtype, geo, op, outs)
    return outs, seen, seen_wgrad


def _check_all(c, dtype, geo, outs):
    n = c.shape[0]
    for name, (got, ref, stored, stats) in outs.items():
        what = f"{c.name} {geo}: {name}"
        host = got.cpu() if got.dim() != 5 or name.startswith("weight") else _ncdhw(got)
        cg.exact_close(what, dtype, host, ref, stored)
        if stats is not None:
            cg.stats_close(what, stats, n, ref)


@GPU
@pytest.mark.parametrize("c,dtype,geo", _params())
def test_conv_parity_at_geometry(c, dtype, geo):
    """Forward (bias + statistics; norm-on-load + fused residual add + statistics; accumulate; fp32- and bf16-stored for bf16
    operands), input gradient (plain, accumulate) and weight / bias gradient (plain, accumulate, norm-on-load of x) of one case
    under one launch geometry, against the exact-operand float64 reference."""
    before = cg.current_options(cg.GEOMETRY_KEYS + (6, 9, 10))
    table = _plan_table([c])
    outs, seen, seen_wgrad = _launch_all(c, dtype, geo, table)
    _check_all(c, dtype, geo, outs)
    if dtype == "bf16" and c.k == 3 and c.stride == 1 and not c.transposed and geo in ("unsplit", "deep"):
        # the row loader's prefetch crosses stages here: both settings of MMTTA_OPT_IGEMM_PIPELINE, bit for bit
        cross = {mode: _launch_all(c, dtype, geo, table, {6: mode})[0] for mode in (0, 1)}
        for name in outs:
            if name.startswith(("forward", "input gradient")):
                assert torch.equal(cross[0][name][0], cross[1][name][0]), f"{c.name} {geo}: {name} differs between the loaders"
                if cross[0][name][3] is not None:
                    assert torch.equal(cross[0][name][3], cross[1][name][3]), f"{c.name} {geo}: {name}: statistics rows differ"
    SEEN.update(p for p in seen if p[1] is not None)
    SEEN_WGRAD.update(seen_wgrad)
    RAN.add((c.name, dtype, geo))
    assert cg.current_options(cg.GEOMETRY_KEYS + (6, 9, 10)) == before


@GPU
@pytest.mark.parametrize("stored", [False, True], ids=["fp32-stored", "bf16-stored"])
def test_class_fused_route_at_the_benchmark_geometry(stored):
    """Route 15 never splits: its smallest admissible shape under inflight24, every forward form."""
    c, dtype, geo = cg.CLS_FUSED_CASE, "bf16", "inflight24"
    plan = cg.planned(c, dtype, geo, "fwd", stored)
    assert plan[1:3] == (1, cg.CLS_FUSED), f"planned {plan}"
    outs = {}
    config, _ = _forward_set(c, dtype, geo, _make_op(c, dtype), stored, plan, outs)
    _check_all(c, dtype, geo, outs)
    SEEN.add((config, "fused"))


@GPU
@pytest.mark.parametrize("dtype", cg.DTYPES)
@pytest.mark.parametrize("name", ["s1_160_64", "s2_96_32"])
def test_epilogue_store_width_at_unsplit(name, dtype):
    """MMTTA_OPT_EPILOGUE_VEC16 0 / 1 after a multi-stage K loop in one workgroup, every epilogue form (bias + statistics,
    residual add under norm-on-load, accumulate; fp32- and bf16-stored): equal outputs bit for bit, statistics within
    summation order of the float64 sums."""
    c = cg.CASES_BY_NAME[name]
    table = _plan_table([c])
    res = {}
    for mode in (0, 1):
        with cg.pinned({9: mode}):
            plans = {k: (v[0],) + cg.planned(c, dtype, "unsplit", k[3], k[4])[1:] for k, v in table.items() if k[1:3] == (dtype, "unsplit")}
            assert all(p[1] == 1 for p in plans.values())
            res[mode] = _launch_all(c, dtype, "unsplit", plans, {9: mode})[0]
            _check_all(c, dtype, "unsplit", res[mode])
    for key in res[0]:
        assert torch.equal(res[0][key][0], res[1][key][0]), f"{name} {dtype}: {key} differs between the store widths"


# wgrad_f32_kernel<TZ, TY, TX, NTW, GBF, DBF> reads either operand fp32- or bf16-stored; the cases above launch it next to an
# fp32-stored dy only.  The storage pairs with a bf16-stored dy, per tile: fp32 precision on bf16-representable
# operands, so what the kernel unpacks is what the float64 reference multiplies.
F32_WGRAD_STORAGE = [(cg.case("f32_k1_40_32", 40, 32, 1, 1, False, (2, 6, 10, 12)), False), (cg.case("f32_k1_32_64", 32, 64, 1, 1, False, (2, 6, 10, 12)), True),
                     (cg.case("f32_s1_32_40", 32, 40, 3, 1, False, (2, 6, 10, 12)), False), (cg.case("f32_s1_40_32", 40, 32, 3, 1, False, (2, 6, 10, 12)), True),
                     (cg.case("f32_s2_32_64", 32, 64, 3, 2, False, (2, 7, 11, 13)), True)]


@GPU
@pytest.mark.parametrize("c,x_bf16", F32_WGRAD_STORAGE, ids=[f"{c.name}-x_{'bf16' if b else 'fp32'}" for c, b in F32_WGRAD_STORAGE])
def test_fp32_operand_wgrad_reads_a_bf16_stored_gradient(c, x_bf16):
    """Weight and bias gradient, plain and accumulating, of the fp32-operand kernel with dy bf16-stored (and x either way),
    against the float64 reference: the kernel id is asserted before the launch."""
    from multimodal_tta_amd import _lib, ops
    o, r = cg.operands(c, "bf16"), cg.reference(c, "bf16")
    op = _make_op(c, "fp32")
    x_cl, gy_cl = (cl_bf16 if x_bf16 else cl)(o.x), cl_bf16(o.gy)
    kid = int(_lib.load().mmtta_conv_wgrad_kernel(C.byref(op.d_fwd), C.byref(ops.desc_cl(x_cl)), C.byref(ops.desc_cl(gy_cl))))
    assert kid == (2 if c.k == 1 else 0 if c.stride == 1 else 1), f"{c.name}: weight-gradient kernel {kid}"
    dw, db = torch.full(cg.weight_shape(c), float("nan"), device="cuda"), torch.full((c.cout,), float("nan"), device="cuda")
    op.wgrad(x_cl, None, gy_cl, dw, db)
    dwa, dba = o.dw0.cuda(), o.db0.cuda()
    op.wgrad(x_cl, None, gy_cl, dwa, dba, accumulate=True)
    torch.cuda.synchronize()
    for what, got, ref in (("weight gradient", dw, r.dw), ("bias gradient", db, r.db),
                           ("weight gradient accumulate", dwa, o.dw0.double() + r.dw), ("bias gradient accumulate", dba, o.db0.double() + r.db)):
        cg.exact_close(f"{c.name} x {'bf16' if x_bf16 else 'fp32'}-stored, dy bf16-stored: {what}", "fp32", got.cpu(), ref)


@GPU
def test_every_config_ran_in_every_class():
    """Closes the module: the (config, class) pairs the launches above made.  A planner change that silently un-covers a
    kernel fails here.  (Needs the whole module to have run.)"""
    expected = {(c.name, dt, geo) for c in cg.CASES for dt in cg.DTYPES for geo in cg.GEOMETRIES}
    assert RAN == expected, f"this test closes a whole run of the module; not run: {sorted(expected - RAN)[:5]} ..."
    print("(config, class) pairs run:", sorted(SEEN))
    print("weight-gradient classes run:", sorted(SEEN_WGRAD))
    for dtype, (worst, what) in sorted(cg.WORST.items()):
        print(f"worst err / bound, {dtype} operands: {worst:.3e} ({what})")
    _assert_complete(SEEN, SEEN_WGRAD)
