"""Parity of the thin and pointwise convolution routes - route 6 (<= 4 produced channels), route 13 (<= 4 gathered channels),
routes 16 and 17 (1x1x1) and the weight-gradient kernels 3, 6, 9 and 10 - per kernel, against an exact-operand float64
reference (layers, layouts, forms and the reference: tests/thin_routes.py, on top of tests/conv_geometry.py).

Each test asks first, then launches.  mmtta_conv_route and mmtta_conv_thin_kernel (the function the launchers of routes 6 and
13 switch on) name the kernel of every call, mmtta_conv_wgrad_kernel and mmtta_conv_wgrad_plan_sets the weight gradient's; the
answer is asserted against the layer table for made-up descriptors (which is all the tests without the `gpu` mark need) and
again for the real tensors, whose descriptors must equal the made-up ones field by field.  A form a kernel does not take is
asserted as the other kernel, the other route or the error code the queries report, and an error is asserted of the run too.

The reference.  float64 torch F.conv3d / F.conv_transpose3d + autograd on the CPU, on the operand values the kernel sees.
Wherever the precision mode or a storage type is bf16, x, the weights, gy, the residual operand and the accumulate prefill
are bf16-representable, so bf16 x bf16 products are exact in fp32 (the gather-GEMM image of the up-convolution regroups taps
and sums none) and only the accumulation order differs:

    fp32-stored results    |got - ref| <= 2e-4 * max|ref| + 1e-5
    bf16-stored results    |got - ref| <= 2^-8 * |ref| + 2e-4 * max|ref| + 1e-5    element by element

Statistics rows go through conv_geometry.stats_close.  No check here uses the 1.5e-2 bf16-operand bound or another kernel.

Norm-on-load.  relu(fmaf(x, scale, shift)) in float64, rounded to fp32 once; the kernels that feed the matrix cores
(conv3_mfma4, upconv8, chan_mfma, route 17, the bf16-operand weight gradients) round that to bf16, and so does their reference;
the vector-ALU kernels (direct, lanes along K, row, up-convolution, head, direct_chan) compute on the fp32 value, and their
reference keeps it - also where the precision mode is bf16 and only the storage rounds.  The LeakyReLU form (slope 2^-3, exact
in fp32) runs the second translation unit's instantiations, one layer per kernel that has them.

Not modelled, because nothing needed it: no kernel of this module rounds an intermediate the reference does not.

Observed worst err / bound per kernel on an MI355X and the run time of this file: DESIGN.md, "Thin and pointwise convolution
parity per kernel" (recorded values, not limits).
"""
import ctypes as C

import pytest
import torch

import conv_geometry as cg
import thin_routes as tr

GPU = pytest.mark.gpu
RAN = {}            # kernel key (1..13, 16, 17) -> [(layer, call)] of every launch the GPU tests made
RAN_WGRAD = set()   # (kernel id, class) of every weight-gradient launch
RAN_LAYERS = set()
THIN_IDS = tuple(k for k in tr.THIN_KERNELS if k not in tr.UNREACHABLE) + (tr.ROUTE_PW_SMALL, tr.ROUTE_PW_MFMA)
FORWARD_LAYERS = [l for l in tr.LAYERS if any(w is not None and w > 0 for w in l.fwd)]


def _name(key):
    return tr.THIN_KERNELS.get(key, f"route {key}")


# ----------------------------------------------------------------------------- coverage of a table of (kernel, call) pairs
def _read_channels(call):
    c = call.layer.case
    return c.cin if call.orientation == "fwd" else c.cout


def _produced_channels(call):
    c = call.layer.case
    return c.cout if call.orientation == "fwd" else c.cin


def _op(call):
    t = call.layer.case.transposed
    return {("fwd", False): "CONV_FWD", ("fwd", True): "CONVT_FWD", ("dgrad", False): "CONV_DGRAD", ("dgrad", True): "CONVT_DGRAD"}[(call.orientation, t)]


def _layouts(call):
    l = call.layer
    return (l.lo, l.hi) if call.orientation == "fwd" else (l.hi, l.lo)


def _assert_complete(reached, wgrad_reached):
    """reached: {kernel key: [call]}; wgrad_reached: {(kernel id, class or None)}."""
    missing = [_name(k) for k in THIN_IDS if not reached.get(k)]
    assert not missing, f"kernels no call reaches: {missing}"
    assert not any(reached.get(k) for k in tr.UNREACHABLE), "a kernel listed as unreachable is reached: take it off the list"
    every = [(k, c) for k, cs in reached.items() for c in cs]
    have = lambda keys, pred: any(k in keys and pred(c) for k, c in every)

    def need(what, keys, pred):
        assert have(keys, pred), f"no call of {[_name(k) for k in keys]} with {what}"

    for k in THIN_IDS:
        need("two batch items", (k,), lambda c: c.layer.case.shape[0] == 2)
        need("odd extents", (k,), lambda c: any(v % 2 for v in c.layer.case.shape[1:]))
    for ch in (1, 2, 3, 4):
        need(f"{ch} gathered channels", (3, 4, 5, 11, 12, 13, 16), lambda c: _read_channels(c) == ch)
        need(f"{ch} produced channels", (1, 2, 3, 4, 5, 6, 8, 9, 10), lambda c: _produced_channels(c) == ch)
    for n in (32, 64):
        need(f"{n} produced channels", (11, 12, 13), lambda c: _produced_channels(c) == n)
        for k in (2, 6, 8, 9, 10):
            need(f"a reduction over {n} channels", (k,), lambda c: _read_channels(c) == n)
    for s in (1, 2):
        need(f"stride {s}", (11, 12), lambda c: c.layer.case.stride == s and c.orientation == "fwd")
        need(f"stride {s}", (1,), lambda c: c.layer.case.stride == s)
    for op in ("CONV_FWD", "CONVT_FWD", "CONV_DGRAD", "CONVT_DGRAD"):
        need(op, THIN_IDS, lambda c: _op(c) == op)
    need("the 64-column input gradient of a 64 -> 3 transposed convolution", (12,), lambda c: _op(c) == "CONVT_DGRAD" and _produced_channels(c) == 64)
    need("the 64-column input gradient of a 64 -> 3 transposed convolution", (13,), lambda c: _op(c) == "CONVT_DGRAD" and _produced_channels(c) == 64)
    # storages: x fp32- and bf16-stored (8-byte voxels on the thin side), y fp32- and bf16-stored where the kernel admits it
    for k in (12, 13, 5):
        need("a bf16-stored x of 8-byte voxels", (k,), lambda c: _layouts(c)[0] == tr.B and _read_channels(c) <= 4)
    for k in (2, 8, 10):
        need("a bf16-stored x", (k,), lambda c: _layouts(c)[0] == tr.B)
        need("an fp32-stored x", (k,), lambda c: _layouts(c)[0] == tr.F)
    for k in (12, tr.ROUTE_PW_SMALL):
        need("a bf16-stored y", (k,), lambda c: _layouts(c)[1] == tr.B)
        need("an fp32-stored y", (k,), lambda c: _layouts(c)[1] == tr.F)
    need("a one-channel slice inside a 16-byte group", (11,), lambda c: _layouts(c)[0] == tr.S)
    # with and without a norm-on-load transform (the lean up-convolution, the head and routes 16 / 17 take none)
    for k in (1, 2, 3, 4, 6, 8, 11, 12, 13):
        need("a norm-on-load of x", (k,), lambda c: c.x_nl is not None)
        need("no norm-on-load", (k,), lambda c: c.x_nl is None)
    for keys in ((1, 2, 3, 4, 6, 8), (11, 12)):
        need("a LeakyReLU norm-on-load", keys, lambda c: c.x_nl == "leaky")
    # MMTTA_OPT_THIN_MFMA: TZ = 8 / 4 / 2
    for v in (1, 2, 3):
        need(f"option 13 = {v}", (4,), lambda c: c.layer.opts.get(tr.OPT_THIN_MFMA) == v)
    need("more than 128 tiles per item", (8,), lambda c: c.layer.case.shape == (1, 20, 24, 40))
    need("more than 128 tiles per item", (9,), lambda c: c.layer.case.shape == (1, 20, 24, 40))
    for kid in tr.WGRAD_KERNELS:
        assert any(k == kid for k, _ in wgrad_reached), f"weight-gradient kernel {kid} is not reached"
    for kid in (3, 10):         # the thin family's slab plans
        for cls in ("one-slab", "multi-tile", "prereduce"):
            assert (kid, cls) in wgrad_reached, f"weight-gradient kernel {kid}: no launch of class {cls}"
    assert (9, "prereduce") in wgrad_reached      # (its slabs are not tuned: four per split, 1024 workgroups wanted)


# ----------------------------------------------------------------------------- without a GPU
def test_layer_table_reaches_every_kernel_on_the_cpu():
    """Every call of the table asks the host-only queries for made-up descriptors: the kernel ids the layers are there for,
    and the axis values the closing assertion wants."""
    from multimodal_tta_amd import ops
    before, tuned_for = cg.current_options(tr.OPTION_KEYS), ops._TUNED_FOR
    reached, wgrad_reached = {}, set()
    for l in tr.LAYERS:
        for call in tr.calls(l):
            got = tr.ask_call(call)
            assert got == call.want, f"{l.case.name}: {call.form}: the queries say {got}, the table {call.want}"
            if got is not None and got > 0:
                reached.setdefault(got, []).append(call)
        for tag, opts, want in (tr.wgrad_variants(l) if l.wgrad is not None else ()):
            for geo in tr.WGRAD_GEOMETRIES:
                kid, plan, cls = tr.ask_wgrad(l, opts, geo)
                assert kid == want, f"{l.case.name}{tag} {geo}: weight-gradient kernel {kid}, the table {want}"
                wgrad_reached.add((kid, cls))
    _assert_complete(reached, wgrad_reached)
    assert cg.current_options(tr.OPTION_KEYS) == before and ops._TUNED_FOR == tuned_for


def test_thin_kernel_query_follows_the_options_and_reports_errors():
    """The query is the launchers' own function: it moves with options 13 and 18, returns 0 off routes 6 and 13 and the
    run's error for operands a launcher refuses."""
    before = cg.current_options(tr.OPTION_KEYS)
    l = tr.LAYERS_BY_NAME["mfma4_4_2_tz8"]
    plain = tr.calls(l)[0]
    for option, want in ((0, 3), (1, 4), (2, 4), (3, 4)):
        with cg.pinned({tr.OPT_THIN_MFMA: option}):
            x, y, _ = tr.made_up_tensors(l, "fwd")
            assert tr.what_runs(tr.conv_desc(l, "fwd"), x, y, stats=None) == want
    l = tr.LAYERS_BY_NAME["chanm_3_32_s2_bf"]
    x, y, _ = tr.made_up_tensors(l, "fwd")
    for option, want in ((0, 12), (1, 13), (2, 12), (3, 13)):
        with cg.pinned({tr.OPT_THIN_LEAN: option}):
            assert tr.what_runs(tr.conv_desc(l, "fwd"), x, y) == want
    # a wide layer: an implicit GEMM, id 0; a bf16-stored result of the fp32 up-convolution: the launcher's error
    wide = tr.layer("wide", 32, 32, 3, 1, False, (1, 4, 4, 8), "fp32", tr.F, tr.F, fwd=())
    x, y, _ = tr.made_up_tensors(wide, "fwd")
    assert tr.what_runs(tr.conv_desc(wide, "fwd"), x, y) is None
    bad = tr.layer("bad", 32, 3, 3, 2, True, (1, 4, 4, 8), "fp32", tr.F, tr.B, fwd=())
    x, y, _ = tr.made_up_tensors(bad, "fwd")
    assert tr.what_runs(tr.conv_desc(bad, "fwd"), x, y) == tr.ERR_UNSUPPORTED
    assert plain.want == 4 and cg.current_options(tr.OPTION_KEYS) == before


def test_norm_on_load_operands_of_the_thin_layers_stay_inside_the_cap():
    """At most 1 in 1000 elements of a bf16 norm-on-load operand may depend on how the fp32 transform is rounded."""
    for l in tr.LAYERS:
        if tr.operand_type(l) == "bf16":
            share = tr.nl_operand_mismatch(l.case)
            print(f"{l.case.name}: share {share:.2e}")
            assert share <= 1e-3, f"{l.case.name}: {share:.2e} of the operand elements differ"


def test_the_exact_bound_sees_one_zeroed_weight():
    """Every forward layer: the float64 reference with the weight element of median magnitude zeroed leaves the exact bound at
    some voxel - no layer is so small or so scaled that it tests nothing.  Printed, not asserted: whether the change also
    leaves the bf16-operand bound 1.5e-2 * max|ref| the older tests of these kernels use."""
    import torch.nn.functional as F
    unseen_by_old = []
    for l in FORWARD_LAYERS:
        c, ot = l.case, tr.operand_type(l)
        o, r = tr.operands(c, ot), tr.reference(c, ot)
        flat = o.w.abs().flatten()
        idx = int(flat.argsort()[flat.numel() // 2])
        w = o.w.clone().double()
        w.view(-1)[idx] = 0.0
        pad = (c.k - 1) // 2
        if c.transposed:
            y = F.conv_transpose3d(o.x.double(), w, o.b.double(), stride=c.stride, padding=pad, output_padding=c.stride - 1)
        else:
            y = F.conv3d(o.x.double(), w, o.b.double(), stride=c.stride, padding=pad)
        stored = l.hi == tr.B
        bound = cg.TOL_REL * r.y.abs().max().item() + cg.TOL_ABS + (cg.BF16_STORE * r.y.abs() if stored else 0.0)
        change = (y - r.y).abs()
        ratio = (change / bound).max().item()
        old = change.max().item() / (1.5e-2 * r.y.abs().max().item())
        print(f"{c.name}: change / exact bound = {ratio:.1f}, change / (1.5e-2 max|ref|) = {old:.2f}{'' if old > 1 else '  (unseen by the old bound)'}")
        if old <= 1:
            unseen_by_old.append(c.name)
        assert ratio > 1.0, f"{c.name}: a zeroed weight of median size moves no voxel past the exact bound ({ratio:.2f})"
    print(f"unseen by the 1.5e-2 bound: {len(unseen_by_old)} of {len(FORWARD_LAYERS)} layers: {unseen_by_old}")


# ----------------------------------------------------------------------------- on the GPU
def _sync():
    """Wait for the launches; a fault of the device ends the run of the suite here: nothing more is launched on it."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported a fault, nothing more is launched: {e}", returncode=3)


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).float().cpu()


def _nl(mu, sc, sh, kind):
    from multimodal_tta_amd import ops
    mu, sc, sh = mu.cuda(), sc.cuda(), sh.cuda()
    if kind == "leaky":
        return ops.NL(mu, sc, scale=sc, shift=sh, act=ops.ACT_LEAKY_RELU, negative_slope=tr.LEAKY_SLOPE)
    return ops.NL(mu, sc, relu=True, scale=sc, shift=sh)


def _make_op(l):
    from multimodal_tta_amd import ops
    c = l.case
    op = ops.ConvOp(c.cin, c.cout, c.k, c.stride, c.transposed, "cuda", dtype=ops.BF16 if l.dtype == "bf16" else ops.F32)
    op.pack(tr.operands(c, tr.operand_type(l)).w.cuda().contiguous())
    return op


def _input(layout, t):
    """A tensor a kernel reads: the pad lanes of a bf16-stored thin one hold 3."""
    return tr.build(layout, t, tr.PAD if layout == tr.B and t.shape[1] < 4 else 0.0)


def _run_call(l, op, call):
    """Ask, compare with the table, launch, compare with the reference.  Returns the kernel key or None."""
    from multimodal_tta_amd import ops
    c, ot = l.case, tr.operand_type(l)
    o = tr.operands(c, ot)
    what = f"{c.name}: {call.form}"
    assert tr.ask_call(call) == call.want, f"{what}: the table"
    nan = float("nan")
    if call.orientation == "fwd":
        x = _input(l.lo, o.x)
        y = tr.build(l.hi, o.y0 if call.accumulate else torch.full_like(o.y0, nan), 0.0 if call.accumulate else nan)
        add = _input(l.hi, o.res) if call.add else None
        desc, packed, bias = op.d_fwd, op.packed_fwd, o.b.cuda()
        x_nl = _nl(o.mu, o.sc, o.sh, call.x_nl) if call.x_nl else None
        add_nl = _nl(o.rmu, o.rsc, o.rsh, "relu") if call.add else None
    else:
        x = _input(l.hi, o.gy)
        dx0 = tr.q_bf16(o.dx0) if l.lo == tr.B else o.dx0
        y = tr.build(l.lo, dx0 if call.accumulate else torch.full_like(dx0, nan), 0.0 if call.accumulate else nan)
        add, desc, packed, bias, x_nl, add_nl = None, op.d_dgrad, op.packed_dgrad, None, None, None
    fx, fy, fadd = tr.made_up_tensors(l, call.orientation)
    dx_, dy_ = ops.desc_cl(x), ops.desc_cl(y)
    assert tr.same_descriptor(dx_, fx) and tr.same_descriptor(dy_, fy), f"{what}: the tensors differ from the made-up descriptors"
    dadd = ops.desc_cl(add) if add is not None else None
    assert dadd is None or tr.same_descriptor(dadd, fadd), f"{what}: the fused add differs from its made-up descriptor"
    stats = None
    if call.stats and call.want is not None and call.want > 0:
        stats = torch.full((op.stats_rows(x, y), 2, y.shape[-1]), nan, device="cuda")
    stats_arg = ops.ptr(stats) if stats is not None else (tr._HOST_COEFFS.data_ptr() if call.stats else None)
    got = tr.what_runs(desc, dx_, dy_, x_nl.struct() if x_nl else None, dadd, add_nl.struct() if add_nl else None,
                       1 if call.accumulate else 0, stats_arg)
    assert got == call.want, f"{what}: the queries say {got} for the real tensors, the table {call.want}"
    if got is None:
        return None                     # another route: not this module's
    if got < 0:
        with pytest.raises(ops.MmttaError, match=f"status {got}"):
            op._run(desc, packed, x, x_nl, bias, y, call.accumulate, None, add, add_nl)
        return None
    op._run(desc, packed, x, x_nl, bias, y, call.accumulate, stats, add, add_nl)
    _sync()
    ref, stats_ref = tr.expected(call, got)
    stored = y.dtype == torch.bfloat16
    ratio = tr.exact_close(f"{what} [{_name(got)}]", ot, _ncdhw(y), ref, stored)
    tr.note_worst(_name(got), ratio, what)
    if stats is not None:
        tr.stats_close(what, stats, c.shape[0], stats_ref)
    RAN.setdefault(got, []).append(call)
    return got


@GPU
@pytest.mark.parametrize("name", [l.case.name for l in tr.LAYERS if tr.calls(l)])
def test_thin_route_parity(name):
    """Every form of one layer - forward with bias; with bias and statistics rows; norm-on-load of x plus a fused add under its
    own ReLU norm-on-load, with statistics; accumulate onto a prefilled result; the LeakyReLU form; the input gradient, plain and
    accumulating - against the exact-operand float64 reference, each after the queries named its kernel."""
    from multimodal_tta_amd import ops
    l = tr.LAYERS_BY_NAME[name]
    before, tuned_for = cg.current_options(tr.OPTION_KEYS), ops._TUNED_FOR
    with cg.pinned(l.opts):
        op = _make_op(l)
        for call in tr.calls(l):
            _run_call(l, op, call)
    RAN_LAYERS.add(name)
    assert cg.current_options(tr.OPTION_KEYS) == before and ops._TUNED_FOR == tuned_for


@GPU
@pytest.mark.parametrize("name", [l.case.name for l in tr.wgrad_layers()])
def test_thin_weight_gradient_parity(name):
    """Weight and bias gradient of one layer - plain, accumulating, with a norm-on-load of x - under the geometries `unsplit`,
    `deep` and `inflight1`, against the float64 reference; the kernel id and the slab plan are asserted before each launch."""
    from multimodal_tta_amd import _lib, ops
    l = tr.LAYERS_BY_NAME[name]
    c, ot = l.case, tr.operand_type(l)
    o, r = tr.operands(c, ot), tr.reference(c, ot)
    before, tuned_for = cg.current_options(tr.OPTION_KEYS), ops._TUNED_FOR
    for tag, opts, want in tr.wgrad_variants(l):
        rounded = l.dtype == "bf16" and want in (3, 9, 10)
        dw_nl = tr.nl_reference(c, ot, rounded, "relu").dw
        for geo in tr.WGRAD_GEOMETRIES:
            kid, plan, cls = tr.ask_wgrad(l, opts, geo)
            assert kid == want, f"{name}{tag} {geo}: the table"
            with cg.pinned(opts), cg.pinned(cg.geometry_values(geo)):
                op = _make_op(l)
                x, gy = _input(l.lo, o.x), _input(l.hi, o.gy)
                fx, fdy, _ = tr.made_up_tensors(l, "fwd")
                tx, tdy = ops.desc_cl(x), ops.desc_cl(gy)
                assert tr.same_descriptor(tx, fx) and tr.same_descriptor(tdy, fdy)
                got = int(_lib.load().mmtta_conv_wgrad_kernel(C.byref(op.d_fwd), C.byref(tx), C.byref(tdy)))
                assert got == want, f"{name}{tag} {geo}: mmtta_conv_wgrad_kernel says {got}"
                real = op.wgrad_plan(x, gy)
                assert [real["nsl"], real["pre_chunks"]] == plan[:2], f"{name}{tag} {geo}: plan {real}, asked {plan}"
                nan = float("nan")
                dw, db = torch.full(cg.weight_shape(c), nan, device="cuda"), torch.full((c.cout,), nan, device="cuda")
                op.wgrad(x, None, gy, dw, db)
                dwa, dba = o.dw0.cuda(), o.db0.cuda()
                op.wgrad(x, None, gy, dwa, dba, accumulate=True)
                dwn = torch.full(cg.weight_shape(c), nan, device="cuda")
                op.wgrad(x, _nl(o.mu, o.sc, o.sh, "relu"), gy, dwn, None)
            _sync()
            kname = tr.WGRAD_KERNELS[want] + tag
            for form, got_t, ref in (("weight gradient", dw, r.dw), ("bias gradient", db, r.db),
                                     ("weight gradient accumulate", dwa, o.dw0.double() + r.dw),
                                     ("bias gradient accumulate", dba, o.db0.double() + r.db),
                                     ("weight gradient, norm-on-load of x", dwn, dw_nl)):
                what = f"{name} {geo}: {form}"
                tr.note_worst(kname, tr.exact_close(f"{what} [{kname}]", ot, got_t.cpu(), ref), what)
            RAN_WGRAD.add((want, cls))
    RAN_LAYERS.add("wgrad " + name)
    assert cg.current_options(tr.OPTION_KEYS) == before and ops._TUNED_FOR == tuned_for


@GPU
def test_every_thin_kernel_ran():
    """Closes the module: what actually ran covers what the CPU test says the table reaches, and every comparison stayed
    inside the exact bound.  (Needs the whole module to have run.)"""
    expected = {l.case.name for l in tr.LAYERS if tr.calls(l)} | {"wgrad " + l.case.name for l in tr.wgrad_layers()}
    assert RAN_LAYERS == expected, f"this test closes a whole run of the module; not run: {sorted(expected - RAN_LAYERS)[:5]} ..."
    for kname, (worst, what) in sorted(tr.WORST.items()):
        print(f"worst err / bound, {kname}: {worst:.3e} ({what})")
        assert worst <= 1.0
    print("weight-gradient (kernel, class) pairs run:", sorted(RAN_WGRAD, key=str))
    _assert_complete(RAN, RAN_WGRAD)
