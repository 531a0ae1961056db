"""Every dispatch class of csrc/pointwise.hip against a float64 reference on exactly the operands the kernel sees, with
derived per-element bounds (tests/pointwise_classes.py holds the case table, the references and the bounds; DESIGN.md,
"Pointwise parity per dispatch class", the rules and the figures measured on an MI355X).

Each test asks mmtta_pointwise_route first and fails if the case no longer reaches the class it is there for, fills every
output buffer with NaN, launches, and checks every output element (every partial row and every (item, channel) for the sums)
against its bound, and that no byte outside the written view changed: row pads the view does not own, the neighbouring
channels / voxels of a slice, `part` rows behind N * rows.  The last test prints the worst err / bound per family.
"""
import numpy as np
import pytest
import torch

import pointwise_classes as pc
from multimodal_tta_amd import ops

pytestmark = pytest.mark.gpu
WORST = {}


def _ids(cases):
    return [c.name for c in cases]


def _route(case, views, nl=None, nl2=None, m1=None, m2=None):
    route = ops.pointwise_route(pc.ROUTE_OP[case.op], views, nl, nl2, m1, m2)
    pc.check_route(case, route)
    assert pc.klass(route) == pc.klass(pc.host_route(case)), f"{case.name}: device tensors and made-up descriptors disagree"
    return route


def _dev(case, who, values=None):
    """(buffer, view) of operand `who` on the GPU: NaN everywhere, `values` in the view."""
    shape, lay, bf = pc.operand_shape(case, who), case.lay(who), pc.operand_bf(case, who)
    n, c, d, h, w = shape
    ldc, wb = lay.geometry(shape)
    buf = torch.full((n, d, h, wb, ldc), float("nan"), dtype=torch.bfloat16 if bf else torch.float32, device="cuda")
    view = buf[lay.index(shape)]
    if values is not None:
        view.copy_(torch.from_numpy(values).to(buf.dtype))
    if lay.own:
        view._mmtta_owns_pad = True
    return buf, view


def _f32(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).float().cuda()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _untouched(case, who, before, after):
    keep = ~torch.from_numpy(pc.owned_mask(pc.operand_shape(case, who), case.lay(who))).cuda()
    assert torch.equal(_bits(before)[keep], _bits(after)[keep]), f"{case.name}: bytes outside the view of `{who}` changed"


def _judge(case, family, what, got, ref, bound, leave_out=None):
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.broadcast_to(bound, np.shape(ref))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    ok = err <= bound                                   # NaN (an unwritten element) compares false
    if leave_out is not None:
        ok = ok | (leave_out & np.isfinite(got))
        err = np.where(leave_out, 0.0, err)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio if np.isfinite(ratio) else float("inf"))
    print(f"{case.name} {what}: worst err / bound = {ratio:.3f}")
    if not ok.all():
        i = np.unravel_index(np.argmax(~ok), ok.shape)
        pytest.fail(f"{case.name} {what}: {int((~ok).sum())} of {ok.size} elements outside their bound, first at {i}: got {got[i]!r}, "
                    f"reference {ref[i]!r}, bound {bound[i]:.3e}")


def _nl(case, o, coeff=None):
    mean, rstd, gamma, beta = coeff if coeff is not None else (o["mean"], o["rstd"], o["gamma"], o["beta"])
    act = case.act if coeff is None or coeff is o.get("ca") else case.kw["act_b"]
    t = [_f32(v.reshape(-1)) if v is not None else None for v in (mean, rstd, gamma, beta)]
    return ops.NL(t[0], t[1], t[2], t[3], relu=False, per_item=bool(case.kw.get("per_item")) and gamma is not None,
                  act=pc.ACT_CODE[act], negative_slope=pc.SLOPE)


def _part(case, route):
    n, c = case.shape[:2]
    used = n * route["rows_per_n"] * 2 * c
    return torch.full((used + 4 * c,), float("nan"), device="cuda"), used


def _check_sums(case, o, route, part, used, family):
    n, c = case.shape[:2]
    torch.cuda.synchronize()
    assert bool(torch.isnan(part[used:]).all()), f"{case.name}: `part` rows behind N * rows were written"
    got = part[:used].view(n, route["rows_per_n"], 2, c).double().cpu().numpy()
    ref = pc.ref_sums(case, o, route)
    for k, name in enumerate(("s0", "s1")):
        _judge(case, family, f"{name} per row", got[:, :, k], ref[name][0], ref[name][1])
        _judge(case, family, f"{name} per (item, channel)", got[:, :, k].sum(1), ref[name][0].sum(1), ref[name][1].sum(1))


# ----------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("case", pc.cases_of("stats"), ids=_ids(pc.cases_of("stats")))
def test_channel_stats(case):
    o = pc.make(case)
    xb, xv = _dev(case, "x", o["x"])
    route = _route(case, [xv])
    part, used = _part(case, route)
    before = xb.clone()
    ops.channel_stats(xv, part)
    _check_sums(case, o, route, part, used, route["family"])
    assert torch.equal(_bits(before), _bits(xb))


@pytest.mark.parametrize("case", pc.cases_of("bwd_reduce"), ids=_ids(pc.cases_of("bwd_reduce")))
def test_norm_bwd_reduce(case):
    o = pc.make(case)
    (db, dv), (yb, yv) = _dev(case, "dout", o["dout"]), _dev(case, "y", o["y"])
    nl = _nl(case, o)
    route = _route(case, [dv, yv], nl)
    part, used = _part(case, route)
    ops.norm_bwd_reduce(dv, yv, nl, part)
    _check_sums(case, o, route, part, used, route["family"])


@pytest.mark.parametrize("case", pc.cases_of("stats_chain"), ids=_ids(pc.cases_of("stats_chain")))
def test_stats_then_finalize(case):
    o = pc.make(case)
    n, c, d, h, w = case.shape
    xb, xv = _dev(case, "x", o["x"])
    route = _route(case, [xv])
    part, used = _part(case, route)
    ops.channel_stats(xv, part)
    nan = lambda k: torch.full((k,), float("nan"), device="cuda")
    mean, rstd = nan(n * c), nan(n * c)
    scale, shift = (nan(n * c), nan(n * c)) if case.kw.get("scale_shift") else (None, None)
    rm, rv = _f32(o.get("rm0")), _f32(o.get("rv0"))
    scratch = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.norm_stats_finalize(ops.NORM_KINDS[case.kw["kind"]], case.kw.get("groups", 1), part, route["rows_per_n"], n, c, d * h * w, 1e-5,
                            case.kw.get("training", True), rm, rv, pc.MOMENTUM, mean, rstd, scratch, _f32(o.get("gamma")),
                            _f32(o.get("beta")), scale, shift)
    torch.cuda.synchronize()
    ref = pc.ref_stats_chain(case, o, route)
    if "_rstd_rel" in ref:
        print(f"{case.name}: derived relative bound of rstd {ref.pop('_rstd_rel'):.3e}")
    got = {"mean": mean, "rstd": rstd, "scale": scale, "shift": shift, "running_mean": rm, "running_var": rv}
    for name, (want, bound) in ref.items():
        g = got[name].double().cpu().numpy().reshape(np.shape(want))
        _judge(case, "stats finalize", name, g, want, bound)
        if name == "rstd" and case.kw.get("offset"):
            print(f"{case.name}: observed relative error of rstd {np.max(np.abs(g - want) / want):.3e}")
    if case.kw.get("running") and not case.kw.get("training", True):
        assert torch.equal(rm, _f32(o["rm0"])) and torch.equal(rv, _f32(o["rv0"])), "evaluation must leave the running statistics"


@pytest.mark.parametrize("case", pc.cases_of("bwd_chain"), ids=_ids(pc.cases_of("bwd_chain")))
def test_bwd_reduce_then_finalize(case):
    o = pc.make(case)
    n, c, d, h, w = case.shape
    (db, dv), (yb, yv) = _dev(case, "dout", o["dout"]), _dev(case, "y", o["y"])
    nl = _nl(case, o)
    route = _route(case, [dv, yv], nl)
    part, used = _part(case, route)
    ops.norm_bwd_reduce(dv, yv, nl, part)
    nan = lambda k: torch.full((k,), float("nan"), device="cuda")
    m1, m2 = nan(n * c), nan(n * c)
    dg = db_ = None
    if case.kw.get("dgamma"):
        dg, db_ = (_f32(o["dgamma0"]), _f32(o["dbeta0"])) if case.kw.get("accumulate") else (nan(c), nan(c))
    scratch = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.norm_bwd_finalize(ops.NORM_KINDS[case.kw["kind"]], case.kw.get("groups", 1), part, route["rows_per_n"], n, c, d * h * w, nl.gamma,
                          case.kw.get("training", True), m1, m2, dg, db_, bool(case.kw.get("accumulate")), scratch)
    torch.cuda.synchronize()
    got = {"m1": m1, "m2": m2, "dgamma": dg, "dbeta": db_}
    for name, (want, bound) in pc.ref_bwd_chain(case, o, route).items():
        _judge(case, "bwd finalize", name, got[name].double().cpu().numpy().reshape(np.shape(want)), want, bound)


# ----------------------------------------------------------------------------- elementwise
def _check_out(case, who, family, buf, view, before, ref, bound, leave_out=None):
    torch.cuda.synchronize()
    _judge(case, family, who, view.double().cpu().numpy(), ref, bound, leave_out)
    _untouched(case, who, before, buf)


@pytest.mark.parametrize("case", pc.cases_of("combine"), ids=_ids(pc.cases_of("combine")))
def test_combine(case):
    o = pc.make(case)
    ab, av = _dev(case, "a", o["a"])
    bv = nlb = None
    if case.kw.get("two"):
        bb, bv = _dev(case, "b", o["b"])
        nlb = _nl(case, o, o["cb"])
    nla = _nl(case, o, o["ca"])
    ob, ov = _dev(case, "out")
    route = _route(case, [av, bv, ov] if bv is not None else [av, ov], nla, nlb)
    before = ob.clone()
    ops.combine(av, nla, bv, nlb, ov)
    ref, bound = pc.ref_combine(case, o)
    _check_out(case, "out", route["family"] + " (combine)", ob, ov, before, ref, bound)


@pytest.mark.parametrize("case", pc.cases_of("apply"), ids=_ids(pc.cases_of("apply")))
def test_norm_bwd_apply(case):
    o = pc.make(case)
    (db, dv), (yb, yv), (ob, ov) = _dev(case, "dout", o["dout"]), _dev(case, "y", o["y"]), _dev(case, "dy")
    nl, m1, m2 = _nl(case, o), _f32(o["m1"].reshape(-1)), _f32(o["m2"].reshape(-1))
    route = _route(case, [dv, yv, ov], nl, None, m1, m2)
    before = ob.clone()
    ops.norm_bwd_apply(dv, yv, nl, m1, m2, ov)
    ref, bound, near = pc.ref_apply(case, o)
    _check_out(case, "dy", route["family"] + " (apply)", ob, ov, before, ref, bound, near)


@pytest.mark.parametrize("case", pc.cases_of("small"), ids=_ids(pc.cases_of("small")))
def test_norm_bwd_small(case):
    o = pc.make(case)
    n, c, d, h, w = case.shape
    (db, dv), (yb, yv) = _dev(case, "dout", o["dout"]), _dev(case, "y", o["y"])
    ob, ov = (db, dv) if case.kw.get("in_place") else _dev(case, "dy")
    nl = _nl(case, o)
    route = _route(case, [dv, yv, ov], nl)
    assert ops.norm_bwd_small_ok(dv, yv, nl, ov)
    before = ob.clone()
    ops.norm_bwd_small(dv, yv, nl, d * h * w, ov)
    ref, bound, near = pc.ref_small(case, o, route)
    _check_out(case, "dy", route["family"], ob, ov, before, ref, bound, near)


@pytest.mark.parametrize("case", pc.cases_of("lincomb"), ids=_ids(pc.cases_of("lincomb")))
def test_lincomb(case):
    o = pc.make(case)
    ins = [_dev(case, f"in{k}", o[f"in{k}"])[1] for k in range(case.kw["count"])]
    ob, ov = _dev(case, "out", o.get("out0"))
    route = _route(case, ins + [ov])
    before = ob.clone()
    ops.lincomb(ins, [float(v) for v in o["w"]], ov, accumulate=case.kw["accumulate"])
    ref, bound = pc.ref_lincomb(case, o)
    _check_out(case, "out", route["family"], ob, ov, before, ref, bound)


@pytest.mark.parametrize("case", pc.cases_of("up_fwd", "up_bwd"), ids=_ids(pc.cases_of("up_fwd", "up_bwd")))
def test_upsample(case):
    o = pc.make(case)
    src, dst = ("x", "y") if case.op == "up_fwd" else ("dy", "dx")
    sb, sv = _dev(case, src, o[src])
    ob, ov = _dev(case, dst, o.get("dx0"))
    route = _route(case, [sv, ov])
    before = ob.clone()
    if case.op == "up_fwd":
        ops.upsample2x_fwd(sv, ov)
    else:
        ops.upsample2x_bwd(sv, ov, accumulate=bool(case.kw.get("accumulate")))
    ref, bound = pc.ref_upsample(case, o)
    _check_out(case, dst, route["family"], ob, ov, before, ref, bound)


def test_worst_ratio_per_family():
    """The figures DESIGN.md records (every test above has already held its own elements to <= 1)."""
    for family in sorted(WORST):
        print(f"worst err / bound, {family}: {WORST[family]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
