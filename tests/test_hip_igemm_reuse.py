"""igemm_reuse_kernel (route 18: the lean 4 x 8 x 8 tile of the 3x3x3 stride-1 32 -> 32 layers of bf16 precision, the rows of a
wave's two MFMA blocks split by the parity of x so that neighbouring kx taps share activation fragments) against
igemm_kernel<1, 2, 4, 8, 8, 16, bf16, 3> (route 14) on the same tensors in the same process: MMTTA_OPT_IGEMM_FRAGMENT_REUSE
(14) 1 / 0.  Both issue the same MFMAs with the same operands in the same order and share one epilogue behind the
transposition tile, so every comparison is torch.equal - outputs and statistics rows - and needs no tolerance.

Shapes come from the tile constants of the source: one tile, one voxel more along each axis in turn (partial tiles, every
border path), two tiles along x (the shifted window meets the seam between two tiles' halos), and a 3 x 3 x 5 grid of tiles
with a partial tile on every axis, which is the smallest shape here that the tuning for 24 volumes in flight - the
benchmark's - leaves unsplit.  Batch 1, and 2 items that are 2 parameter sets (own weights and bias per item).  Every
geometry the tuner sets is run; K = 32 admits no `deep` split (two stages: a split is one stage per workgroup).  The new
route takes unsplit launches only: where a geometry splits K the call stays on route 14 under both settings, which the
test asserts before it compares.
"""
import ctypes as C
import os
import re

import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl, cl_bf16

GPU = pytest.mark.gpu
OPT_REUSE = 14
ROUTE_LEAN, ROUTE_REUSE = 14, 18
CH = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    """(TZ, TY, TX) of igemm_reuse_kernel, from its instantiation of the shared body."""
    with open(os.path.join(ROOT, "multimodal_tta_amd", "csrc", "conv_igemm.hip")) as fh:
        src = fh.read()
    m = re.search(r"void igemm_reuse_kernel\(GArgs a\) \{\s*constexpr int NB = 1, MB = 2, TZ = (\d+), TY = (\d+), TX = (\d+),", src)
    assert m, "igemm_reuse_kernel's instantiation not found"
    return tuple(int(v) for v in m.groups())


TZ, TY, TX = _tile()
SHAPES = {
    "tile": (TZ, TY, TX),
    "z+1": (TZ + 1, TY, TX),
    "y+1": (TZ, TY + 1, TX),
    "x+1": (TZ, TY, TX + 1),
    "2x": (TZ, TY, 2 * TX),
    "grid": (2 * TZ + 1, 2 * TY + 1, 4 * TX + 1),
}
GEOMETRIES = tuple(g for g in cg.GEOMETRIES if g != "deep")


def _case(shape, n):
    return cg.case(f"reuse_{n}x" + "x".join(map(str, shape)), CH, CH, 3, 1, False, (n,) + tuple(shape))


def _fake(base, n, dhw, bf):
    from multimodal_tta_amd import _lib
    return cg._fake_tensor(_lib, base, n, CH, dhw, bf)


def _ask_route(desc, x, y, x_nl=None, add=None, add_nl=None, accumulate=0, stats=None):
    """mmtta_conv_route for descriptors `x`, `y`, `add` (_lib.Tensor)."""
    from multimodal_tta_amd import _lib
    epi = None
    if add is not None:
        epi = _lib.ConvEpilogue(C.pointer(add), add_nl if add_nl is not None else _lib.norm_on_load())
    return int(_lib.load().mmtta_conv_route(C.byref(desc), C.byref(x), C.byref(x_nl) if x_nl is not None else None,
                                            C.byref(epi) if epi is not None else None, C.byref(y), accumulate, stats))


# ----------------------------------------------------------------------------- without a GPU
def test_tile_constants_are_the_lean_tile():
    assert (TZ, TY, TX) == (4, 8, 8)
    assert all(max(s) <= 40 for s in SHAPES.values())


def test_k32_admits_no_deep_split():
    for n in (1, 2):
        for shape in SHAPES.values():
            assert cg.deep_target(_case(shape, n), "bf16", "fwd") is None


def test_the_reuse_route_is_the_default():
    """Option 14 untouched (the launch geometry of the benchmark and the defaults of the options the gate reads are pinned): it reads 1 and the 64^3 32 -> 32
    forward runs route 18.  What the header and DESIGN.md say the default is, is asserted here."""
    from multimodal_tta_amd._lib import BF16, CONV_FWD, ConvDesc
    assert cg.current_options((OPT_REUSE,)) == {OPT_REUSE: 1}
    with cg.pinned({**cg.geometry_values("inflight24"), 6: 1, 9: 1, 10: 1}):      # (their defaults; other modules pin them)
        x, y = _fake(1 << 30, 8, (64, 64, 64), True), _fake(1 << 40, 8, (64, 64, 64), True)
        assert _ask_route(ConvDesc(CONV_FWD, 3, 1, CH, CH, BF16), x, y) == ROUTE_REUSE


def test_route_names_the_reuse_kernel_for_the_headline_class_only():
    """With option 14 on, under the tuning of the benchmark (3 lanes x 8 volumes in flight), the 32 -> 32 layers of the 64^3 level run route 18,
    forward (bf16-stored) and input gradient (fp32-stored), with and without the fused operands; mmtta_conv_plan, which
    sees no run-time operands, keeps reporting the tile (14).  Neighbouring classes keep their routes."""
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_DGRAD, CONV_FWD, F32, ConvDesc, ConvPlan, NormOnLoad
    lib = _lib.load()
    X, Y, A, STATS = 1 << 30, 1 << 40, 1 << 41, 1 << 20
    e64, e32 = (64, 64, 64), (32, 32, 32)

    def config(desc, x, y):
        plan = ConvPlan()
        assert lib.mmtta_conv_plan(C.byref(desc), C.byref(x), C.byref(y), C.byref(plan)) == 0
        return int(plan.config), int(plan.ksplit)

    with cg.pinned({**cg.geometry_values("inflight24"), OPT_REUSE: 1, 6: 1, 9: 1, 10: 1}):
        for op, stored in ((CONV_FWD, True), (CONV_FWD, False), (CONV_DGRAD, False)):
            desc = ConvDesc(op, 3, 1, CH, CH, BF16)
            x, y, add = _fake(X, 8, e64, stored), _fake(Y, 8, e64, stored), _fake(A, 8, e64, stored)
            assert config(desc, x, y) == (ROUTE_LEAN, 1)
            assert _ask_route(desc, x, y) == ROUTE_REUSE
            assert _ask_route(desc, x, y, stats=STATS, accumulate=1) == ROUTE_REUSE
            assert _ask_route(desc, x, y, x_nl=NormOnLoad(scale=1 << 21, shift=1 << 22), add=add) == ROUTE_REUSE
            # what the kernel has no path for stays on the tile's plain kernel
            assert _ask_route(desc, x, _fake(Y, 8, e64, not stored)) == ROUTE_LEAN, "x and y in different storage types"
            assert _ask_route(desc, x, y, add=_fake(A + 4, 8, e64, stored)) == ROUTE_LEAN, "add off its 16-byte quads"
            assert _ask_route(desc, _fake(X + 4, 8, e64, stored), y) == ROUTE_LEAN, "x off its 16-byte items: no row loader"
            for key in (OPT_REUSE, 6, 9):
                with cg.pinned({key: 0}):
                    assert _ask_route(desc, x, y) == ROUTE_LEAN, f"option {key} = 0"
            with cg.pinned({10: 0}):
                assert _ask_route(desc, x, y) == 7, "the 8 x 8 x 8 tile"
            # fp32 precision: the fp32 tile of the shape
            d32 = ConvDesc(op, 3, 1, CH, CH, F32)
            assert _ask_route(d32, _fake(X, 8, e64, False), _fake(Y, 8, e64, False)) == 0
        # a small grid splits K: route 14 (the split-K partial sums are the plain kernel's)
        desc = ConvDesc(CONV_FWD, 3, 1, CH, CH, BF16)
        small = (TZ, TY, TX)
        assert config(desc, _fake(X, 1, small, True), _fake(Y, 1, small, True)) == (ROUTE_LEAN, 2)
        assert _ask_route(desc, _fake(X, 1, small, True), _fake(Y, 1, small, True)) == ROUTE_LEAN
        # 32 -> 64 stride 2 (forward 11; its input gradient is the per-class or class-fused form), 64 -> 64 at 32^3 (8),
        # 96 -> 32 on the lean tile (14: not this class)
        t = lambda base, c, dhw, bf=True: cg._fake_tensor(_lib, base, 8, c, dhw, bf)
        assert _ask_route(ConvDesc(CONV_FWD, 3, 2, 32, 64, BF16), t(X, 32, e64), t(Y, 64, e32)) == 11
        assert _ask_route(ConvDesc(CONV_DGRAD, 3, 2, 32, 64, BF16), t(X, 64, e32, False), t(Y, 32, e64, False)) in (14, 15)
        for op in (CONV_FWD, CONV_DGRAD):
            assert _ask_route(ConvDesc(op, 3, 1, 64, 64, BF16), t(X, 64, e32, op == CONV_FWD), t(Y, 64, e32, op == CONV_FWD)) == 8
        assert _ask_route(ConvDesc(CONV_FWD, 3, 1, 96, 32, BF16), t(X, 96, e64), t(Y, 32, e64)) == ROUTE_LEAN
        assert _ask_route(ConvDesc(CONV_DGRAD, 3, 1, 32, 96, BF16), t(X, 96, e64, False), t(Y, 32, e64, False)) == ROUTE_LEAN


# ----------------------------------------------------------------------------- on the GPU
def _inputs(shape, n):
    g = torch.Generator().manual_seed(4242 + 31 * n + sum(shape))
    rnd = lambda *s: torch.randn(*s, generator=g)
    d, h, w = shape
    full = (n, CH, d, h, w)
    return dict(x=rnd(*full) * 1.5 + 0.25, gy=rnd(*full), res=rnd(*full) * 1.5 + 0.2, y0=rnd(*full), w=rnd(n, CH, CH, 3, 3, 3) * (CH * 27) ** -0.5,
                b=rnd(n, CH), sc=rnd(n * CH).abs() + 0.5, sh=rnd(n * CH) * 0.3, rsc=rnd(n * CH).abs() + 0.5, rsh=rnd(n * CH) * 0.3)


def _make_op(inp, n):
    from multimodal_tta_amd import ops

    class Ctl:
        use_sets = True

    op = ops.ConvOp(CH, CH, 3, 1, False, "cuda", dtype=ops.BF16, n_sets=n)
    for j in range(n):
        op.pack(inp["w"][j].cuda().contiguous(), j)
    if n > 1:
        op.set_param_sets(1, 1, CH * CH * 27, 0, CH, 0, Ctl())      # item j reads image j and bias row j
    return op, inp["b"].cuda().contiguous()


def _nl(sc, sh, leaky=False):
    from multimodal_tta_amd import ops
    sc, sh = sc.cuda(), sh.cuda()
    if leaky:
        return ops.NL(sc, sc, scale=sc, shift=sh, act=ops.ACT_LEAKY_RELU, negative_slope=0.1)
    return ops.NL(sc, sc, relu=True, scale=sc, shift=sh)


def _run_all(op, bias, inp, n, shape, want_route):
    """Every form of the class under the options as they are: {name: (output, statistics rows or None)}.  Asserts the route
    of each call first."""
    from multimodal_tta_amd import ops
    d, h, w = shape
    out = {}

    def launch(name, desc, packed, x, x_nl, b, y, accumulate=False, stats=False, add=None, add_nl=None):
        st = torch.full((op.stats_rows(x, y), 2, CH), float("nan"), device="cuda") if stats else None
        route = _ask_route(desc, ops.desc_cl(x), ops.desc_cl(y), x_nl.struct() if x_nl is not None else None,
                           ops.desc_cl(add) if add is not None else None, add_nl.struct() if add_nl is not None else None,
                           1 if accumulate else 0, ops.ptr(st))
        assert route == want_route, f"{name}: route {route}, expected {want_route}"
        op._run(desc, packed, x, x_nl, b, y, accumulate, st, add, add_nl)
        out[name] = (y, st)

    for stored in (False, True):
        put = cl_bf16 if stored else cl
        tag = "bf16-stored" if stored else "fp32-stored"
        fresh = lambda: put(torch.zeros(n, CH, d, h, w))
        x = put(inp["x"])
        fwd = lambda name, *a, **k: launch(f"forward {name}, {tag}", op.d_fwd, op.packed_fwd, x, *a, **k)
        fwd("bias + statistics", None, bias, fresh(), stats=True)
        fwd("norm-on-load ReLU + statistics", _nl(inp["sc"], inp["sh"]), bias, fresh(), stats=True)
        fwd("norm-on-load LeakyReLU", _nl(inp["sc"], inp["sh"], leaky=True), bias, fresh())
        fwd("norm-on-load + fused add under its own norm-on-load + statistics", _nl(inp["sc"], inp["sh"]), bias, fresh(), stats=True,
            add=put(inp["res"]), add_nl=_nl(inp["rsc"], inp["rsh"]))
        fwd("fused add under a LeakyReLU norm-on-load", None, bias, fresh(), add=put(inp["res"]), add_nl=_nl(inp["rsc"], inp["rsh"], leaky=True))
        fwd("accumulate", None, bias, put(inp["y0"]), accumulate=True)
    gy = cl(inp["gy"])
    fresh = lambda: cl(torch.zeros(n, CH, d, h, w))
    dg = lambda name, *a, **k: launch(f"input gradient {name}", op.d_dgrad, op.packed_dgrad, gy, *a, **k)
    dg("plain", None, None, fresh())
    dg("norm-on-load ReLU", _nl(inp["sc"], inp["sh"]), None, fresh())
    dg("norm-on-load LeakyReLU", _nl(inp["sc"], inp["sh"], leaky=True), None, fresh())
    dg("fused add under its own norm-on-load", None, None, fresh(), add=cl(inp["res"]), add_nl=_nl(inp["rsc"], inp["rsh"]))
    dg("accumulate", None, None, cl(inp["y0"]), accumulate=True)
    dg("accumulate + fused add", None, None, cl(inp["y0"]), accumulate=True, add=cl(inp["res"]))
    torch.cuda.synchronize()
    return out


@GPU
@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("n", [1, 2], ids=["one-item", "two-sets"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_reuse_route_equals_the_plain_lean_kernel(shape, n, geo):
    from multimodal_tta_amd import ops
    dhw = SHAPES[shape]
    c = _case(dhw, n)
    before = cg.current_options(cg.GEOMETRY_KEYS + (6, 9, 10, OPT_REUSE))
    vals, ksplit, config, _ = cg.planned(c, "bf16", geo, "fwd", False)
    assert config == ROUTE_LEAN and cg.planned(c, "bf16", geo, "dgrad", False)[1] == ksplit
    if geo == "unsplit" or (geo == "inflight24" and shape == "grid"):
        assert ksplit == 1, "this geometry is here for the new route"
    inp = _inputs(dhw, n)
    res = {}
    for mode in (0, 1):
        with cg.pinned({**vals, OPT_REUSE: mode}):
            op, bias = _make_op(inp, n)
            res[mode] = _run_all(op, bias, inp, n, dhw, ROUTE_REUSE if (mode and ksplit == 1) else ROUTE_LEAN)
    assert res[0].keys() == res[1].keys() and len(res[0]) == 18
    for name, (y0, st0) in res[0].items():
        y1, st1 = res[1][name]
        assert torch.isfinite(y0.float()).all(), f"{name}: the plain kernel left non-finite values"
        assert torch.equal(y0, y1), f"{shape} x{n} {geo}: {name}: outputs differ, max |diff| {(y0.float() - y1.float()).abs().max().item():.3e}"
        if st0 is not None:
            assert torch.isfinite(st0).all() and torch.equal(st0, st1), f"{shape} x{n} {geo}: {name}: statistics rows differ"
    assert cg.current_options(cg.GEOMETRY_KEYS + (6, 9, 10, OPT_REUSE)) == before


@GPU
def test_a_bias_off_its_16_bytes_keeps_the_plain_kernel():
    """mmtta_conv_route sees no bias; the run does.  A bias that is not 16-byte aligned sends the tile's plain kernel to its
    4-byte epilogue, whose statistics rows sum in another order, so such a run stays on route 14 under option 14 = 1 as
    well: outputs and statistics rows equal bit for bit between the two settings, and the output equals the aligned
    run's (the statistics rows of the two epilogues agree within summation order only, and are not compared)."""
    dhw, n = SHAPES["grid"], 1
    inp = _inputs(dhw, n)
    vals = cg.geometry_values("unsplit")
    res = {}
    for mode in (0, 1):
        with cg.pinned({**vals, OPT_REUSE: mode}):
            op, bias = _make_op(inp, n)
            off = torch.zeros(CH + 1, device="cuda")
            off[1:] = bias[0]
            x = cl_bf16(inp["x"])
            out = []
            for b in (off[1:], bias):
                assert (b.data_ptr() % 16 == 0) == (b is bias)
                y = cl_bf16(torch.zeros(n, CH, *dhw))
                st = torch.full((op.stats_rows(x, y), 2, CH), float("nan"), device="cuda")
                op.forward(x, None, b, y, stats=st)
                out.append((y, st))
            torch.cuda.synchronize()
            res[mode] = out
    for k in (0, 1):
        assert torch.equal(res[0][k][0], res[1][k][0]) and torch.equal(res[0][k][1], res[1][k][1])
    assert torch.equal(res[1][0][0], res[1][1][0]) and torch.isfinite(res[1][0][1]).all()
