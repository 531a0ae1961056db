"""Raw staging of the implicit-GEMM family (MMTTA_OPT_RAW_STAGING, option 16, bit 0: igemm_raw_kernel, igemm_reuse_raw_kernel,
igemm_cls8_raw_kernel) against the transform kernels on the same tensors in the same process: option 16 at 0, then at its
default.  A bf16-stored input without norm-on-load goes through unpack, x * 1 + 0, max with -inf and a round back to bf16
in the transform kernels, which returns the bits it was given; the raw kernels store the loaded item under its mask.  The
MFMAs, their operands and their order are the same, so every comparison - outputs, statistics rows, split-K results - is
torch.equal and needs no tolerance.  mmtta_conv_stages_raw must say that the second run staged raw, and mmtta_conv_route
the same route under both settings.

Shapes come from the tile of each kind, not from the workload: one tile, one voxel more along each axis in turn (partial
tiles, every border path), two tiles along x; for the tile that only a large grid selects (<4,4,4,4,8,32> on 27 taps: at
least 96 tiles) that grid with a partial tile on every axis.  Every geometry of conv_geometry.GEOMETRIES that the case
admits is run (`deep` needs K > 64).  Each case runs plain (bias + statistics rows for a forward) and with accumulate plus
a fused add, at batch 1 and 2.

What the raw path has to blank by itself - the halo, and the chunks past Ci of a partial last stage, where the loader
re-reads the last valid chunk - is made visible: the last valid chunk holds large values, and the rows of the packed
weight image behind K, zeros in a real image, are set to 1 for both runs, so that whatever is staged there reaches the
result.  A few inputs are -0.0, the one stored value the transform changes (to +0.0), which no sum that starts at +0 shows.
"""
import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl_bf16

GPU = pytest.mark.gpu
OPT_RAW = 16
ROUTE_LEAN, ROUTE_CLS_FUSED, ROUTE_REUSE = 14, 15, 18
BIG = 2.0 ** 40       # bf16-representable; the squares the statistics rows sum stay far inside fp32

# name: (cin, cout, k, stride, transposed, orientation, tile of the grid the call's tiles cover, extra options, route or None)
KINDS = {
    # the lean tile: route 18 where the geometry leaves K unsplit, 14 where it splits (both have a raw twin)
    "lean-dgrad-32-32": (32, 32, 3, 1, False, "dgrad", (4, 8, 8), {}, None),
    "s1-64-64": (64, 64, 3, 1, False, "fwd", (4, 8, 8), {}, 8),                 # <2,4,4,8,8,32>
    "s1-128-128": (128, 128, 3, 1, False, "fwd", (4, 4, 8), {}, None),          # <4,4,4,4,8,16>; the big grid: <4,4,4,4,8,32>
    "s1-256-128": (256, 128, 3, 1, False, "fwd", (4, 4, 8), {}, 12),            # <4,4,4,4,8,16>, K deep enough for `deep`
    "s2-32-64": (32, 64, 3, 2, False, "fwd", (4, 4, 8), {}, 11),                # <2,2,4,4,8,16>
    "s2-64-128": (64, 128, 3, 2, False, "fwd", (4, 4, 8), {}, 12),              # <4,4,4,4,8,16> at stride 2
    "pw-256-512": (256, 512, 1, 1, False, "fwd", (4, 4, 8), {}, None),          # generic walk of a one-tap class
    "cls8-dgrad-s2-32-64": (32, 64, 3, 2, False, "dgrad", (4, 4, 8), {12: 1}, ROUTE_CLS_FUSED),
    "cls8-convT-128-32": (128, 32, 3, 2, True, "fwd", (4, 4, 8), {12: 1}, ROUTE_CLS_FUSED),
    "classes-dgrad-s2-32-64": (32, 64, 3, 2, False, "dgrad", (4, 8, 8), {12: 1 << 20}, ROUTE_LEAN),      # 8 classes, igemm_kernel
    "convT-dgrad-128-32": (128, 32, 3, 2, True, "dgrad", (4, 4, 8), {}, 12),    # the stride-2 gather of a transposed layer
    # Ci a multiple of 8 but not of the stage depth: row loader (16-deep), generic walk (16-deep, 32-deep), class-fused
    "ci40-lean": (40, 32, 3, 1, False, "fwd", (4, 8, 8), {}, ROUTE_LEAN),
    "ci40-s2": (40, 64, 3, 2, False, "fwd", (4, 4, 8), {}, 11),
    "ci72-s1-64": (72, 64, 3, 1, False, "fwd", (4, 8, 8), {}, 8),
    "ci40-cls8-dgrad": (32, 40, 3, 2, False, "dgrad", (4, 4, 8), {12: 1}, ROUTE_CLS_FUSED),
}
BIG_GRID = {"s1-128-128": (17, 25, 33)}      # 5 x 7 x 5 = 175 tiles >= 96: the 32-deep four-block tile


def _extents(kind):
    tz, ty, tx = KINDS[kind][6]
    out = {"tile": (tz, ty, tx), "z+1": (tz + 1, ty, tx), "y+1": (tz, ty + 1, tx), "x+1": (tz, ty, tx + 1), "2x": (tz, ty, 2 * tx)}
    if kind in BIG_GRID:
        out["grid"] = BIG_GRID[kind]
    return out


def _case(kind, grid, n):
    """The conv_geometry case whose call of the kind's orientation tiles `grid`."""
    cin, cout, k, stride, transposed, orient, _, _, _ = KINDS[kind]
    if transposed:
        shape = grid                                   # forward: x is the coarse tensor; input gradient: dx is
    elif stride == 1:
        shape = grid
    elif orient == "fwd":
        shape = tuple(2 * v - 1 for v in grid)         # odd extents: the halo crosses the high border
    else:
        shape = tuple(2 * v for v in grid)             # dy = grid
    return cg.case(f"raw_{kind}_{n}x" + "x".join(map(str, grid)), cin, cout, k, stride, transposed, (n,) + tuple(shape))


_query = cg.query


def _stages_raw(*a, **k):
    return _query("mmtta_conv_stages_raw", *a, **k)


def _route(*a, **k):
    return _query("mmtta_conv_route", *a, **k)


# ----------------------------------------------------------------------------- without a GPU
def test_option_16_defaults_to_both_bits_and_restores():
    from multimodal_tta_amd import ops
    assert cg.current_options((OPT_RAW,)) == {OPT_RAW: 3}
    with cg.pinned({OPT_RAW: 0}):
        assert cg.current_options((OPT_RAW,)) == {OPT_RAW: 0}
    assert ops.set_option(OPT_RAW, 3) == 3


def test_query_names_the_eligible_calls_only():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_DGRAD, CONV_FWD, CONVT_FWD, F32, ConvDesc, NormOnLoad
    X, Y, A, P = 1 << 30, 1 << 40, 1 << 41, 1 << 21
    e = (16, 16, 16)
    t = lambda base, c, dhw=e, bf=True, n=2: cg._fake_tensor(_lib, base, n, c, dhw, bf)
    d64 = ConvDesc(CONV_FWD, 3, 1, 64, 64, BF16)
    with cg.pinned({OPT_RAW: 3}):
        assert _stages_raw(d64, t(X, 64), t(Y, 64)) == 1
        assert _stages_raw(d64, t(X, 64), t(Y, 64), add=t(A, 64), accumulate=1, stats=P) == 1
        assert _stages_raw(d64, t(X, 64), t(Y, 64), x_nl=NormOnLoad()) == 1, "a norm-on-load that does nothing"
        assert _stages_raw(ConvDesc(CONV_DGRAD, 3, 1, 32, 32, BF16), t(X, 32), t(Y, 32)) == 1
        assert _stages_raw(ConvDesc(CONV_DGRAD, 3, 2, 32, 64, BF16), t(X, 64, (8, 8, 8)), t(Y, 32)) == 1
        assert _stages_raw(ConvDesc(CONVT_FWD, 3, 2, 128, 32, BF16), t(X, 128, (8, 8, 8)), t(Y, 32)) == 1
        # not raw
        assert _stages_raw(d64, t(X, 64, bf=False), t(Y, 64, bf=False)) == 0, "fp32-stored x"
        assert _stages_raw(ConvDesc(CONV_FWD, 3, 1, 36, 64, BF16), t(X, 36), t(Y, 64)) == 0, "Ci = 36: a chunk with row padding"
        assert _stages_raw(d64, t(X, 64), t(Y, 64), x_nl=NormOnLoad(mean=P, rstd=P)) == 0, "norm-on-load with mean"
        assert _stages_raw(d64, t(X, 64), t(Y, 64), x_nl=NormOnLoad(scale=P, shift=P)) == 0, "norm-on-load with scale"
        assert _stages_raw(d64, t(X, 64), t(Y, 64), x_nl=_lib.norm_on_load(relu=True)) == 0, "activation-only norm-on-load"
        assert _stages_raw(d64, t(X, 64), t(Y, 64), x_nl=_lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=0.1)) == 0
        assert _stages_raw(d64, t(X + 8, 64), t(Y, 64)) == 0, "x off its 16-byte items"
        assert _stages_raw(ConvDesc(CONV_FWD, 3, 1, 64, 64, F32), t(X, 64, bf=False), t(Y, 64, bf=False)) == 0, "fp32 precision"
        assert _stages_raw(ConvDesc(CONV_FWD, 3, 1, 64, 4, BF16), t(X, 64), t(Y, 4)) == 0, "the direct kernels (<= 4 produced channels)"
        assert _stages_raw(ConvDesc(CONV_FWD, 1, 1, 64, 64, BF16), t(X, 64, (32, 32, 32)), t(Y, 64, (32, 32, 32))) == 0, \
            "the streaming 1x1x1 kernel (route 17)"
        for bits, want in ((0, 0), (2, 0), (1, 1)):
            with cg.pinned({OPT_RAW: bits}):
                assert _stages_raw(d64, t(X, 64), t(Y, 64)) == want, f"option 16 = {bits}"
        assert _stages_raw(ConvDesc(CONV_FWD, 5, 1, 64, 64, BF16), t(X, 64), t(Y, 64)) < 0, "an invalid call is an error"


def test_routes_do_not_depend_on_the_option():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_DGRAD, CONV_FWD, CONVT_DGRAD, CONVT_FWD, ConvDesc
    X, Y = 1 << 30, 1 << 40
    seen = set()
    for geo in ("inflight1", "inflight24", "unsplit"):
        for kind, (cin, cout, k, stride, transposed, orient, tile, extra, _) in KINDS.items():
            for grid in (tile, (16, 16, 16)):
                c = _case(kind, grid, 2)
                desc, x, y = cg._descs(c, "bf16", orient, True)
                got = []
                for bits in (0, 3):
                    with cg.pinned({**cg.geometry_values(geo), **extra, OPT_RAW: bits}):
                        got.append(_route(desc, x, y))
                assert got[0] == got[1] and got[0] >= 0, (kind, grid, geo, got)
                seen.add(got[0])
    assert {8, 11, 12, ROUTE_LEAN, ROUTE_CLS_FUSED, ROUTE_REUSE} <= seen


def test_shapes_are_small():
    for kind in KINDS:
        for name, grid in _extents(kind).items():
            assert name == "grid" or max(grid) <= 16


# ----------------------------------------------------------------------------- on the GPU
def _operands(kind, grid, n, sliced):
    """x (with -0.0 entries; Ci off the stage depth: large values in its last chunk), the fused-add operand, the accumulate
    prefill - all bf16-stored, channels-last - and weights / bias."""
    c = _case(kind, grid, n)
    orient = KINDS[kind][5]
    g = torch.Generator().manual_seed(977 + sum(ord(ch) for ch in c.name))
    rnd = lambda *s: torch.randn(*s, generator=g)
    lo = (n, c.cin) + tuple(c.shape[1:])
    hi = (n, c.cout) + cg.out_dhw(c)
    xs, ys = (lo, hi) if orient == "fwd" else (hi, lo)
    x = rnd(*xs) * 1.5 + 0.25
    x[rnd(*xs) > 1.2] = -0.0
    if xs[1] % 16:
        x[:, xs[1] - 8:] *= BIG
    if sliced:
        # x as cat[..., :c] of a buffer twice as wide, the neighbour's channels large too
        wide = cl_bf16(torch.cat([x, torch.full(xs, BIG)], dim=1))
        xd = wide[..., :xs[1]]
    else:
        xd = cl_bf16(x)
    assert (xd.float() == 0).any() and torch.signbit(xd.float()[xd.float() == 0]).any()
    fan = (c.cout if c.transposed else c.cin) * c.k ** 3
    return c, xd, rnd(*ys) * 1.5 + 0.2, rnd(*ys), rnd(*cg.weight_shape(c)) * fan ** -0.5, rnd(ys[1]).cuda()


def _op(c, w, orient):
    """The ConvOp with its weights packed; the rows of the image behind K (zeros in a real image) set to 1."""
    from multimodal_tta_amd import ops
    op = ops.ConvOp(c.cin, c.cout, c.k, c.stride, c.transposed, "cuda", dtype=ops.BF16)
    op.pack(w.cuda().contiguous())
    K = c.cin if orient == "fwd" else c.cout
    N = c.cout if orient == "fwd" else c.cin
    Kp, Np = (K + 31) // 32 * 32, (N + 31) // 32 * 32
    img = (op.packed_fwd if orient == "fwd" else op.packed_dgrad).view(torch.bfloat16)
    assert img.numel() == c.k ** 3 * Kp * Np      # the bf16 image [T][Kp / 8][Np][8]
    img.view(c.k ** 3, Kp // 8, Np, 8)[:, K // 8:] = 1.0
    return op


def _run_forms(op, c, orient, xd, res, y0, bias, want_raw):
    """{form: (y, statistics rows or None)} under the options as they are; asserts what the query says first."""
    from multimodal_tta_amd import ops
    fwd = orient == "fwd"
    desc, packed = (op.d_fwd, op.packed_fwd) if fwd else (op.d_dgrad, op.packed_dgrad)
    out = {}
    for form in ("plain", "accumulate + fused add"):
        fused = form != "plain"
        y = cl_bf16(y0 if fused else torch.zeros_like(y0))
        add = cl_bf16(res) if fused else None
        st = torch.full((op.plan(desc, xd, y).stats_rows, 2, y.shape[-1]), float("nan"), device="cuda") if fwd else None
        args = (desc, ops.desc_cl(xd), ops.desc_cl(y))
        kw = dict(add=ops.desc_cl(add) if fused else None, accumulate=1 if fused else 0, stats=ops.ptr(st))
        assert _stages_raw(*args, **kw) == want_raw, f"{form}: mmtta_conv_stages_raw"
        route = _route(*args, **kw)
        op._run(desc, packed, xd, None, bias if fwd else None, y, fused, st, add, None)
        out[form] = (y, st, route)
    torch.cuda.synchronize()
    return out


@GPU
@pytest.mark.parametrize("n", [1, 2], ids=["batch1", "batch2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_raw_staging_equals_the_transform_kernels(kind, n):
    cin, cout, k, stride, transposed, orient, tile, extra, want_route = KINDS[kind]
    before = cg.current_options(cg.GEOMETRY_KEYS + (OPT_RAW,))
    ran = 0
    for ext, grid in _extents(kind).items():
        sliced = ext == "x+1"
        c, xd, res, y0, w, bias = _operands(kind, grid, n, sliced)
        geos = ("inflight24",) if ext == "grid" else cg.GEOMETRIES
        for geo in geos:
            vals = cg.planned(c, "bf16", geo, orient, True)[0]
            if vals is None:          # the shape admits no deep split
                continue
            got = {}
            for bits in (0, 3):
                with cg.pinned({**vals, **extra, OPT_RAW: bits}):
                    got[bits] = _run_forms(_op(c, w, orient), c, orient, xd, res, y0, bias, 1 if bits else 0)
            for form, (ya, sa, ra) in got[0].items():
                yb, sb, rb = got[3][form]
                what = f"{kind} {ext} x{n} {geo}: {form}"
                assert ra == rb and (want_route is None or ra == want_route or ext == "grid"), f"{what}: routes {ra}, {rb}"
                assert torch.isfinite(ya.float()).all(), f"{what}: the transform kernel left non-finite values"
                assert torch.equal(ya, yb), f"{what}: outputs differ, max |diff| {(ya.float() - yb.float()).abs().max().item():.3e}"
                if sa is not None:
                    assert torch.isfinite(sa).all() and torch.equal(sa, sb), f"{what}: statistics rows differ"
            ran += 1
    assert ran >= 5 * 4
    assert cg.current_options(cg.GEOMETRY_KEYS + (OPT_RAW,)) == before


def test_the_big_grid_runs_the_32_deep_four_block_tile():
    """What the `grid` extent of s1-128-128 is there for: config 9 (<4,4,4,4,8,32>) under the benchmark's tuning."""
    c = _case("s1-128-128", BIG_GRID["s1-128-128"], 1)
    with cg.pinned(cg.geometry_values("inflight24")):
        assert cg.ask_plan(c, "bf16", "fwd", True)[1] == 9
