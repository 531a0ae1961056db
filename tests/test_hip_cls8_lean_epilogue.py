"""The class-fused stride-2 kernel with the lean interior epilogue (MMTTA_OPT_CLS8_LEAN_EPILOGUE, option 21:
igemm_cls8_lean_kernel) against igemm_cls8_pipe_kernel on the same tensors in the same process: options {12: 1, 20: 1} with
option 21 at 0, then at 1.  The K loop is the same text; a tile whose 8 x 8 x 16 output block lies inside the tensor takes
epilogue_cls8_lean - row offsets once per tile, operands of the next classes requested ahead, 16-byte stores through a lane-pair
exchange, no statistics arithmetic when no rows are asked for - and every other tile the eight epilogue_vec16 calls of the twin.
The values go through the same operations in the same order, so every comparison - outputs, accumulated / fused-add
destinations, statistics rows - is torch.equal and needs no tolerance.  mmtta_conv_cls8_lean_epilogue must say 1 for the
second run and mmtta_conv_route 15 both times.

Both forms: ConvTranspose3d forward (K = cin gathered, N = cout produced) and the input gradient of a stride-2 Conv3d (K = cout,
N = cin), on the coarse grid of the form; each case four ways: plain (a forward: bias + statistics rows), with a fused add
only, with accumulate only, with both (the four instantiations of the lean epilogue).  The shapes are the smallest that reach
every path of the new code:
  tiles      coarse 4 x 4 x 8: one interior tile; 8 x 4 x 8: two and the face between them; 5 x 4 x 9: one interior tile beside
             three border tiles, both epilogues in one launch; 5 x 3 x 9: no interior tile
  stages     K = 16 and 48: one stage and an odd number of them (which LDS image the epilogue meets last); K = 40: a partial
             last stage
  columns    N = 64: two column groups; N = 24 and 40: a partial column block, whose dead lane pairs must store nothing - y is
             the leading channels of a tensor 8 channels wider that holds a sentinel, and the whole tensor is compared
  odd dx     an input gradient with dy coarse 4 x 4 x 8 and dx 7 x 7 x 15: the classes of odd parity are one voxel shorter, the
             single tile must take the border path
  batching   batch 3 with a parameter set per item
  slices     a fused add that is a channel slice of a wider tensor (its strides differ from y's)
Refused calls - a norm-on-load on x; 36 produced channels (y is then a 36-channel slice of 40-channel rows, which route 15
admits) - must report 0 from the query and give the same result under both settings."""
import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl_bf16

GPU = pytest.mark.gpu
OPT_LEAN, OPT_PIPE, OPT_CLS_MIN = 21, 20, 12
ROUTE_CLS_FUSED = 15
BIG = 2.0 ** 40       # bf16-representable; the squares the statistics rows sum stay far inside fp32
SENTINEL = 7.0
TILE, FACE, MIXED, RAGGED = (4, 4, 8), (8, 4, 8), (5, 4, 9), (5, 3, 9)
VARIANTS = {"plain": (False, False), "fused add": (True, False), "accumulate": (False, True), "accumulate + fused add": (True, True)}

# name: (K, N, coarse extent, batch, a parameter set per item, extra channels behind y's rows, extra channels behind the add's,
#        the fine extent where it is not twice the coarse one)
SHAPES = {
    "tile": (32, 32, TILE, 1, False, 0, 0, None),
    "face": (32, 32, FACE, 1, False, 0, 0, None),
    "mixed": (32, 32, MIXED, 1, False, 0, 0, None),
    "ragged": (32, 32, RAGGED, 1, False, 0, 0, None),
    "K16": (16, 32, TILE, 1, False, 0, 0, None),
    "K48": (48, 32, MIXED, 1, False, 0, 0, None),
    "K40-partial": (40, 32, TILE, 1, False, 0, 0, None),
    "N64": (32, 64, TILE, 1, False, 0, 0, None),
    "N24": (32, 24, MIXED, 1, False, 8, 0, None),
    "N40": (32, 40, TILE, 1, False, 8, 0, None),
    "odd-dx": (32, 32, TILE, 1, False, 0, 0, (7, 7, 15)),
    "batch3-sets": (32, 32, MIXED, 3, True, 0, 0, None),
    "add-slice": (32, 32, MIXED, 1, False, 0, 16, None),
}
FORMS = ("convT-fwd", "s2-dgrad")
CASES = [(form, name) for name in SHAPES for form in FORMS if not (form == "convT-fwd" and SHAPES[name][7] is not None)]
REFUSED = {"N36": (32, 36, MIXED, 1, False, 0, 0, None)}      # channels in groups of 4, not 8
SHAPES_ALL = dict(SHAPES, **REFUSED)


def _case(form, name):
    K, N, grid, n, _, _, _, fine = SHAPES_ALL[name]
    if form == "convT-fwd":
        return cg.case(f"lean_{form}_{name}", K, N, 3, 2, True, (n,) + grid), "fwd"
    fine = fine if fine is not None else tuple(2 * v for v in grid)
    return cg.case(f"lean_{form}_{name}", N, K, 3, 2, False, (n,) + fine), "dgrad"      # dy = grid


_query = cg.query


def test_shapes_are_small():
    for K, N, grid, n, _, ypad, apad, fine in SHAPES_ALL.values():
        assert max(grid) <= 9 and n <= 3 and max(K, N) + max(ypad, apad) <= 64 + 16
        assert max(K, N) <= 64 and (fine is None or all(2 * g - 1 <= f <= 2 * g for g, f in zip(grid, fine)))


def test_the_shapes_reach_both_epilogues():
    """Interior tiles (coarse 4 x 4 x 8 tiles whose output block lies inside y) and border tiles per shape, from the extents."""
    def tiles(name):
        _, _, grid, _, _, _, _, fine = SHAPES_ALL[name]
        fine = fine if fine is not None else tuple(2 * v for v in grid)
        per_axis = [[2 * (t0 + T) <= f for t0 in range(0, g, T)] for g, f, T in zip(grid, fine, TILE)]
        inside = sum(a and b and c for a in per_axis[0] for b in per_axis[1] for c in per_axis[2])
        return inside, len(per_axis[0]) * len(per_axis[1]) * len(per_axis[2]) - inside
    assert tiles("tile") == (1, 0) and tiles("face") == (2, 0) and tiles("mixed") == (1, 3) and tiles("ragged") == (0, 4)
    assert tiles("odd-dx") == (0, 1)


def _wide(t, pad, fill):
    """A bf16 channels-last copy of `t` ([N, D, H, W, C] view) as the leading channels of rows `pad` channels wider that hold
    `fill`: (view, whole tensor).  pad = 0: the tensor itself."""
    if pad == 0:
        return t, t
    whole = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), fill, dtype=torch.bfloat16, device="cuda")
    view = whole[..., :t.shape[-1]]
    view.copy_(t)
    return view, whole


def _operands(form, name):
    c, orient = _case(form, name)
    K, N, grid, n, per_item = SHAPES_ALL[name][:5]
    g = torch.Generator().manual_seed(21 + sum(ord(ch) for ch in c.name))
    rnd = lambda *s: torch.randn(*s, generator=g)
    lo, hi = (n, c.cin) + tuple(c.shape[1:]), (n, c.cout) + cg.out_dhw(c)
    xs, ys = (lo, hi) if orient == "fwd" else (hi, lo)
    assert xs[1] == K and ys[1] == N and tuple(xs[2:]) == grid
    x = rnd(*xs) * 1.5 + 0.25
    if K % 16:
        x[:, K - 8:] *= BIG
    nw = n if per_item else 1
    fan = (c.cout if c.transposed else c.cin) * 27
    return dict(c=c, orient=orient, x=cl_bf16(x), res=rnd(*ys) * 1.5 + 0.2, y0=rnd(*ys), w=rnd(nw, *cg.weight_shape(c)) * fan ** -0.5,
                bias=rnd(nw, N).cuda().contiguous())


def _op(o, name):
    """The ConvOp with its weights packed (one image per item where the case says so); the rows of every image behind K
    (zeros in a real image) set to 1."""
    from multimodal_tta_amd import ops

    class Ctl:
        use_sets = True

    c, orient = o["c"], o["orient"]
    K, N, _, n, per_item = SHAPES_ALL[name][:5]
    nw = o["w"].shape[0]
    op = ops.ConvOp(c.cin, c.cout, 3, 2, c.transposed, "cuda", dtype=ops.BF16, n_sets=nw)
    for j in range(nw):
        op.pack(o["w"][j].cuda().contiguous(), j)
    if per_item:
        op.set_param_sets(1, 1, o["w"][0].numel(), 0, N, 0, Ctl())      # item j reads image j and bias row j
    Kp, Np = (K + 31) // 32 * 32, (N + 31) // 32 * 32
    img = (op.packed_fwd if orient == "fwd" else op.packed_dgrad).view(torch.bfloat16)
    assert img.numel() == nw * 27 * Kp * Np      # bf16 images [T][Kp / 8][Np][8]
    img.view(nw, 27, Kp // 8, Np, 8)[:, :, K // 8:] = 1.0
    return op


def _run_variants(op, o, name, want, x_nl=None):
    """{variant: (whole y tensor, statistics rows or None, route)} under the options as they are; asserts what the queries say
    first."""
    from multimodal_tta_amd import ops
    fwd = o["orient"] == "fwd"
    ypad, apad = SHAPES_ALL[name][5:7]
    desc, packed = (op.d_fwd, op.packed_fwd) if fwd else (op.d_dgrad, op.packed_dgrad)
    xd, out = o["x"], {}
    for variant, (fused, accumulate) in VARIANTS.items():
        y, whole = _wide(cl_bf16(o["y0"] if accumulate else torch.full_like(o["y0"], SENTINEL)), ypad, SENTINEL)
        add = _wide(cl_bf16(o["res"]), apad, SENTINEL)[0] if fused else None
        st = torch.full((op.plan(desc, xd, y).stats_rows, 2, y.shape[-1]), float("nan"), device="cuda") if fwd else None
        args = (desc, ops.desc_cl(xd), ops.desc_cl(y))
        kw = dict(x_nl=x_nl.struct() if x_nl is not None else None, add=ops.desc_cl(add) if fused else None,
                  accumulate=1 if accumulate else 0, stats=ops.ptr(st))
        assert _query("mmtta_conv_cls8_pipelined", *args, **kw) == (0 if x_nl is not None else 1), f"{variant}: mmtta_conv_cls8_pipelined"
        assert _query("mmtta_conv_cls8_lean_epilogue", *args, **kw) == want, f"{variant}: mmtta_conv_cls8_lean_epilogue"
        route = _query("mmtta_conv_route", *args, **kw)
        op._run(desc, packed, xd, x_nl, o["bias"] if fwd else None, y, accumulate, st, add, None)
        out[variant] = (whole, st, route)
    torch.cuda.synchronize()
    return out


def _compare(what, o, name, x_nl=None, want_on=1):
    got = {}
    for bit in (0, 1):
        with cg.pinned({OPT_CLS_MIN: 1, OPT_PIPE: 1, OPT_LEAN: bit}):
            got[bit] = _run_variants(_op(o, name), o, name, want_on if bit else 0, x_nl)
    ypad = SHAPES_ALL[name][5]
    for variant, (ya, sa, ra) in got[0].items():
        yb, sb, rb = got[1][variant]
        assert ra == rb == ROUTE_CLS_FUSED, f"{what}: {variant}: routes {ra}, {rb}"
        assert torch.isfinite(ya.float()).all(), f"{what}: {variant}: the reference kernel left non-finite values"
        n_y = ya.shape[-1] - ypad
        if not VARIANTS[variant][1]:
            assert not (ya[..., :n_y] == SENTINEL).all(dim=-1).any(), f"{what}: {variant}: the reference kernel left a voxel unwritten"
        if ypad:
            assert (ya[..., n_y:] == SENTINEL).all(), f"{what}: {variant}: the reference kernel wrote behind y's channels"
        assert torch.equal(ya, yb), f"{what}: {variant}: outputs differ, max |diff| {(ya.float() - yb.float()).abs().max().item():.3e}"
        if sa is not None:
            assert torch.isfinite(sa).all() and torch.equal(sa, sb), f"{what}: {variant}: statistics rows differ"


@GPU
@pytest.mark.parametrize("form,name", CASES)
def test_the_lean_epilogue_equals_the_pipelined_kernel(form, name):
    before = cg.current_options(cg.GEOMETRY_KEYS + (OPT_PIPE, OPT_LEAN))
    _compare(f"{form} {name}", _operands(form, name), name)
    assert cg.current_options(cg.GEOMETRY_KEYS + (OPT_PIPE, OPT_LEAN)) == before


@GPU
def test_a_call_under_a_norm_on_load_keeps_its_kernel():
    from multimodal_tta_amd import ops
    o = _operands("convT-fwd", "K40-partial")
    g = torch.Generator().manual_seed(5)
    sc, sh = (torch.rand(40, generator=g) + 0.5).cuda(), (torch.randn(40, generator=g) * 0.3).cuda()
    _compare("convT-fwd under a norm-on-load", o, "K40-partial", x_nl=ops.NL(sc, sc, relu=True, scale=sc, shift=sh), want_on=0)


@GPU
@pytest.mark.parametrize("form", FORMS)
def test_a_channel_count_that_is_no_multiple_of_8_keeps_its_kernel(form):
    """36 produced channels in rows of 40 (and the add likewise): route 15 admits 4-channel groups, the lean epilogue's lane
    pairs need 8."""
    _compare(f"{form} 36 channels", _operands(form, "N36"), "N36", want_on=0)
