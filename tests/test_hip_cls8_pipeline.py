"""The pipelined class-fused stride-2 kernel (MMTTA_OPT_CLS8_PIPELINE, option 20: igemm_cls8_pipe_kernel) against
igemm_cls8_raw_kernel on the same tensors in the same process: option 20 at 0, then at 1.  The pipelined kernel fetches the
weight image of channel stage k + 1 by direct global-to-LDS loads into a second LDS image while stage k multiplies and requests
the box items a stage ahead; the MFMAs, their operands, their order and the epilogue are the raw kernel's, so every comparison
- outputs, statistics rows, accumulated / fused-add destinations - is torch.equal and needs no tolerance.
mmtta_conv_cls8_pipelined must say 1 for the second run and mmtta_conv_route 15 both times.

Both forms: ConvTranspose3d forward (K = cin gathered, N = cout produced) and the input gradient of a stride-2 Conv3d (K = cout,
N = cin), on the coarse grid of the form.  The shapes are the smallest that reach every path of the new code:
  stages     coarse 4 x 4 x 8 (one tile); K = 16: the prologue alone; K = 32, 48, 64: both images, image 0 again; K = 24, 40: a
             partial last stage, whose chunk mask has to blank the re-read chunk (made visible as in test_hip_raw_staging.py:
             large values in the last valid chunk, ones in the image rows behind K)
  border     coarse 5 x 3 x 9: partial tiles on every axis; 8 x 4 x 8: an interior face between two tiles
  columns    N = 64 (two column groups), 24 and 40 (columns past N; at 40 a column block of 8)
  batching   batch 1 and 3, one parameter set and one per item (weights and bias)
Every case runs plain (a forward: bias + statistics rows) and with accumulate plus a fused add.  One refused call - a
norm-on-load on x - must report 0 from the query and give the same result under both settings."""
import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl_bf16

GPU = pytest.mark.gpu
OPT_PIPE, OPT_CLS_MIN = 20, 12
ROUTE_CLS_FUSED = 15
BIG = 2.0 ** 40       # bf16-representable; the squares the statistics rows sum stay far inside fp32
TILE, RAGGED, FACE = (4, 4, 8), (5, 3, 9), (8, 4, 8)

# name: (K, N, coarse extent, batch, a parameter set per item)
SHAPES = {
    "one-stage": (16, 32, TILE, 1, False),
    "K32": (32, 32, TILE, 1, False),
    "K48": (48, 32, TILE, 1, False),
    "K64": (64, 32, TILE, 1, False),
    "K24-partial": (24, 32, TILE, 1, False),
    "K40-partial": (40, 32, TILE, 1, False),
    "ragged": (32, 32, RAGGED, 1, False),
    "face": (32, 32, FACE, 1, False),
    "N64": (32, 64, TILE, 1, False),
    "N24": (32, 24, TILE, 1, False),
    "N40": (32, 40, TILE, 1, False),
    "batch1-sets": (32, 32, RAGGED, 1, True),
    "batch3": (32, 32, RAGGED, 3, False),
    "batch3-sets": (40, 40, RAGGED, 3, True),
}
FORMS = ("convT-fwd", "s2-dgrad")


def _case(form, name):
    K, N, grid, n, _ = SHAPES[name]
    if form == "convT-fwd":
        return cg.case(f"pipe_{form}_{name}", K, N, 3, 2, True, (n,) + grid), "fwd"
    return cg.case(f"pipe_{form}_{name}", N, K, 3, 2, False, (n,) + tuple(2 * v for v in grid)), "dgrad"      # dy = grid


_query = cg.query


def test_shapes_are_small():
    assert all(max(grid) <= 9 and n <= 3 and max(K, N) <= 64 for K, N, grid, n, _ in SHAPES.values())


def _operands(form, name):
    c, orient = _case(form, name)
    K, N, grid, n, per_item = SHAPES[name]
    g = torch.Generator().manual_seed(20 + sum(ord(ch) for ch in c.name))
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
    K, N, _, n, per_item = SHAPES[name]
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


def _run_forms(op, o, want, x_nl=None):
    """{form: (y, statistics rows or None, route)} under the options as they are; asserts what the query says first."""
    from multimodal_tta_amd import ops
    fwd = o["orient"] == "fwd"
    desc, packed = (op.d_fwd, op.packed_fwd) if fwd else (op.d_dgrad, op.packed_dgrad)
    xd, out = o["x"], {}
    for form in ("plain", "accumulate + fused add"):
        fused = form != "plain"
        y = cl_bf16(o["y0"] if fused else torch.zeros_like(o["y0"]))
        add = cl_bf16(o["res"]) if fused else None
        st = torch.full((op.plan(desc, xd, y).stats_rows, 2, y.shape[-1]), float("nan"), device="cuda") if fwd else None
        args = (desc, ops.desc_cl(xd), ops.desc_cl(y))
        kw = dict(x_nl=x_nl.struct() if x_nl is not None else None, add=ops.desc_cl(add) if fused else None,
                  accumulate=1 if fused else 0, stats=ops.ptr(st))
        assert _query("mmtta_conv_cls8_pipelined", *args, **kw) == want, f"{form}: mmtta_conv_cls8_pipelined"
        route = _query("mmtta_conv_route", *args, **kw)
        op._run(desc, packed, xd, x_nl, o["bias"] if fwd else None, y, fused, st, add, None)
        out[form] = (y, st, route)
    torch.cuda.synchronize()
    return out


def _compare(what, o, name, x_nl=None, want_on=1):
    got = {}
    for bit in (0, 1):
        with cg.pinned({OPT_CLS_MIN: 1, OPT_PIPE: bit}):
            got[bit] = _run_forms(_op(o, name), o, want_on if bit else 0, x_nl)
    for form, (ya, sa, ra) in got[0].items():
        yb, sb, rb = got[1][form]
        assert ra == rb == ROUTE_CLS_FUSED, f"{what}: {form}: routes {ra}, {rb}"
        assert torch.isfinite(ya.float()).all(), f"{what}: {form}: the raw kernel left non-finite values"
        assert torch.equal(ya, yb), f"{what}: {form}: outputs differ, max |diff| {(ya.float() - yb.float()).abs().max().item():.3e}"
        if sa is not None:
            assert torch.isfinite(sa).all() and torch.equal(sa, sb), f"{what}: {form}: statistics rows differ"


@GPU
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("form", FORMS)
def test_the_pipelined_kernel_equals_the_raw_kernel(form, name):
    before = cg.current_options(cg.GEOMETRY_KEYS + (OPT_PIPE,))
    _compare(f"{form} {name}", _operands(form, name), name)
    assert cg.current_options(cg.GEOMETRY_KEYS + (OPT_PIPE,)) == before


@GPU
def test_a_call_under_a_norm_on_load_keeps_its_kernel():
    from multimodal_tta_amd import ops
    o = _operands("convT-fwd", "K40-partial")
    g = torch.Generator().manual_seed(5)
    sc, sh = (torch.rand(40, generator=g) + 0.5).cuda(), (torch.randn(40, generator=g) * 0.3).cuda()
    _compare("convT-fwd under a norm-on-load", o, "K40-partial", x_nl=ops.NL(sc, sc, relu=True, scale=sc, shift=sh), want_on=0)
