"""The lean kernels of the thin full-resolution convolutions (MMTTA_OPT_THIN_LEAN, option 18: bit 0 chan_mfma_lean_kernel,
bit 1 upconv8_lean_kernel) against the plain kernels on the same tensors in the same process: option 18 at 0, then at its
default.  The lean kernels run the same MFMAs on the same operands, add bias and the fused add in the same order, round the
same fp32 value to bf16 and sum the statistics in the same order, so every comparison - outputs and statistics rows - is
torch.equal and needs no tolerance.  mmtta_conv_thin_lean must name the lean kernel of the second run and mmtta_conv_route the
same route under both settings.

Shapes come from the tiles, not from the workload: one tile (4 x 4 x 8 output voxels of the thin-K convolution, coarse voxels
of the up-convolution), one voxel more along z, y and x in turn (partial tiles on every border), two tiles along x, and for
the up-convolution one grid of 5 x 6 x 5 tiles, more than the 128 persistent workgroups of an item.

What a stage has to blank by itself is made visible: the planes next to the out-of-range voxels hold 2^40 (the loaders read
them again for the halo), a few inputs are -0.0, and for K < 4 the pad lanes of the 8-byte voxels hold 3 while the weight
fragments behind K - zeros in a real image - are set to 1 for both runs, so that anything staged there reaches the result.
"""
import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl, cl_bf16

GPU = pytest.mark.gpu
OPT_LEAN = 18
ROUTE_DIRECT, ROUTE_THIN = 6, 13
LEAN_THIN, LEAN_UPCONV = 1, 2
BIG = 2.0 ** 40       # bf16-representable; the squares the statistics rows sum stay far inside fp32
TILE = (4, 4, 8)
GRIDS = {"tile": TILE, "z+1": (5, 4, 8), "y+1": (4, 5, 8), "x+1": (4, 4, 9), "2x": (4, 4, 16)}
UPCONV_BIG = (20, 24, 40)      # 5 x 6 x 5 = 150 tiles: a persistent workgroup walks more than one


_query = cg.query


def _gen(*key):
    return torch.Generator().manual_seed(1800 + sum((i + 1) * int(v) for i, v in enumerate(key)))


def _with_borders(x, g):
    """x (NCDHW) with a few -0.0 entries and its outermost planes scaled to 2^40."""
    x = x.clone()
    x[torch.rand(x.shape, generator=g) > 0.9] = -0.0
    border = torch.zeros(x.shape[2:], dtype=torch.bool)
    for dim in (0, 1, 2):
        border.index_fill_(dim, torch.tensor([0, x.shape[2 + dim] - 1]), True)
    x[:, :, border] *= BIG
    assert torch.signbit(x[x == 0]).any()
    return x


def _thin_bf16(x, pad_value=3.0):
    """NCDHW cpu fp32 (<= 4 channels) -> bf16-stored channels-last cuda view with 8-byte voxels; the pad lanes hold `pad_value`."""
    n, c, d, h, w = x.shape
    buf = torch.full((n, d, h, w, 4), pad_value, dtype=torch.bfloat16, device="cuda")
    buf[..., :c] = x.permute(0, 2, 3, 4, 1).to(torch.bfloat16).cuda()
    view = buf[..., :c]
    view._mmtta_owns_pad = True
    return view


def _sets_op(cin, cout, transposed, w, n, per_item):
    """ConvOp of bf16 precision; per_item: batch item j reads image j and bias row j."""
    from multimodal_tta_amd import ops

    class Ctl:
        use_sets = True

    sets = n if per_item else 1
    op = ops.ConvOp(cin, cout, 3, 2, transposed, "cuda", dtype=ops.BF16, n_sets=sets)
    for j in range(sets):
        op.pack(w[j].cuda().contiguous(), j)
    if per_item:
        op.set_param_sets(1, 1, w[0].numel(), 0, 64, 0, Ctl())      # (bias rows of 64 floats)
    return op


def _ones_behind_k(op, dgrad, K, N):
    """The B fragments of the thin-K kernel, entry (s2 * NB + nb, lane): 8 values k = (tap offset e >> 2, channel e & 3); the
    channels behind K become 1 (tap 27, the zero pad of the last k-step, stays 0)."""
    NB = N // 32
    for j in range(op.n_sets):
        img = op.packed_image(dgrad, j)
        frag = img[img.numel() - 7 * NB * 64 * 16:].view(torch.bfloat16).view(7, NB, 2, 32, 2, 4)      # [s2][nb][h][r][tap][ch]
        frag[..., K:] = 1.0
        frag[6, :, 1, :, 1, :] = 0.0
        torch.cuda.synchronize()


def _nl(sc, sh, leaky=False):
    from multimodal_tta_amd import ops
    sc, sh = sc.cuda(), sh.cuda()
    if leaky:
        return ops.NL(sc, sc, scale=sc, shift=sh, act=ops.ACT_LEAKY_RELU, negative_slope=0.1)
    return ops.NL(sc, sc, relu=True, scale=sc, shift=sh)


def _launch(op, desc, packed, x, x_nl, bias, y, stats_rows, add, add_nl, accumulate, want_lean, want_route, what):
    from multimodal_tta_amd import ops
    st = torch.full((stats_rows, 2, y.shape[-1]), float("nan"), device="cuda") if stats_rows else None
    args = (desc, ops.desc_cl(x), ops.desc_cl(y))
    kw = dict(x_nl=x_nl.struct() if x_nl is not None else None, add=ops.desc_cl(add) if add is not None else None,
              add_nl=add_nl.struct() if add_nl is not None else None, accumulate=1 if accumulate else 0, stats=ops.ptr(st))
    assert _query("mmtta_conv_thin_lean", *args, **kw) == want_lean, f"{what}: mmtta_conv_thin_lean"
    route = _query("mmtta_conv_route", *args, **kw)
    assert route == want_route, f"{what}: route {route}"
    op._run(desc, packed, x, x_nl, bias, y, accumulate, st, add, add_nl)
    return y, st


def _compare(run, lean_bit, what):
    """run(want_lean) -> {form: (y, statistics rows or None)} under option 18 = 0 and at its default."""
    before = cg.current_options((OPT_LEAN,))
    got = {}
    for bits in (0, 3):
        with cg.pinned({OPT_LEAN: bits}):
            got[bits] = run(lean_bit if bits else 0)
    torch.cuda.synchronize()
    for form, (ya, sa) in got[0].items():
        yb, sb = got[3][form]
        assert torch.isfinite(ya.float()).all(), f"{what}: {form}: the plain kernel left non-finite values"
        assert torch.equal(ya, yb), f"{what}: {form}: outputs differ, max |diff| {(ya.float() - yb.float()).abs().max().item():.3e}"
        if sa is not None:
            assert torch.isfinite(sa).all() and torch.equal(sa, sb), f"{what}: {form}: statistics rows differ"
    assert cg.current_options((OPT_LEAN,)) == before


# ----------------------------------------------------------------------------- the thin-K convolution
def _thin_forward_case(K, grid, n, per_item, N=32):
    g = _gen(K, N, n, per_item, *grid)
    rnd = lambda *s: torch.randn(*s, generator=g)
    ext = tuple(2 * v - 1 for v in grid)                 # odd extents: the halo crosses the high border
    x = _thin_bf16(_with_borders(rnd(n, K, *ext) * 1.5 + 0.25, g))
    sets = n if per_item else 1
    w = rnd(sets, N, K, 3, 3, 3) * (K * 27) ** -0.5
    bias = torch.zeros(sets, 64)
    bias[:, :N] = rnd(sets, N)
    bias = bias.cuda()
    res = cl_bf16(rnd(n, N, *grid) * 1.5 + 0.2)
    rsc, rsh = rnd(n * N).abs() + 0.5, rnd(n * N) * 0.3
    xsc, xsh = rnd(n * K).abs() + 0.5, rnd(n * K) * 0.3
    y0 = rnd(n, N, *grid)

    def run(want_lean):
        op = _sets_op(K, N, False, w, n, per_item)
        _ones_behind_k(op, False, K, N)
        out = {}
        fresh = lambda: cl_bf16(torch.zeros(n, N, *grid))
        rows = op.stats_rows(x, fresh())
        go = lambda name, y, lean, **k: out.__setitem__(name, _launch(
            op, op.d_fwd, op.packed_fwd, x, k.pop("x_nl", None), bias, y, k.pop("rows", rows), k.pop("add", None), k.pop("add_nl", None),
            k.pop("accumulate", False), lean, ROUTE_THIN, f"thin-K {K}->{N} {grid} x{n}: {name}"))
        go("bias + statistics", fresh(), want_lean)
        go("fused add under a norm-on-load + statistics (the residual form)", fresh(), want_lean, add=res, add_nl=_nl(rsc, rsh))
        go("norm-on-load on x + statistics", fresh(), want_lean, x_nl=_nl(xsc, xsh))
        go("norm-on-load on x, fused add under its own + statistics", fresh(), want_lean, x_nl=_nl(xsc, xsh), add=res, add_nl=_nl(rsc, rsh))
        # these stay on chan_mfma_kernel
        go("accumulate", cl_bf16(y0), 0, accumulate=True)
        go("fp32-stored output", cl(torch.zeros(n, N, *grid)), 0)
        go("fused add under a LeakyReLU", fresh(), 0, add=res, add_nl=_nl(rsc, rsh, leaky=True))
        return out

    return run


@GPU
@pytest.mark.parametrize("K", [2, 3, 4])
def test_thin_k_forward_at_stride_2_equals_the_plain_kernel(K):
    for name, grid in GRIDS.items():
        for n, per_item in ((1, False), (3, False), (3, True)):
            _compare(_thin_forward_case(K, grid, n, per_item), LEAN_THIN, f"thin-K forward K={K} {name} x{n} sets={per_item}")


@GPU
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_thin_k_forward_into_64_channels_equals_the_plain_kernel(K):
    """The two-column-block kernels (NB = 2) with everything a forward carries: bias, statistics rows, a norm-on-load on x, the
    residual form.  K = 1 from a bf16-stored x exists with 64 columns only."""
    for name, grid in GRIDS.items():
        for n, per_item in ((1, False), (3, True)):
            _compare(_thin_forward_case(K, grid, n, per_item, N=64), LEAN_THIN, f"thin-K forward {K}->64 {name} x{n} sets={per_item}")


@GPU
def test_the_64_column_form_equals_the_plain_kernel():
    """The input gradient of a 64 -> 3 transposed convolution: dy bf16-stored with 8-byte voxels, 3 -> 64 gathered at stride 2."""
    K, N = 3, 64
    for name, grid in GRIDS.items():
        for n, per_item in ((1, False), (3, False), (3, True)):
            g = _gen(64, n, per_item, *grid)
            rnd = lambda *s: torch.randn(*s, generator=g)
            dy = _thin_bf16(_with_borders(rnd(n, K, *(2 * v for v in grid)), g))
            sets = n if per_item else 1
            w = rnd(sets, N, K, 3, 3, 3) * (N * 27) ** -0.5
            add = cl_bf16(rnd(n, N, *grid))

            def run(want_lean):
                op = _sets_op(N, K, True, w, n, per_item)
                _ones_behind_k(op, True, K, N)
                what = f"64-column form {name} x{n} sets={per_item}"
                fresh = lambda: cl_bf16(torch.zeros(n, N, *grid))
                mk = lambda y, lean, add=None: _launch(op, op.d_dgrad, op.packed_dgrad, dy, None, None, y, 0, add, None, False, lean,
                                                       ROUTE_THIN, what)
                return {"plain": mk(fresh(), want_lean), "fused add": mk(fresh(), want_lean, add)}

            _compare(run, LEAN_THIN, f"64-column form {name} x{n} sets={per_item}")


# ----------------------------------------------------------------------------- the gather-GEMM up-convolution
@GPU
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [32, 64])
def test_upconv8_equals_the_plain_kernel(K, R):
    from multimodal_tta_amd import ops
    grids = dict(GRIDS, grid=UPCONV_BIG)
    for name, grid in grids.items():
        for n in (1, 3):
            g = _gen(K, R, n, *grid)
            rnd = lambda *s: torch.randn(*s, generator=g)
            x = cl_bf16(_with_borders(rnd(n, K, *grid) * 1.5 + 0.25, g))
            w = rnd(1, K, R, 3, 3, 3) * (K * 8) ** -0.5
            bias = rnd(R).cuda()
            fine = tuple(2 * v for v in grid)
            res = ops.to_cl(rnd(n, R, *fine).cuda())
            sc, sh = rnd(n * K).abs() + 0.5, rnd(n * K) * 0.3

            def run(want_lean):
                op = _sets_op(K, R, True, w, n, False)
                fresh = lambda: ops.new_cl(n, *fine, R, "cuda", ldc=4, zero=True)
                rows = op.stats_rows(x, fresh())
                what = f"upconv8 {K}->{R} {name} x{n}"
                mk = lambda lean, x_nl=None, add=None: _launch(op, op.d_fwd, op.packed_fwd, x, x_nl, bias, fresh(), rows, add, None, False,
                                                               lean, ROUTE_DIRECT, what)
                return {"bias + statistics": mk(want_lean), "fused add + statistics": mk(want_lean, add=res),
                        "under a norm-on-load (the plain stage)": mk(0, x_nl=_nl(sc, sh))}

            _compare(run, LEAN_UPCONV, f"upconv8 {K}->{R} {name} x{n}")
