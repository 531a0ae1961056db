"""Raw staging in the transposed-read weight gradient (MMTTA_OPT_RAW_STAGING, option 16, bit 1: wgrad_tr_raw_kernel) against
wgrad_tr_kernel on the same tensors in the same process: option 16 at 0, then at its default.  The raw forms exist for the
stride-2 layers, convolutions and transposed convolutions (the stride-1 forms measured slower than their twins,
profiles/raw_staging_ab.md, and are not built: the query says 0 there and both settings run one kernel).  With x and dy both
bf16-stored, dy - which never takes a transform - and, next to it, an x whose norm-on-load is the identity go to LDS as
loaded instead of through unpack / (x * 1 + 0, max with -inf) / repack, which returns the bits it was given.  The MFMAs,
their operands and their order are the same: the workspace (slabs, bias rows), the reduced dw and db, and everything the
fused update writes are compared with torch.equal.  mmtta_conv_wgrad_stages_raw must name the operands that went raw: both
for an identity x, dy alone for an x under a real norm-on-load.

Shapes come from the kernel's tile (2 x 4 x 8 voxels of the coarse tensor at stride 2; 4 x 8 x 8 of dy at stride 1): one
tile, one voxel more along each axis in turn, two tiles along x; batch 1 and 2; every geometry of conv_geometry.GEOMETRIES.
"""
import ctypes as C

import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl_bf16

GPU = pytest.mark.gpu
OPT_RAW = 16
X_RAW, DY_RAW = 1, 2
W_TR = (7, 8)      # mmtta_conv_wgrad_kernel: wgrad_tr_kernel at stride 1 / 2

# name: (cin, cout, stride, transposed, tile of the coarse tensor)
KINDS = {
    "s2-32-32": (32, 32, 2, False, (2, 4, 8)),          # one dense column block
    "s2-32-64": (32, 64, 2, False, (2, 4, 8)),          # paired column blocks
    "convT-128-32": (128, 32, 2, True, (2, 4, 8)),      # the module input is the dense operand, four column blocks of it
    "convT-32-32": (32, 32, 2, True, (2, 4, 8)),        # ... one
    "s2-40-32": (40, 32, 2, False, (2, 4, 8)),          # Cg = 40: a column block with one whole chunk and three past the end
    "s2-32-40": (32, 40, 2, False, (2, 4, 8)),          # Cd = 40
    "convT-40-32": (40, 32, 2, True, (2, 4, 8)),        # Cd = 40 on the module-input side
    "s1-32-32": (32, 32, 1, False, (4, 8, 8)),          # stride 1: no raw form, one kernel under both settings
    "s1-64-64": (64, 64, 1, False, (4, 8, 8)),
}
RAW_KINDS = [k for k, v in KINDS.items() if v[2] == 2]


def _extents(kind):
    tz, ty, tx = KINDS[kind][4]
    return {"tile": (tz, ty, tx), "z+1": (tz + 1, ty, tx), "y+1": (tz, ty + 1, tx), "x+1": (tz, ty, tx + 1), "2x": (tz, ty, 2 * tx)}


def _x_dhw(kind, grid):
    cin, cout, stride, transposed, _ = KINDS[kind]
    return tuple(grid) if (transposed or stride == 1) else tuple(2 * v for v in grid)


def _stages_raw(desc, x, dy, x_nl=None):
    from multimodal_tta_amd import _lib
    return int(_lib.load().mmtta_conv_wgrad_stages_raw(C.byref(desc), C.byref(x), C.byref(x_nl) if x_nl is not None else None, C.byref(dy)))


# ----------------------------------------------------------------------------- without a GPU
def test_query_names_the_raw_operands():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_FWD, CONVT_FWD, F32, ConvDesc, NormOnLoad
    X, Y, P = 1 << 30, 1 << 40, 1 << 21
    e = (8, 8, 16)
    t = lambda base, c, dhw=e, bf=True: cg._fake_tensor(_lib, base, 2, c, dhw, bf)
    real = NormOnLoad(scale=P, shift=P, relu=1)
    with cg.pinned({OPT_RAW: 3, 11: 1}):
        ty = lambda c: t(Y, c, (4, 4, 8))      # dy of a stride-2 convolution of e
        for cin, cout in ((32, 32), (32, 64), (40, 32), (32, 40)):
            d = ConvDesc(CONV_FWD, 3, 2, cin, cout, BF16)
            assert _lib.load().mmtta_conv_wgrad_kernel(C.byref(d), C.byref(t(X, cin)), C.byref(ty(cout))) in W_TR
            assert _stages_raw(d, t(X, cin), ty(cout)) == X_RAW | DY_RAW
            assert _stages_raw(d, t(X, cin), ty(cout), NormOnLoad()) == X_RAW | DY_RAW
            assert _stages_raw(d, t(X, cin), ty(cout), real) == DY_RAW, "x under a real norm-on-load: dy alone"
            assert _stages_raw(d, t(X, cin), ty(cout), _lib.norm_on_load(relu=True)) == DY_RAW, "activation-only norm-on-load"
            assert _stages_raw(d, t(X, cin), ty(cout), NormOnLoad(mean=P, rstd=P)) == DY_RAW
            d1 = ConvDesc(CONV_FWD, 3, 1, cin, cout, BF16)
            assert _lib.load().mmtta_conv_wgrad_kernel(C.byref(d1), C.byref(t(X, cin)), C.byref(t(Y, cout))) in W_TR
            assert _stages_raw(d1, t(X, cin), t(Y, cout)) == 0, "stride 1: no raw form"
        dT = ConvDesc(CONVT_FWD, 3, 2, 128, 32, BF16)
        assert _stages_raw(dT, t(X, 128), t(Y, 32, (16, 16, 32))) == X_RAW | DY_RAW
        assert _stages_raw(dT, t(X, 128), t(Y, 32, (16, 16, 32)), real) == DY_RAW
        d = ConvDesc(CONV_FWD, 3, 2, 64, 64, BF16)
        assert _stages_raw(d, t(X, 64), ty(64)) == X_RAW | DY_RAW
        assert _stages_raw(d, t(X, 64), t(Y, 64, (4, 4, 8), bf=False)) == 0, "fp32-stored dy"
        assert _stages_raw(d, t(X, 64, bf=False), t(Y, 64, (4, 4, 8), bf=False)) == 0, "fp32-stored x and dy"
        assert _stages_raw(ConvDesc(CONV_FWD, 3, 2, 36, 64, BF16), t(X, 36), ty(64)) == DY_RAW, "Cin = 36: x keeps the transform"
        assert _stages_raw(ConvDesc(CONV_FWD, 3, 2, 64, 36, BF16), t(X, 64), ty(36)) == 0, "Cout = 36: dy is not raw, so nothing is"
        assert _stages_raw(ConvDesc(CONV_FWD, 3, 2, 64, 64, F32), t(X, 64, bf=False), t(Y, 64, (4, 4, 8), bf=False)) == 0, "fp32 precision"
        assert _stages_raw(ConvDesc(CONV_FWD, 1, 1, 64, 64, BF16), t(X, 64), t(Y, 64)) == 0, "1x1x1: another kernel"
        for bits, want in ((0, 0), (1, 0), (2, X_RAW | DY_RAW)):
            with cg.pinned({OPT_RAW: bits}):
                assert _stages_raw(d, t(X, 64), ty(64)) == want, f"option 16 = {bits}"
        with cg.pinned({11: 0}):
            assert _stages_raw(d, t(X, 64), ty(64)) == 0, "the fp32-operand kernel (option 11 = 0)"


# ----------------------------------------------------------------------------- on the GPU
def _operands(kind, grid, n):
    cin, cout, stride, transposed, _ = KINDS[kind]
    c = cg.case(f"rawwg_{kind}_{n}x" + "x".join(map(str, grid)), cin, cout, 3, stride, transposed, (n,) + _x_dhw(kind, grid))
    g = torch.Generator().manual_seed(4099 + sum(ord(ch) for ch in c.name))
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(n, cin, *c.shape[1:]) * 1.5 + 0.25
    gy = rnd(n, cout, *cg.out_dhw(c))
    x[rnd(*x.shape) > 1.2] = -0.0
    gy[rnd(*gy.shape) > 1.2] = -0.0
    return c, cl_bf16(x), cl_bf16(gy), (rnd(n * cin).abs() + 0.5).cuda(), (rnd(n * cin) * 0.3).cuda()


def _wgrad_all(c, x, gy, sc, sh, want_bits):
    """{form: (workspace, dw, db)} under the options as they are, for an identity x and an x under a real norm-on-load, with
    and without a bias gradient; asserts what the query says first."""
    from multimodal_tta_amd import _lib, ops
    op = ops.ConvOp(c.cin, c.cout, 3, c.stride, c.transposed, "cuda", dtype=ops.BF16)
    tx, tdy = ops.desc_cl(x), ops.desc_cl(gy)
    assert int(_lib.load().mmtta_conv_wgrad_kernel(C.byref(op.d_fwd), C.byref(tx), C.byref(tdy))) in W_TR
    need = int(_lib.load().mmtta_conv_wgrad_workspace_bytes(C.byref(op.d_fwd), C.byref(tx), C.byref(tdy)))
    out = {}
    for nl_name, nl in (("identity x", None), ("norm-on-load x", ops.NL(sc, sc, relu=True, scale=sc, shift=sh))):
        want = want_bits if nl is None else (want_bits & DY_RAW)
        assert _stages_raw(op.d_fwd, tx, tdy, nl.struct() if nl is not None else None) == want, f"{nl_name}: mmtta_conv_wgrad_stages_raw"
        for with_db in (False, True):
            ws = ops.Workspace.get(need, x.device)
            ws.view(-1)[:] = 0
            dw = torch.full(op.weight_shape(), float("nan"), device="cuda")
            db = torch.full((c.cout,), float("nan"), device="cuda") if with_db else None
            op.wgrad(x, nl, gy, dw, db)
            torch.cuda.synchronize()
            out[f"{nl_name}, {'dw + db' if with_db else 'dw'}"] = (ops.Workspace.get(need, x.device).view(-1).clone(), dw, db)
    return out


@GPU
@pytest.mark.parametrize("n", [1, 2], ids=["batch1", "batch2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_raw_wgrad_equals_the_transform_kernel(kind, n):
    before = cg.current_options(cg.GEOMETRY_KEYS + (OPT_RAW,))
    for ext, grid in _extents(kind).items():
        c, x, gy, sc, sh = _operands(kind, grid, n)
        for geo in cg.GEOMETRIES:
            vals = cg.geometry_values(geo)
            got = {}
            for bits in (0, 3):
                with cg.pinned({**vals, OPT_RAW: bits}):
                    got[bits] = _wgrad_all(c, x, gy, sc, sh, (X_RAW | DY_RAW) if (bits and kind in RAW_KINDS) else 0)
            assert len(got[0]) == 4
            for form, (wa, dwa, dba) in got[0].items():
                wb, dwb, dbb = got[3][form]
                what = f"{kind} {ext} x{n} {geo}: {form}"
                assert torch.isfinite(dwa).all(), f"{what}: the transform kernel left non-finite values"
                assert wa.numel() == wb.numel() and torch.equal(wa, wb), f"{what}: workspaces (slabs, bias rows) differ"
                assert torch.equal(dwa, dwb), f"{what}: dw differs, max |diff| {(dwa - dwb).abs().max().item():.3e}"
                if dba is not None:
                    assert torch.isfinite(dba).all() and torch.equal(dba, dbb), f"{what}: db differs"
    assert cg.current_options(cg.GEOMETRY_KEYS + (OPT_RAW,)) == before


@GPU
@pytest.mark.parametrize("kind", ["s2-32-32", "s2-32-64", "convT-128-32"])
def test_raw_wgrad_through_the_fused_update(kind):
    """mmtta_conv_wgrad_update_sets (tests/test_hip_fused_update.py shows the call) on the raw kernel against the transform
    kernel: parameters, moments and both repacked images after two steps, bit for bit."""
    from multimodal_tta_amd import ops
    if not ops.fused_update_enabled():
        pytest.fail("MMTTA_FUSED_UPDATE=0 is set: the fused entry point is switched off")
    cin, cout, stride, transposed, tile = KINDS[kind]
    grid = (tile[0] + 1, tile[1] + 1, 2 * tile[2] + 1)
    c, x, gy, sc, sh = _operands(kind, grid, 2)
    spec = ops.OptimSpec(name="adam", lr=1e-2, weight_decay=5e-2, momentum=0.0)
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    wnum = cin * cout * 27
    boff = (wnum + 3) // 4 * 4
    total = boff + (cout + 3) // 4 * 4
    g = torch.Generator().manual_seed(31 + cin + cout)
    P0 = torch.zeros(1, total)
    P0[:, :wnum] = 0.05 * torch.randn(1, wnum, generator=g)
    P0[:, boff:boff + cout] = 0.05 * torch.randn(1, cout, generator=g)
    res = {}
    for bits in (0, 3):
        with cg.pinned({**cg.geometry_values("inflight4"), OPT_RAW: bits}):
            op = ops.ConvOp(cin, cout, 3, stride, transposed, "cuda", dtype=ops.BF16)
            assert op.plain_bf16_images()
            P, M, V, G = P0.cuda(), torch.zeros(1, total, device="cuda"), torch.zeros(1, total, device="cuda"), torch.zeros(1, total, device="cuda")
            step = torch.zeros(1, dtype=torch.int32, device="cuda")
            op.pack(P[0, :wnum].view(wshape))
            bias_here = not transposed
            sl = slice(boff, boff + cout)
            target = op.update_target(spec, P[0, :wnum], M[0, :wnum], V[0, :wnum], P[0, sl] if bias_here else None,
                                      M[0, sl] if bias_here else None, V[0, sl] if bias_here else None,
                                      None if bias_here else G[0, sl], True, True, step)
            for t in range(2):
                op.wgrad_update(x, None, gy, target)
                step += 1
            torch.cuda.synchronize()
            res[bits] = dict(P=P, M=M, V=V, G=G, fwd=op.packed_fwd, dgrad=op.packed_dgrad)
    assert not torch.equal(res[0]["P"], P0.cuda()), "the step moved no weight"
    for k in res[0]:
        assert torch.isfinite(res[0][k].float()).all() if res[0][k].dtype != torch.uint8 else True
        assert torch.equal(res[0][k], res[3][k]), f"{kind}: {k} differs between the raw and the transform kernel"
