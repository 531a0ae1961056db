"""Shared helpers of tests/test_hip_thin_routes.py: the layers, layouts and forms of the thin and pointwise convolution routes
(6, 13, 16, 17 of mmtta_conv_route; weight-gradient kernels 3, 6, 9, 10), the host-only queries that name the kernel of each
call, and the exact float64 reference (tests/conv_geometry.py).  No test lives here.

A `Layer` is one Conv3d / ConvTranspose3d (a conv_geometry.Case) with the storage of its thin and wide tensors, the options
that select its kernels and the kernel id every form of it is there for.  Each call of a layer - `calls(layer)` - is described
once and turned into descriptors twice: made-up ones (`fake`, for the tests without a GPU) and the real tensors' (`build`); the
GPU test asserts that the two agree field by field before it launches, so the table the CPU test evaluates is the table the
GPU runs."""
import ctypes as C
import functools
from collections import namedtuple

import torch

import conv_geometry as cg
from conv_geometry import (Case, operands, reference, exact_close, stats_close, pinned, ask_plan, ask_wgrad_plan,      # noqa: F401
                           q_bf16, fmaf_relu, nl_operand_mismatch)

# ----------------------------------------------------------------------------- ids (include/mmtta.h)
ROUTE_DIRECT, ROUTE_THIN, ROUTE_PW_SMALL, ROUTE_PW_MFMA = 6, 13, 16, 17
THIN_KERNELS = {1: "direct_conv_kernel", 2: "direct_klane_kernel", 3: "direct_row_kernel", 4: "conv3_mfma4_kernel",
                5: "conv3_mfma4_kernel (thin_bf)", 6: "direct_upconv_kernel", 7: "upconv_mfma_kernel", 8: "upconv8_kernel",
                9: "upconv8_lean_kernel", 10: "pointwise_head_kernel", 11: "direct_chan_kernel", 12: "chan_mfma_kernel",
                13: "chan_mfma_lean_kernel"}
# upconv_mfma_kernel: direct_variant sends every bf16-precision up-convolution whose input has 16-byte rows (fp32: strides in
# multiples of 4, bf16: of 8 elements, base on 16 bytes) to upconv8_kernel, and ops.new_cl / ops.row_pad build no other rows of
# 32 or 64 channels.  It is named here and in DESIGN.md, and left out of the closing assertions.
UNREACHABLE = (7,)
WGRAD_KERNELS = {3: "wgrad_small_kernel", 6: "wgrad_tiny_kernel", 9: "wgrad_tr1_kernel", 10: "wgrad_thin_tr_kernel"}
ERR_UNSUPPORTED = -2
OPT_WGRAD_SLABS, OPT_WGRAD_VEC, OPT_THIN_MFMA, OPT_THIN_LEAN = 5, 11, 13, 18
OPTION_KEYS = cg.GEOMETRY_KEYS + (OPT_WGRAD_VEC, OPT_THIN_MFMA, OPT_THIN_LEAN)
LEAKY_SLOPE = 0.125          # a power of two: slope * v is exact in fp32
PAD = 3.0                    # what the pad lanes of a bf16-stored thin input hold

# ----------------------------------------------------------------------------- layouts
# "f32": fp32-stored, rows padded to 4 channels        "bf16": bf16-stored, rows of 8 channels, or 8-byte voxels for <= 4
# "slice": channel 1 of a 4-channel fp32 tensor (a one-channel view that starts 4 bytes into its 16-byte group)


def row_elems(layout, ch):
    if layout == "bf16" and ch > 4:
        return (ch + 7) // 8 * 8
    return (ch + 3) // 4 * 4


def fake(layout, slot, n, ch, dhw):
    """A made-up descriptor with the strides, alignment and flags `build` gives the real tensor."""
    from multimodal_tta_amd import _lib
    d, h, w = dhw
    sw = row_elems(layout, ch)
    base = (slot + 1) << 32
    if layout == "slice":
        assert ch == 1
        return _lib.Tensor(base + 4, n, 1, d, h, w, d * h * w * 4, 1, h * w * 4, w * 4, 4, _lib.F32, 0)
    flags = _lib.TENSOR_OWNS_PAD if sw != ch else 0
    return _lib.Tensor(base, n, ch, d, h, w, d * h * w * sw, 1, h * w * sw, w * sw, sw, _lib.BF16 if layout == "bf16" else _lib.F32, flags)


def build(layout, t, pad=0.0):
    """NCDHW cpu fp32 -> the channels-last cuda view of that layout; pad lanes hold `pad`."""
    n, ch, d, h, w = t.shape
    sw = row_elems(layout, ch)
    if layout == "slice":
        g = torch.Generator().manual_seed(77)
        buf = torch.randn(n, d, h, w, 4, generator=g).cuda()
        buf[..., 1] = t[:, 0].cuda()
        return buf[..., 1:2]
    buf = torch.full((n, d, h, w, sw), pad, dtype=torch.bfloat16 if layout == "bf16" else torch.float32, device="cuda")
    buf[..., :ch] = t.permute(0, 2, 3, 4, 1).to(buf.dtype).cuda()
    if sw == ch:
        return buf
    view = buf[..., :ch]
    view._mmtta_owns_pad = True
    return view


def same_descriptor(real, made_up):
    """Every field the planners read, the pointer by its place in a 16-byte group."""
    fields = [f for f, _ in real._fields_ if f not in ("ptr", "_pad")]
    return all(int(getattr(real, f)) == int(getattr(made_up, f)) for f in fields) and \
        int(real.ptr or 0) % 16 == int(made_up.ptr or 0) % 16


def query(fn, desc, x, y, x_nl=None, add=None, add_nl=None, accumulate=0, stats=None):
    """One of the host-only queries that take the operands of mmtta_conv_route."""
    from multimodal_tta_amd import _lib
    epi = None
    if add is not None:
        epi = _lib.ConvEpilogue(C.pointer(add), add_nl if add_nl is not None else _lib.norm_on_load())
    return int(getattr(_lib.load(), fn)(C.byref(desc), C.byref(x), C.byref(x_nl) if x_nl is not None else None,
                                        C.byref(epi) if epi is not None else None, C.byref(y), accumulate, stats))


# ----------------------------------------------------------------------------- layers
# dtype: desc.dtype (the precision mode); lo / hi: the layouts of the cin-side and the cout-side tensor (x and y of the
# forward, dx and gy of the input gradient, x and dy of the weight gradient); opts: options pinned around every call.
# fwd: what runs the forms FWD_FORMS in their order, dgrad: DGRAD_FORMS, leaky: the LeakyReLU form (or absent); wgrad: the
# weight-gradient kernel id.  A value 1..13 is an id of mmtta_conv_thin_kernel, 16 / 17 the route, a negative one the error
# the run returns, None a call of another route (an implicit GEMM: tests/test_hip_conv_geometry.py) that is not launched here.
Layer = namedtuple("Layer", "case dtype lo hi opts fwd dgrad leaky wgrad")
FWD_FORMS = ("bias", "bias + statistics", "norm-on-load + fused add + statistics", "accumulate")
DGRAD_FORMS = ("input gradient", "input gradient accumulate")
LEAKY_FORM = "LeakyReLU norm-on-load + fused add + statistics"


def layer(name, cin, cout, k, stride, transposed, shape, dtype, lo, hi, fwd, dgrad=None, leaky=None, wgrad=None, opts=None):
    return Layer(cg.case(name, cin, cout, k, stride, transposed, shape), dtype, lo, hi, dict(opts or {}), tuple(fwd),
                 tuple(dgrad) if dgrad else None, leaky, wgrad)


F, B, S = "f32", "bf16", "slice"
LAYERS = [
    # ---- route 6.  direct_conv_kernel: 256 voxels per workgroup; whatever no other variant takes (K = 8; stride 2)
    layer("direct_8_3", 8, 3, 3, 1, False, (2, 5, 7, 9), "fp32", F, F, fwd=(1, 1, 1, 1), leaky=1),
    layer("direct_s2_3_1", 3, 1, 3, 2, False, (2, 5, 7, 9), "fp32", F, F, fwd=(1, 1, 1, 1), dgrad=(1, 1), wgrad=3),
    # direct_klane_kernel: 64-voxel chunks of a row, K = 32 / 64; the streaming head takes the bare 1x1x1 form of it
    layer("klane_32_3", 32, 3, 3, 1, False, (1, 3, 5, 70), "fp32", F, F, fwd=(2, 2, 2, 2), leaky=2),
    layer("klane_64_2", 64, 2, 3, 1, False, (2, 4, 4, 8), "bf16", B, F, fwd=(2, 2, 2, 2)),
    layer("klane_32_1", 32, 1, 3, 1, False, (2, 4, 4, 8), "fp32", F, F, fwd=(2, 2, 2, 2)),
    layer("klane_1x1_64_4", 64, 4, 1, 1, False, (2, 4, 4, 8), "bf16", B, F, fwd=(2, 2, 2, 2), wgrad=9),
    # (chan_4_32_s2 below runs it as the stride-2 input gradient of a thin-K convolution)
    # direct_row_kernel: K <= 4, 3x3x3 stride 1, rows in pairs
    layer("row_3_3", 3, 3, 3, 1, False, (1, 3, 5, 70), "fp32", F, F, fwd=(3, 3, 3, 3), dgrad=(3, 3), leaky=3, wgrad=6),
    layer("row_1_4", 1, 4, 3, 1, False, (2, 4, 4, 8), "fp32", F, F, fwd=(3, 3, 3, 3), dgrad=(3, 3), wgrad=6),
    # conv3_mfma4_kernel: TZ x 8 x 64 output voxels, TZ = 8 / 4 / 2 (MMTTA_OPT_THIN_MFMA = 1 / 2 / 3)
    layer("mfma4_4_2_tz8", 4, 2, 3, 1, False, (2, 9, 9, 70), "bf16", F, F, fwd=(4, 4, 4, 4), dgrad=(4, 4), leaky=4, wgrad=10,
          opts={OPT_THIN_MFMA: 1}),
    layer("mfma4_2_3_tz4", 2, 3, 3, 1, False, (2, 9, 9, 70), "bf16", F, F, fwd=(4, 4, 4, 4), dgrad=(4, 4), wgrad=10, opts={OPT_THIN_MFMA: 2}),
    layer("mfma4_3_1_tz2", 3, 1, 3, 1, False, (2, 9, 9, 70), "bf16", F, F, fwd=(4, 4, 4, 4), dgrad=(4, 4), opts={OPT_THIN_MFMA: 3}),
    # ... with every thin tensor bf16-stored (thin_bf); MMTTA_OPT_THIN_MFMA = 0 sends the shape back to the row kernel, which
    # writes fp32 only
    layer("mfma4_bf_2_3", 2, 3, 3, 1, False, (2, 9, 9, 70), "bf16", B, B, fwd=(5, 5, 5, 5), dgrad=(5, 5), opts={OPT_THIN_MFMA: 1}),
    layer("mfma4_bf_4_4_tz4", 4, 4, 3, 1, False, (1, 5, 9, 65), "bf16", B, B, fwd=(5, 5, 5, 5), dgrad=(5, 5), opts={OPT_THIN_MFMA: 2}),
    layer("mfma4_off_2_3", 2, 3, 3, 1, False, (2, 4, 4, 8), "bf16", B, B, fwd=(ERR_UNSUPPORTED,) * 4, opts={OPT_THIN_MFMA: 0}),
    # direct_upconv_kernel: one 64-voxel chunk of a coarse row pair (fp32 precision)
    layer("upconv_32_3", 32, 3, 3, 2, True, (1, 3, 5, 70), "fp32", F, F, fwd=(6, 6, 6, 6), dgrad=(11, 11), leaky=6, wgrad=3),
    layer("upconv_64_1", 64, 1, 3, 2, True, (2, 4, 4, 8), "fp32", F, F, fwd=(6, 6, 6, 6)),
    # upconv8_kernel / upconv8_lean_kernel: one coarse 4 x 4 x 8 tile; lean: a bf16-stored x without a transform
    layer("upconv8_64_3", 64, 3, 3, 2, True, (2, 5, 5, 9), "bf16", F, F, fwd=(8, 8, 8, 8), dgrad=(12, 12), leaky=8, wgrad=10),
    layer("upconv8_64_3_bf", 64, 3, 3, 2, True, (2, 5, 5, 9), "bf16", B, F, fwd=(9, 9, 8, 9), leaky=8, wgrad=10),
    layer("upconv8_32_4_bf", 32, 4, 3, 2, True, (2, 5, 5, 9), "bf16", B, F, fwd=(9, 9, 8, 9)),
    layer("upconv8_32_2", 32, 2, 3, 2, True, (2, 5, 5, 9), "bf16", F, F, fwd=(8, 8, 8, 8)),
    layer("upconv8_32_2_bf_plain", 32, 2, 3, 2, True, (2, 5, 5, 9), "bf16", B, F, fwd=(8, 8, 8, 8), opts={OPT_THIN_LEAN: 0}),
    # more than 128 tiles per item: a persistent workgroup walks more than one (5 x 6 x 5 = 150)
    layer("upconv8_32_1_grid", 32, 1, 3, 2, True, (1, 20, 24, 40), "bf16", B, F, fwd=(9, 9, 8, 9)),
    layer("upconv8_32_1_grid_plain", 32, 1, 3, 2, True, (1, 20, 24, 40), "bf16", B, F, fwd=(8, 8, 8, 8), opts={OPT_THIN_LEAN: 0}),
    # pointwise_head_kernel: 256 voxels per workgroup, the bare 1x1x1 head; any fused form is the lanes-along-K kernel's
    layer("head_32_3", 32, 3, 1, 1, False, (1, 3, 5, 70), "fp32", F, F, fwd=(10, 2, 2, 2), dgrad=(16, 16), leaky=2, wgrad=3),
    layer("head_64_2_bf", 64, 2, 1, 1, False, (2, 4, 4, 8), "bf16", B, F, fwd=(10, 2, 2, 2), wgrad=9),
    layer("head_32_1", 32, 1, 1, 1, False, (2, 4, 4, 8), "fp32", F, F, fwd=(10, 2, 2, 2)),
    # ---- route 13: one 4 x 4 x 8 output tile.  direct_chan_kernel (fp32 precision; one input channel of bf16 precision)
    layer("chan_4_32_s2", 4, 32, 3, 2, False, (2, 9, 9, 17), "fp32", F, F, fwd=(11, 11, 11, 11), dgrad=(2, 2), leaky=11, wgrad=3),
    layer("chan_3_32_s1", 3, 32, 3, 1, False, (2, 5, 5, 9), "fp32", F, F, fwd=(11, 11, 11, 11), wgrad=3),
    layer("chan_2_32_s1", 2, 32, 3, 1, False, (2, 5, 5, 9), "fp32", F, F, fwd=(11, 11, 11, 11)),
    # a one-channel slice of a 4-channel tensor that starts inside a 16-byte group (CArgs::koff = 1)
    layer("chan_slice_1_32_s2", 1, 32, 3, 2, False, (2, 9, 9, 17), "fp32", S, F, fwd=(11, 11, 11, 11)),
    layer("chan_slice_1_32_bf16", 1, 32, 3, 1, False, (2, 5, 5, 9), "bf16", S, F, fwd=(11, 11, 11, 11)),
    # chan_mfma_kernel (bf16 precision) and its lean form: stride 2, bf16-stored x and y, 16-byte rows, no accumulate
    layer("chanm_2_32_s1", 2, 32, 3, 1, False, (2, 5, 5, 9), "bf16", F, F, fwd=(12, 12, 12, 12), leaky=12, wgrad=10),
    layer("chanm_3_32_s2_bf", 3, 32, 3, 2, False, (2, 9, 9, 17), "bf16", B, B, fwd=(13, 13, 13, 12), leaky=12, wgrad=10),
    layer("chanm_4_64_s2_bf", 4, 64, 3, 2, False, (2, 9, 9, 17), "bf16", B, B, fwd=(13, 13, 13, 12), wgrad=10),
    layer("chanm_1_64_s1_bf", 1, 64, 3, 1, False, (2, 5, 5, 9), "bf16", B, B, fwd=(12, 12, 12, 12)),
    layer("chanm_4_32_s2_plain", 4, 32, 3, 2, False, (2, 9, 9, 17), "bf16", B, B, fwd=(12, 12, 12, 12), opts={OPT_THIN_LEAN: 0}),
    layer("chanm_4_32_s2_f32out", 4, 32, 3, 2, False, (2, 9, 9, 17), "bf16", B, F, fwd=(12, 12, 12, 12), wgrad=10),
    # the 64-column form: the input gradient of a 64 -> 3 transposed convolution (gy bf16-stored with 8-byte voxels)
    layer("upconv8_64_3_thin_grads", 64, 3, 3, 2, True, (2, 5, 5, 9), "bf16", B, B, fwd=(ERR_UNSUPPORTED,) * 4, dgrad=(13, 12)),
    # ---- routes 16 and 17
    layer("pw_small_3_32", 3, 32, 1, 1, False, (1, 5, 7, 9), "fp32", F, F, fwd=(16, None, None, 16)),
    layer("pw_small_1_32", 1, 32, 1, 1, False, (2, 4, 4, 8), "fp32", F, F, fwd=(16, None, None, 16)),
    layer("pw_small_4_32_bfout", 4, 32, 1, 1, False, (1, 5, 7, 9), "fp32", F, B, fwd=(16, None, None, 16)),
    layer("pw_small_2_64", 2, 64, 1, 1, False, (1, 5, 7, 9), "fp32", F, F, fwd=(16, None, None, 16)),
    layer("pw_mfma_32_32", 32, 32, 1, 1, False, (1, 16, 16, 17), "bf16", B, B, fwd=(17, None, None, 17), dgrad=(17, 17), wgrad=9),
    layer("pw_mfma_64_32", 64, 32, 1, 1, False, (2, 16, 16, 17), "bf16", B, B, fwd=(17, None, None, 17)),
    # ---- weight gradients only: the smallest shapes whose thin-family plans pass 32 slabs (the pre-reduce stage) under inflight1:
    # 45 tiles of 4 x 4 x 8 for wgrad_small_kernel; 288 tiles of 4 x 8 x 8, eight to a slab, for wgrad_thin_tr_kernel
    layer("wgrad_small_slabs", 4, 32, 3, 2, False, (1, 17, 33, 33), "fp32", F, F, fwd=(), wgrad=3),
    layer("wgrad_thin_tr_slabs", 4, 2, 3, 1, False, (1, 12, 64, 90), "bf16", F, F, fwd=(), wgrad=10, opts={OPT_THIN_MFMA: 1}),
    # ---- weight gradients only: the instantiations of the launch tables no layer above reaches.
    # wgrad_thin_tr_kernel with a bf16-stored thin tensor (QBF): stride 1 next to an fp32-stored P of one and of two column
    # blocks, stride 1 next to a bf16-stored P of two, stride 2 next to an fp32-stored P of two
    layer("wgrad_thin_tr_qbf_2_32_s1", 2, 32, 3, 1, False, (2, 6, 10, 12), "bf16", B, F, fwd=(), wgrad=10),
    layer("wgrad_thin_tr_qbf_3_64_s1", 3, 64, 3, 1, False, (2, 6, 10, 12), "bf16", B, F, fwd=(), wgrad=10),
    layer("wgrad_thin_tr_qbf_4_64_s1_bf", 4, 64, 3, 1, False, (2, 6, 10, 12), "bf16", B, B, fwd=(), wgrad=10),
    layer("wgrad_thin_tr_qbf_3_64_s2", 3, 64, 3, 2, False, (2, 7, 11, 13), "bf16", B, F, fwd=(), wgrad=10),
] + [
    # wgrad_tiny_kernel<CS, CB, HAS_T>: the (cin, cout) pairs not above; a layer runs without and with a norm-on-load of x
    layer(f"wgrad_tiny_{ci}_{co}", ci, co, 3, 1, False, (2, 5, 7, 12), "fp32", F, F, fwd=(), wgrad=6)
    for ci, co in ((1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (3, 4), (4, 1), (4, 3), (4, 4))
]
LAYERS_BY_NAME = {l.case.name: l for l in LAYERS}
assert len(LAYERS_BY_NAME) == len(LAYERS)


def operand_type(l):
    """bf16-representable operands wherever the precision mode or a storage type is bf16."""
    return "bf16" if "bf16" in (l.dtype, l.lo, l.hi) else "fp32"


def rounds_operands(kernel):
    """The kernels that round the transformed operand of a norm-on-load to bf16 (matrix-core operands); the others compute
    on the fp32 value."""
    return kernel in (4, 5, 7, 8, 9, 12, 13, 17)


# ----------------------------------------------------------------------------- the calls of a layer
Call = namedtuple("Call", "layer orientation form want x_nl add accumulate stats")


def calls(l):
    out = []
    for form, want in zip(FWD_FORMS, l.fwd):
        fused = form.startswith("norm-on-load")
        out.append(Call(l, "fwd", form, want, "relu" if fused else None, fused, form == "accumulate", "statistics" in form))
    if l.leaky is not None:
        out.append(Call(l, "fwd", LEAKY_FORM, l.leaky, "leaky", True, False, True))
    for form, want in zip(DGRAD_FORMS, l.dgrad or ()):
        out.append(Call(l, "dgrad", form, want, None, False, form.endswith("accumulate"), False))
    return out


def conv_desc(l, orientation):
    from multimodal_tta_amd import _lib
    c = l.case
    fo, do = (_lib.CONVT_FWD, _lib.CONVT_DGRAD) if c.transposed else (_lib.CONV_FWD, _lib.CONV_DGRAD)
    return _lib.ConvDesc(fo if orientation == "fwd" else do, c.k, c.stride, c.cin, c.cout, _lib.BF16 if l.dtype == "bf16" else _lib.F32)


def made_up_tensors(l, orientation):
    """(x, y, add) descriptors of a call: what it reads, what it produces and a fused add of y's layout."""
    c = l.case
    n = c.shape[0]
    lo = lambda slot: fake(l.lo, slot, n, c.cin, c.shape[1:])
    hi = lambda slot: fake(l.hi, slot, n, c.cout, cg.out_dhw(c))
    return (lo(0), hi(1), hi(2)) if orientation == "fwd" else (hi(0), lo(1), lo(2))


_HOST_COEFFS = torch.zeros(4)      # stands for the coefficient arrays of a norm-on-load in the host-only queries


def made_up_nl(kind):
    from multimodal_tta_amd import _lib
    z = _HOST_COEFFS
    if kind == "leaky":
        return _lib.norm_on_load(z, z, scale=z, shift=z, act=_lib.ACT_LEAKY_RELU, negative_slope=LEAKY_SLOPE)
    return _lib.norm_on_load(z, z, relu=True, scale=z, shift=z)


def what_runs(desc, x, y, x_nl=None, add=None, add_nl=None, accumulate=0, stats=None):
    """The kernel of a call in the terms of `Layer`: from mmtta_conv_route and mmtta_conv_thin_kernel."""
    kw = dict(x_nl=x_nl, add=add, add_nl=add_nl, accumulate=accumulate, stats=stats)
    route, kernel = query("mmtta_conv_route", desc, x, y, **kw), query("mmtta_conv_thin_kernel", desc, x, y, **kw)
    if route < 0:
        assert kernel == route, f"mmtta_conv_thin_kernel {kernel} after mmtta_conv_route {route}"
        return route
    if route in (ROUTE_DIRECT, ROUTE_THIN):
        assert kernel < 0 or (1 <= kernel <= 10 if route == ROUTE_DIRECT else 11 <= kernel <= 13), f"route {route}: kernel id {kernel}"
        return kernel
    assert kernel == 0, f"route {route}: mmtta_conv_thin_kernel says {kernel}"
    return route if route in (ROUTE_PW_SMALL, ROUTE_PW_MFMA) else None


def ask_call(call):
    """What the call runs for made-up descriptors under the layer's options: host-only."""
    l = call.layer
    x, y, add = made_up_tensors(l, call.orientation)
    with pinned(l.opts):
        return what_runs(conv_desc(l, call.orientation), x, y, made_up_nl(call.x_nl) if call.x_nl else None,
                         add if call.add else None, made_up_nl("relu") if call.add else None, 1 if call.accumulate else 0,
                         _HOST_COEFFS.data_ptr() if call.stats else None)


# ----------------------------------------------------------------------------- weight gradients
WGRAD_GEOMETRIES = ("unsplit", "deep", "inflight1")


def wgrad_layers():
    return [l for l in LAYERS if l.wgrad is not None]


def wgrad_variants(l):
    """[(tag, options, kernel id)]: kernel 3 also in its bf16-operand branch - a thin layer of bf16 precision with
    MMTTA_OPT_WGRAD_VECTOR_STAGING = 0."""
    out = [("", dict(l.opts), l.wgrad)]
    if l.wgrad == 10 and l.lo == F and l.case.name in ("chanm_2_32_s1", "upconv8_64_3"):
        out.append((" (option 11 = 0)", {**l.opts, OPT_WGRAD_VEC: 0}, 3))
    return out


def ask_wgrad(l, opts, geo):
    """(kernel id, plan, class) of the layer's weight gradient under a named geometry: host-only."""
    from multimodal_tta_amd import _lib
    x, dy, _ = made_up_tensors(l, "fwd")
    desc = conv_desc(l, "fwd")
    with pinned(opts), pinned(cg.geometry_values(geo)):
        kid = int(_lib.load().mmtta_conv_wgrad_kernel(C.byref(desc), C.byref(x), C.byref(dy)))
        out = (C.c_int32 * 4)()
        st = int(_lib.load().mmtta_conv_wgrad_plan_sets(C.byref(desc), C.byref(x), C.byref(dy), None, out))
    assert st == 0, f"{l.case.name}: mmtta_conv_wgrad_plan_sets status {st}"
    plan = [int(v) for v in out]
    return kid, plan, wgrad_class(l, plan)


def wgrad_class(l, plan):
    """conv_geometry.wgrad_class for the thin family, whose tiles are 4 x 4 (stride 1 on the transposed reads: 8) x 8 voxels of
    the coarse tensor: `multi-tile` rests on the smaller count."""
    nsl, pre = plan[0], plan[1]
    c = l.case
    d, h, w = c.shape[1:] if c.transposed else cg.out_dhw(c)
    tiles = c.shape[0] * ((d + 3) // 4) * ((h + 7) // 8) * ((w + 7) // 8)
    if pre > 0:
        return "prereduce"
    if nsl == 1:
        return "one-slab"
    if nsl > 1 and tiles >= 2 * nsl:
        return "multi-tile"
    return None


# ----------------------------------------------------------------------------- exact reference
def nl_transform(x, sc, sh, kind):
    """relu / LeakyReLU of fmaf(x, sc, sh) as the kernels compute it: the multiply-add rounded to fp32 once, the slope a power
    of two."""
    if kind != "leaky":
        return fmaf_relu(x, sc, sh)
    n, ch = x.shape[:2]
    v = (x.double() * sc.view(n, ch, 1, 1, 1).double() + sh.view(n, ch, 1, 1, 1).double()).float()
    return torch.where(v > 0, v, v * LEAKY_SLOPE)


NlReference = namedtuple("NlReference", "y dw")


@functools.lru_cache(maxsize=None)
def nl_reference(c, ot, rounded, kind):
    """Forward and weight gradient with x under its norm-on-load, float64: the transformed operand rounded to bf16 where the
    kernel feeds the matrix cores (`rounded`), kept in fp32 where it computes on the vector ALU.  For `rounded` ReLU operands
    of bf16 type this is conv_geometry.reference's y_nl / dw_nl."""
    import torch.nn.functional as F_
    o = operands(c, ot)
    xin = nl_transform(o.x, o.sc, o.sh, kind)
    if rounded:
        xin = q_bf16(xin)
    pad = (c.k - 1) // 2
    w = o.w.double().requires_grad_(True)
    if c.transposed:
        y = F_.conv_transpose3d(xin.double(), w, o.b.double(), stride=c.stride, padding=pad, output_padding=c.stride - 1)
    else:
        y = F_.conv3d(xin.double(), w, o.b.double(), stride=c.stride, padding=pad)
    y.backward(o.gy.double())
    return NlReference(y.detach(), w.grad)


def expected(call, kernel):
    """(float64 reference, statistics reference or None) of a call that `kernel` runs."""
    l = call.layer
    c, ot = l.case, operand_type(l)
    o, r = operands(c, ot), reference(c, ot)
    if call.orientation == "dgrad":
        dx0 = q_bf16(o.dx0) if l.lo == B else o.dx0
        return (dx0.double() + r.dx if call.accumulate else r.dx), None
    if call.x_nl:
        y = nl_reference(c, ot, rounds_operands(kernel), call.x_nl).y + r.rin
    else:
        y = o.y0.double() + r.y if call.accumulate else r.y
    return y, (y if call.stats else None)


WORST = {}      # kernel name -> (worst err / bound, what): recorded, not a limit


def note_worst(kernel_name, ratio, what):
    if ratio > WORST.get(kernel_name, (-1.0, ""))[0]:
        WORST[kernel_name] = (ratio, what)
