"""Shared helpers of tests/test_hip_conv_geometry.py (and the knob-pinning fixtures of the other convolution test modules):
the launch-geometry axis, host-only plan queries, the case table and the exact float64 reference.  No test lives here.

Everything that decides which class of launch a case is (`classify`) rests on what the ABI reports - `ksplit`, `config` - and
on K, never on a copy of the planner's stage depths."""
import contextlib
import ctypes as C
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

GEOMETRY_KEYS = (2, 3, 4, 5, 12)      # SPLITK_BELOW, SPLITK_TARGET, WGRAD_WORKGROUPS, WGRAD_THIN_SLABS, CLASS_FUSED_MIN_WORKGROUPS
GEOMETRIES = ("inflight1", "inflight4", "inflight24", "unsplit", "deep")
IGEMM_CONFIGS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 14)
CLS_FUSED = 15
CLASSES = ("unsplit", "deep", "single")
TOL_REL, TOL_ABS = 2e-4, 1e-5          # tests/test_hip_conv.py: fp32 accumulation order
BF16_STORE = 2.0 ** -8                 # one more rounding when the result is stored as bf16, per element


# ----------------------------------------------------------------------------- the geometry axis
def current_options(keys=GEOMETRY_KEYS):
    from multimodal_tta_amd import ops
    now = {}
    for key in keys:
        now[key] = ops.set_option(key, 1)       # (mmtta_set_option returns the previous value)
        ops.set_option(key, now[key])
    return now


@contextlib.contextmanager
def pinned(values):
    """Set the options in `values` ({key: value}) for the block; the launch-geometry knobs, every other key of `values` and
    ops._TUNED_FOR are afterwards what they were, on failure too."""
    from multimodal_tta_amd import ops
    saved, tuned_for = current_options(tuple(GEOMETRY_KEYS) + tuple(k for k in values if k not in GEOMETRY_KEYS)), ops._TUNED_FOR
    try:
        for key, val in values.items():
            ops.set_option(key, int(val))
        yield
    finally:
        for key, val in saved.items():
            ops.set_option(key, val)
        ops._TUNED_FOR = tuned_for


def inflight_values(volumes):
    """What ops.tune_for_volumes_in_flight(volumes) sets, read from its return value; the process is left as it was."""
    from multimodal_tta_amd import ops
    with pinned({}):
        return {int(k): int(v) for k, v in ops.tune_for_volumes_in_flight(volumes).items()}


def geometry_values(name, target=None):
    """{key: value} of one named geometry.  `deep` takes the split-K target of the call it is made for (`deep_target`)."""
    if name.startswith("inflight"):
        return inflight_values(int(name[len("inflight"):]))
    vals = dict(inflight_values(4))            # (key 12 stays at its default outside the inflight rows)
    if name == "unsplit":
        vals.update({2: 1, 3: 1, 4: 1, 5: 1})
    elif name == "deep":
        vals.update({2: 1 << 20, 3: int(target) if target else 1, 4: 4, 5: 4})
    else:
        raise KeyError(name)
    return vals


# ----------------------------------------------------------------------------- cases
Case = namedtuple("Case", "name cin cout k stride transposed shape lean deep_fwd deep_dgrad")


def case(name, cin, cout, k, stride, transposed, shape, lean=1, deep_fwd=None, deep_dgrad=None):
    return Case(name, cin, cout, k, stride, transposed, tuple(shape), lean, deep_fwd, deep_dgrad)


# Stage depths quoted in the comments are pick_config's (fp32 / bf16 operands); the tests never read them.
CASES = [
    # Np = 32, stride 1: configs 0 / 14.  K = 96, odd extents, two batch items
    case("s1_96_32", 96, 32, 3, 1, False, (2, 5, 9, 11)),
    # the same layer on the 8x8x8 bf16 tile (config 7: MMTTA_OPT_IGEMM_LEAN = 0; fp32 operands: config 0 again)
    case("s1_96_32_wide", 96, 32, 3, 1, False, (2, 9, 8, 10), lean=0),
    # Np = 64, stride 1: configs 1 / 8 (stages of 16 / 32 channels).  K = 160: 10 / 5 stages; deep with ksplit 3 is
    # 4 + 4 + 2 / 2 + 2 + 1 stages: the last split is the short one for both operand types
    case("s1_160_64", 160, 64, 3, 1, False, (2, 5, 7, 9), deep_fwd=3),
    # the four-block tile with a partly idle last column group: 136 produced channels (configs 5 / 12, stages of 8 / 16).
    # forward K = 128: 16 / 8 stages, ksplit 3 = 6 + 6 + 4 / 3 + 3 + 2 (short last split); input gradient K = 136
    case("s1_128_136", 128, 136, 3, 1, False, (2, 4, 6, 8), deep_fwd=3, deep_dgrad=3),
    # configs 2 / 9 (32-channel stages): tiles x column groups x ceil(K / 32) >= 384.  1x1x1 keeps the reference cheap;
    # forward K = 384 (12 stages, deep = 4 splits of 3), input gradient K = 128 into 384; 34 ragged tiles, two batch items
    case("pw_384_128", 384, 128, 1, 1, False, (2, 15, 17, 17), deep_fwd=4),
    # ... and the 27-tap form, where the row loader's prefetch crosses stages: K = 128 = 4 stages, deep = 2 + 2
    case("s1_128_128_big", 128, 128, 3, 1, False, (1, 16, 24, 32)),
    # stride 2, odd extents: forward configs 3 / 10 (Np = 32), 4 / 11 (Np = 64), 5 / 12 (Np = 128); the input gradient is the
    # per-class form of the stride-1 tile
    case("s2_96_32", 96, 32, 3, 2, False, (2, 7, 9, 13)),
    case("s2_96_64", 96, 64, 3, 2, False, (2, 5, 9, 11)),
    case("s2_96_128", 96, 128, 3, 2, False, (1, 5, 6, 7)),
    # transposed: the forward is the per-class stride-1 form (K = 96), the input gradient the stride-2 form (K = cout)
    case("t_96_32", 96, 32, 3, 2, True, (2, 3, 5, 6)),
    case("t_32_96", 32, 96, 3, 2, True, (1, 4, 4, 8)),
    case("t_64_96", 64, 96, 3, 2, True, (1, 3, 4, 5)),
    # weight gradient with more than 32 slabs (the pre-reduce stage) at one volume in flight: 96 / 48 tiles
    case("s1_32_32_slabs", 32, 32, 3, 1, False, (2, 16, 16, 24)),
]
CASES_BY_NAME = {c.name: c for c in CASES}
# the class-fused kernel (route 15) at its smallest admissible shape under inflight24 (threshold 22 workgroups per item):
# 2 x 2 x 2 coarse tiles x 3 column blocks = 24
CLS_FUSED_CASE = case("t_32_96_fused", 32, 96, 3, 2, True, (1, 8, 8, 16))

DTYPES = ("fp32", "bf16")


def out_dhw(c):
    return tuple(2 * v if c.transposed else (v if c.stride == 1 else (v + 1) // 2) for v in c.shape[1:])


def weight_shape(c):
    return (c.cin, c.cout, c.k, c.k, c.k) if c.transposed else (c.cout, c.cin, c.k, c.k, c.k)


def reduction_depth(c, orientation):
    """K of the call: the channels it reduces over."""
    return c.cin if orientation == "fwd" else c.cout


# ----------------------------------------------------------------------------- host-only plan queries
def _fake_tensor(_lib, base, n, ch, dhw, bf):
    d, h, w = dhw
    sw = (ch + 3) // 4 * 4 if (not bf or ch <= 4) else (ch + 7) // 8 * 8
    return _lib.Tensor(base, n, ch, d, h, w, d * h * w * sw, 1, h * w * sw, w * sw, sw, _lib.BF16 if bf else _lib.F32, 0)


def fake(base, c, dhw, bf=True, n=2):
    """A channels-last descriptor of dense voxel rows at a made-up address: the planner never reads tensor memory."""
    from multimodal_tta_amd import _lib
    return _fake_tensor(_lib, base, n, c, dhw, bf)


def query(fn, desc, x, y, x_nl=None, add=None, add_nl=None, accumulate=0, stats=None):
    """One of the queries of a run (mmtta_conv_route, mmtta_conv_stages_raw, ...: they share a signature) for the call
    mmtta_conv_run would get; `add` is the fused add's tensor, `add_nl` its norm-on-load (default: none)."""
    from multimodal_tta_amd import _lib
    epi = None
    if add is not None:
        epi = _lib.ConvEpilogue(C.pointer(add), add_nl if add_nl is not None else _lib.norm_on_load())
    return int(getattr(_lib.load(), fn)(C.byref(desc), C.byref(x), C.byref(x_nl) if x_nl is not None else None,
                                        C.byref(epi) if epi is not None else None, C.byref(y), accumulate, stats))


def _descs(c, dtype, orientation, stored_bf16):
    from multimodal_tta_amd import _lib
    fo, do = (_lib.CONVT_FWD, _lib.CONVT_DGRAD) if c.transposed else (_lib.CONV_FWD, _lib.CONV_DGRAD)
    n = c.shape[0]
    lo = _fake_tensor(_lib, 1 << 30, n, c.cin, c.shape[1:], stored_bf16)
    hi = _fake_tensor(_lib, 1 << 40, n, c.cout, out_dhw(c), stored_bf16)
    desc = _lib.ConvDesc(fo if orientation == "fwd" else do, c.k, c.stride, c.cin, c.cout, _lib.BF16 if dtype == "bf16" else _lib.F32)
    return (desc, lo, hi) if orientation == "fwd" else (desc, hi, lo)


def ask_plan(c, dtype, orientation, stored_bf16=False):
    """(ksplit, config) of mmtta_conv_plan for the call under the options as they are now.  Reads descriptors only: no GPU."""
    from multimodal_tta_amd import _lib
    desc, x, y = _descs(c, dtype, orientation, stored_bf16)
    plan = _lib.ConvPlan()
    st = int(_lib.load().mmtta_conv_plan(C.byref(desc), C.byref(x), C.byref(y), C.byref(plan)))
    assert st == 0, f"{c.name} {dtype} {orientation}: mmtta_conv_plan status {st}"
    return int(plan.ksplit), int(plan.config)


def ask_wgrad_plan(c, dtype, x_bf16=False):
    """[slabs per set, pre-reduce chunks, CGp, CDp] of mmtta_conv_wgrad_plan_sets, host-only."""
    from multimodal_tta_amd import _lib
    desc, x, y = _descs(c, dtype, "fwd", False)
    if x_bf16:
        x = _fake_tensor(_lib, 1 << 30, c.shape[0], c.cin, c.shape[1:], True)
    out = (C.c_int32 * 4)()
    st = int(_lib.load().mmtta_conv_wgrad_plan_sets(C.byref(desc), C.byref(x), C.byref(y), None, out))
    assert st == 0, f"{c.name} {dtype}: mmtta_conv_wgrad_plan_sets status {st}"
    return [int(v) for v in out]


def max_ksplit(c, dtype, orientation, stored_bf16=False):
    """ksplit with the split forced and no bound on the target: one stage per split."""
    with pinned({2: 1 << 20, 3: 1 << 20}):
        return ask_plan(c, dtype, orientation, stored_bf16)[0]


def deep_bounds(k_depth):
    """1 < ksplit < ceil(K / 32): no stage is deeper than 32 channels, so every split then runs at least two."""
    return 1, (k_depth + 31) // 32


@functools.lru_cache(maxsize=None)
def deep_target(c, dtype, orientation, stored_bf16=False):
    """The smallest split-K target (key 3, with key 2 out of the way) at which the call gets the wanted deep split - the
    case's own ksplit if it names one, else any 1 < ksplit < ceil(K / 32); None when the shape admits none (K <= 64)."""
    lo, hi = deep_bounds(reduction_depth(c, orientation))
    want = c.deep_fwd if orientation == "fwd" else c.deep_dgrad
    if hi - lo < 2:
        return None
    with pinned({2: 1 << 20}):
        from multimodal_tta_amd import ops
        for target in range(2, 1 << 14):
            ops.set_option(3, target)
            ks = ask_plan(c, dtype, orientation, stored_bf16)[0]
            if lo < ks < hi and (want is None or ks == want):
                return target
            if ks >= hi:
                break
    assert want is None, f"{c.name} {dtype} {orientation}: no target gives ksplit {want}"
    return None


def classify(ksplit, kmax, k_depth):
    """The class of a launch from what the plan reports: `unsplit` (the whole K loop in one workgroup, K > 32: at least two
    stages), `deep` (at least two stages in every split), `single` (one stage per split), or None (anything else)."""
    lo, hi = deep_bounds(k_depth)
    if ksplit == 1:
        return "unsplit" if k_depth > 32 else None
    if lo < ksplit < hi:
        return "deep"
    if ksplit == kmax:
        return "single"
    return None


def case_options(c):
    return {} if c.lean else {10: 0}


def planned(c, dtype, geo, orientation, stored_bf16=False):
    """(values, ksplit, config, class) of the call under the named geometry; values None where `deep` is not admitted."""
    with pinned(case_options(c)):
        target = deep_target(c, dtype, orientation, stored_bf16) if geo == "deep" else None
        if geo == "deep" and target is None:
            return None, 0, -1, None
        vals = geometry_values(geo, target)
        kmax = max_ksplit(c, dtype, orientation, stored_bf16)
        with pinned(vals):
            ksplit, config = ask_plan(c, dtype, orientation, stored_bf16)
    return vals, ksplit, config, classify(ksplit, kmax, reduction_depth(c, orientation))


def assert_planned_class(c, dtype, geo, orientation, ksplit, k_depth):
    """What the forced geometries are there for."""
    lo, hi = deep_bounds(k_depth)
    if geo == "unsplit":
        assert ksplit == 1, f"{c.name} {dtype} {orientation}: unsplit geometry planned ksplit {ksplit}"
    if geo == "deep":
        assert lo < ksplit < hi, f"{c.name} {dtype} {orientation}: deep geometry planned ksplit {ksplit}, K = {k_depth}"
        want = c.deep_fwd if orientation == "fwd" else c.deep_dgrad
        assert want is None or ksplit == want, f"{c.name} {dtype} {orientation}: ksplit {ksplit}, the case wants {want}"


def wgrad_tiles_at_least(c):
    """A lower bound of the tiles a weight-gradient launch walks: its largest tile is 4 x 8 x 8 voxels of the coarse tensor."""
    d, h, w = (c.shape[1:] if c.transposed else out_dhw(c))
    return c.shape[0] * ((d + 3) // 4) * ((h + 7) // 8) * ((w + 7) // 8)


def wgrad_class(c, geo, plan):
    """`one-slab`, `multi-tile` (every slab loops over at least two tiles), `prereduce`, or None."""
    nsl, pre = plan[0], plan[1]
    if pre > 0:
        return "prereduce"
    if nsl == 1:
        return "one-slab"
    if wgrad_tiles_at_least(c) >= 2 * nsl:
        return "multi-tile"
    return None


# ----------------------------------------------------------------------------- exact reference
def q_bf16(t):
    return t.to(torch.bfloat16).float()


Operands = namedtuple("Operands", "x w b gy res y0 dx0 dw0 db0 mu sc sh rmu rsc rsh xin")


def fmaf_relu(x, sc, sh):
    """relu(fmaf(x, sc, sh)) per (n, c) as the kernels compute it: the product and the sum are exact in float64 for these
    operands up to one rounding, the result is rounded to fp32 once."""
    n, ch = x.shape[:2]
    s = sc.view(n, ch, 1, 1, 1).double()
    t = sh.view(n, ch, 1, 1, 1).double()
    return torch.relu((x.double() * s + t).float())


@functools.lru_cache(maxsize=None)
def operands(c, dtype):
    """The inputs of a case, fixed by its name.  bf16 operands: x, the weights, gy, the residual operand and the accumulate
    prefill of a bf16-stored output are bf16-representable, so bf16 x bf16 products are exact in fp32 and the kernels differ
    from float64 by their accumulation order only.  `xin` is relu(fmaf(x, sc, sh)) - rounded to bf16 for bf16 operands, as
    the loader rounds it."""
    bf = dtype == "bf16"
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) for ch in c.name) + (7 if bf else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)
    q = q_bf16 if bf else (lambda t: t)
    n, d, h, w = c.shape
    yshape = (n, c.cout) + out_dhw(c)
    x = q(rnd(n, c.cin, d, h, w) * 1.5 + 0.25)
    fan = (c.cout if c.transposed else c.cin) * c.k ** 3
    wt = q(rnd(*weight_shape(c)) * fan ** -0.5)
    b = rnd(c.cout)
    gy, res, y0 = q(rnd(*yshape)), q(rnd(*yshape) * 1.5 + 0.2), q(rnd(*yshape))
    dx0, dw0, db0 = rnd(n, c.cin, d, h, w), rnd(*weight_shape(c)), rnd(c.cout)

    def coeffs(t):
        mu = t.mean(dim=(2, 3, 4)).reshape(-1).contiguous()
        sc = (1.0 / torch.sqrt(t.var(dim=(2, 3, 4), unbiased=False) + 1e-5)).reshape(-1).contiguous()
        return mu, sc, (-(mu * sc)).contiguous()          # scale = rstd, shift = -mean * scale, as nl_coeff combines them

    mu, sc, sh = coeffs(x)
    rmu, rsc, rsh = coeffs(res)
    xin = q(fmaf_relu(x, sc, sh))
    return Operands(x, wt, b, gy, res, y0, dx0, dw0, db0, mu, sc, sh, rmu, rsc, rsh, xin)


def nl_operand_mismatch(c):
    """Share of the bf16 norm-on-load operand elements that differ when the transform is the two-rounding torch.addcmul
    instead of the fused multiply-add: the cap of elements allowed to sit one bf16 ulp off is 1 in 1000."""
    o = operands(c, "bf16")
    n, ch = o.x.shape[:2]
    two = q_bf16(torch.relu(torch.addcmul(o.sh.view(n, ch, 1, 1, 1), o.x, o.sc.view(n, ch, 1, 1, 1))))
    return (two != o.xin).double().mean().item()


Reference = namedtuple("Reference", "y dx dw db y_nl dw_nl rin")


@functools.lru_cache(maxsize=None)
def reference(c, dtype):
    """float64 on the CPU, torch F.conv3d / F.conv_transpose3d + autograd, on exactly the operand values the kernels see.
    Computed once per (case, operand type) and shared by every geometry; nobody writes into it."""
    o = operands(c, dtype)
    pad = (c.k - 1) // 2

    def conv(x, w, b):
        if c.transposed:
            return F.conv_transpose3d(x, w, b, stride=c.stride, padding=pad, output_padding=c.stride - 1)
        return F.conv3d(x, w, b, stride=c.stride, padding=pad)

    x = o.x.double().requires_grad_(True)
    w = o.w.double().requires_grad_(True)
    b = o.b.double().requires_grad_(True)
    gy = o.gy.double()
    y = conv(x, w, b)
    y.backward(gy)
    w2 = o.w.double().requires_grad_(True)
    y_nl = conv(o.xin.double(), w2, o.b.double())
    y_nl.backward(gy)
    n, ch = o.res.shape[:2]
    rin = torch.relu(o.res.double() * o.rsc.view(n, ch, 1, 1, 1).double() + o.rsh.view(n, ch, 1, 1, 1).double())
    return Reference(y.detach(), x.grad, w.grad, b.grad, y_nl.detach(), w2.grad, rin)


WORST = {}      # operand type -> (worst err / bound, what): recorded, not a limit


def exact_close(what, dtype, got, ref, stored_bf16=False):
    """|got - ref| <= 2e-4 * max|ref| + 1e-5 (fp32 accumulation order), plus 2^-8 * |ref| element by element when the result
    was rounded to bf16 by its store."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bound = torch.full_like(ref, TOL_REL * ref.abs().max().item() + TOL_ABS)
    if stored_bf16:
        bound = bound + BF16_STORE * ref.abs()
    ratio = ((got - ref).abs() / bound)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    worst = ratio.max().item()
    print(f"{what} [{dtype}{', bf16-stored' if stored_bf16 else ''}]: err/bound = {worst:.3e}")
    if worst > WORST.get(dtype, (0.0, ""))[0]:
        WORST[dtype] = (worst, what)
    assert worst <= 1.0, f"{what}: err / bound = {worst:.3e} at {int(ratio.argmax())} (max|ref| = {ref.abs().max().item():.3e})"
    return worst


def stats_close(what, stats, n, y_ref):
    """The statistics rows add up to the per-(n, c) sum and sum of squares of the fp32 result, against the float64 sums
    (bounds of tests/test_hip_conv.py)."""
    cout = y_ref.shape[1]
    st = stats.view(n, -1, 2, cout).double().sum(1).cpu()
    ref_sum = y_ref.sum(dim=(2, 3, 4))
    ref_sq = (y_ref * y_ref).sum(dim=(2, 3, 4))
    assert torch.allclose(st[:, 0], ref_sum, rtol=1e-3, atol=1e-2 * max(1.0, ref_sq.max().item()) ** 0.5), f"{what}: statistics sum"
    assert torch.allclose(st[:, 1], ref_sq, rtol=1e-3, atol=1e-3), f"{what}: statistics sum of squares"
