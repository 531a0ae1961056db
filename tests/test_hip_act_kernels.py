"""LeakyReLU (and no activation) in the norm-on-load transform, kernel by kernel, against torch:
conv(leaky_relu(norm(x))) forward and weight gradient, the epilogue's fused add, combine and the norm backward passes,
with slopes inside and outside [0, 1]; plus bitwise cross-checks through the same entry points (slope 1 == no
activation, slope 0 == ReLU).  Tolerances are those of tests/test_hip_conv.py and tests/test_hip_pointwise.py."""
import pytest
import torch
import torch.nn.functional as F

from test_hip_conv import BF16_CASES, CASES, cl, cl_bf16, close, ncdhw, ref_module

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _default_launch_geometry():
    """The launch-geometry knobs (options 2 - 5 and 12) are process wide and a plugin test that ran earlier may have tuned
    them: this module runs at the library defaults (4 volumes in flight) and leaves the knobs as it found them."""
    import conv_geometry
    with conv_geometry.pinned(conv_geometry.inflight_values(4)):
        yield

SLOPES = [0.01, 0.2, -0.3, 1.5]


def _stats(t):
    mu = t.mean(dim=(2, 3, 4))
    var = t.var(dim=(2, 3, 4), unbiased=False)
    return mu.reshape(-1).cuda().contiguous(), (1.0 / torch.sqrt(var + 1e-5)).reshape(-1).cuda().contiguous()


def _leaky_nl(mean, rstd, slope):
    from multimodal_tta_amd import ops
    return ops.NL(mean, rstd, act=ops.ACT_LEAKY_RELU, negative_slope=slope)


def _conv_case(case, slope, stored, bf=False):
    """forward with a LeakyReLU norm-on-load on the input and on the epilogue add, input gradient, weight gradient"""
    from multimodal_tta_amd import ops

    cin, cout, k, stride, transposed, shape = case
    torch.manual_seed(4321 + cin * 5 + cout)
    n, d, h, w = shape
    mod = ref_module(cin, cout, k, stride, transposed)
    x = torch.randn(n, cin, d, h, w) * 1.5 + 0.3
    if stored:
        x = x.to(torch.bfloat16).float()
    mx, rx = _stats(x)
    xin = F.leaky_relu((x - mx.cpu().view(n, cin, 1, 1, 1)) * rx.cpu().view(n, cin, 1, 1, 1), slope)
    y0 = mod(xin).detach()
    r = torch.randn(y0.shape) * 0.7
    if stored:
        r = r.to(torch.bfloat16).float()
    mr, rr = _stats(r)
    radd = F.leaky_relu((r - mr.cpu().view(n, cout, 1, 1, 1)) * rr.cpu().view(n, cout, 1, 1, 1), slope)
    y_ref = y0 + radd

    op = ops.ConvOp(cin, cout, k, stride, transposed, "cuda", dtype=ops.BF16 if (bf or stored) else ops.F32)
    op.pack(mod.weight.detach().cuda().contiguous())
    x_cl = cl_bf16(x) if stored else cl(x)
    r_cl = cl_bf16(r) if stored else cl(r)
    if stored:
        y_cl = ops.new_cl(*op.out_shape(x_cl)[:4], cout, "cuda", ldc=ops.row_pad(cout, torch.bfloat16), zero=True,
                          dtype=torch.bfloat16)
    else:
        y_cl = ops.new_cl(*op.out_shape(x_cl)[:4], cout, "cuda")
    op.forward(x_cl, _leaky_nl(mx, rx, slope), mod.bias.detach().cuda(), y_cl, add=r_cl, add_nl=_leaky_nl(mr, rr, slope))
    torch.cuda.synchronize()
    return op, x_cl, y_cl, y_ref, xin, mx, rx, mod


def _wgrad_ref(case, xin, mod, gy):
    cin, cout, k, stride, transposed, shape = case
    pad = (k - 1) // 2
    w_ = mod.weight.detach().clone().requires_grad_(True)
    b_ = mod.bias.detach().clone().requires_grad_(True)
    if transposed:
        F.conv_transpose3d(xin, w_, b_, stride=stride, padding=pad, output_padding=stride - 1).backward(gy)
    else:
        F.conv3d(xin, w_, b_, stride=stride, padding=pad).backward(gy)
    return w_.grad, b_.grad


def _bound(name, got, ref, rel):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs().max().item()
    assert err <= rel * ref.abs().max().item() + 1e-5, f"{name}: max|err|={err:.3e} (max|ref|={ref.abs().max().item():.3e})"


@pytest.mark.parametrize("slope", [0.2, -0.3])
@pytest.mark.parametrize("case", CASES)
def test_conv_forward_and_wgrad_with_leaky_norm_on_load(case, slope):
    """fp32 operands: every forward kernel (row / generic loaders, direct, thin, up-convolution) and every weight-gradient
    kernel of the case table with a LeakyReLU norm-on-load on the input and on the fused add"""
    op, x_cl, y_cl, y_ref, xin, mx, rx, mod = _conv_case(case, slope, stored=False)
    close("forward (leaky input + leaky add)", ncdhw(y_cl), y_ref)
    gy = torch.randn_like(y_ref)
    dw_ref, db_ref = _wgrad_ref(case, xin, mod, gy)
    dw = torch.empty(dw_ref.shape, device="cuda")
    db = torch.empty(db_ref.shape, device="cuda")
    op.wgrad(x_cl, _leaky_nl(mx, rx, slope), cl(gy), dw, db)
    torch.cuda.synchronize()
    close("wgrad (leaky input)", dw, dw_ref)
    close("bgrad", db, db_ref)


@pytest.mark.parametrize("case,stored", [(c, False) for c in BF16_CASES] +
                         [(c, True) for c in BF16_CASES if c[0] >= 16 and c[1] > 4])
def test_conv_bf16_with_leaky_norm_on_load(case, stored):
    """bf16 operands (fp32- or bf16-stored activations): the bound of tests/test_hip_conv.py::test_conv_bf16_operands"""
    op, x_cl, y_cl, y_ref, xin, mx, rx, mod = _conv_case(case, 1.5, stored=stored, bf=True)
    _bound("forward (bf16, leaky)", ncdhw(y_cl), y_ref, 1.5e-2)
    gy = torch.randn_like(y_ref)
    dw_ref, _ = _wgrad_ref(case, xin, mod, gy)
    dw = torch.empty(dw_ref.shape, device="cuda")
    op.wgrad(x_cl, _leaky_nl(mx, rx, 1.5), cl(gy), dw, None)
    torch.cuda.synchronize()
    _bound("wgrad (bf16, leaky)", dw, dw_ref, 1.5e-2)


def _norm_setup(kind, groups, shape, affine, seed=3):
    from multimodal_tta_amd import ops

    torch.manual_seed(seed)
    n, c, d, h, w = shape
    y = (torch.randn(shape) * 1.7 + 0.3)
    gamma = (torch.rand(c) + 0.5) if affine else None
    beta = (torch.randn(c) * 0.1) if affine else None
    y_cl = cl(y)
    rows = ops.reduce_rows_per_n(y_cl)
    part = torch.empty(n * rows * 2 * c, device="cuda")
    ops.channel_stats(y_cl, part)
    mean, rstd = torch.empty(n * c, device="cuda"), torch.empty(n * c, device="cuda")
    scratch = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.norm_stats_finalize(ops.NORM_KINDS[kind], groups, part, rows, n, c, d * h * w, 1e-5, True,
                            torch.zeros(c, device="cuda") if kind == "BATCH" else None,
                            torch.ones(c, device="cuda") if kind == "BATCH" else None, 0.1, mean, rstd, scratch)
    return y, gamma, beta, y_cl, rows, mean, rstd, scratch


def _norm_ref(kind, groups, y, gamma, beta):
    if kind == "INSTANCE":
        return F.instance_norm(y, weight=gamma, bias=beta, eps=1e-5)
    if kind == "BATCH":
        c = y.shape[1]
        return F.batch_norm(y, torch.zeros(c), torch.ones(c), gamma, beta, training=True, momentum=0.1, eps=1e-5)
    return F.group_norm(y, groups, gamma, beta, eps=1e-5)


def _norm_fwd_bwd(kind, groups, shape, affine, nl_kw, act_ref, per_item=False):
    """combine (forward) and reduce / finalize / apply (backward) of act(norm(y)) against torch autograd"""
    from multimodal_tta_amd import ops

    y, gamma, beta, y_cl, rows, mean, rstd, scratch = _norm_setup(kind, groups, shape, affine)
    n, c, d, h, w = shape
    yr = y.clone().requires_grad_(True)
    g_r = gamma.clone().requires_grad_(True) if affine else None
    b_r = beta.clone().requires_grad_(True) if affine else None
    ref = act_ref(_norm_ref(kind, groups, yr, g_r, b_r))
    gout = torch.randn_like(ref)
    ref.backward(gout)
    g_d = gamma.cuda() if affine else None
    b_d = beta.cuda() if affine else None
    if per_item and affine:
        nl = ops.NL(mean, rstd, g_d.repeat(n), b_d.repeat(n), per_item=True, **nl_kw)
    else:
        nl = ops.NL(mean, rstd, g_d, b_d, **nl_kw)
    out = torch.empty_like(y_cl)
    ops.combine(y_cl, nl, None, None, out)
    dT = cl(gout)
    bpart = torch.empty(n * rows * 2 * c, device="cuda")
    m1, m2 = torch.empty(n * c, device="cuda"), torch.empty(n * c, device="cuda")
    dg = torch.zeros(c, device="cuda") if affine else None
    db = torch.zeros(c, device="cuda") if affine else None
    ops.norm_bwd_reduce(dT, y_cl, nl, bpart)
    ops.norm_bwd_finalize(ops.NORM_KINDS[kind], groups, bpart, rows, n, c, d * h * w, g_d, True, m1, m2, dg, db, False,
                          scratch)
    dy = torch.empty_like(y_cl)
    ops.norm_bwd_apply(dT, y_cl, nl, m1, m2, dy)
    torch.cuda.synchronize()
    return out, dy, dg, db, ref, yr, g_r, b_r


NORMS = [("INSTANCE", 1, (2, 32, 6, 7, 8), False), ("INSTANCE", 1, (1, 16, 8, 8, 8), True),
         ("BATCH", 1, (2, 16, 5, 6, 7), True), ("GROUP", 4, (2, 32, 6, 6, 6), True), ("GROUP", 2, (1, 8, 5, 5, 9), True)]


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("kind,groups,shape,affine,per_item", [nm + (False,) for nm in NORMS] + [nm + (True,) for nm in NORMS if nm[3]])
def test_combine_and_norm_backward_with_leaky_relu(kind, groups, shape, affine, per_item, slope):
    from multimodal_tta_amd import ops

    out, dy, dg, db, ref, yr, g_r, b_r = _norm_fwd_bwd(
        kind, groups, shape, affine, dict(act=ops.ACT_LEAKY_RELU, negative_slope=slope),
        lambda t: F.leaky_relu(t, slope), per_item)
    from test_hip_pointwise import close as pclose
    pclose("leaky combine", ncdhw(out), ref)
    pclose("leaky norm backward dx", ncdhw(dy), yr.grad, rel=2e-4, abs_=2e-6)
    if affine:
        pclose("dgamma", dg, g_r.grad, rel=2e-4, abs_=1e-4)
        pclose("dbeta", db, b_r.grad, rel=2e-4, abs_=1e-4)


@pytest.mark.parametrize("kind,groups,shape,affine", NORMS[:3])
def test_norm_without_activation(kind, groups, shape, affine):
    from multimodal_tta_amd import ops
    from test_hip_pointwise import close as pclose

    out, dy, dg, db, ref, yr, g_r, b_r = _norm_fwd_bwd(kind, groups, shape, affine, dict(act=ops.ACT_NONE), lambda t: t)
    pclose("combine (no act)", ncdhw(out), ref)
    pclose("norm backward (no act)", ncdhw(dy), yr.grad, rel=2e-4, abs_=2e-6)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("shape,affine", [((1, 64, 5, 7, 6), False), ((1, 128, 8, 8, 8), True)])
def test_small_norm_backward_with_leaky_relu(shape, affine, slope):
    from multimodal_tta_amd import ops
    from test_hip_pointwise import close as pclose

    y, gamma, beta, y_cl, rows, mean, rstd, scratch = _norm_setup("INSTANCE", 1, shape, affine, seed=9)
    n, c, d, h, w = shape
    yr = y.clone().requires_grad_(True)
    ref = F.leaky_relu(F.instance_norm(yr, weight=gamma, bias=beta, eps=1e-5), slope)
    gout = torch.randn_like(ref)
    ref.backward(gout)
    nl = _leaky_nl(mean, rstd, slope)
    nl.gamma = gamma.cuda() if affine else None
    nl.beta = beta.cuda() if affine else None
    dT = cl(gout)
    dy = torch.empty_like(y_cl)
    assert ops.norm_bwd_small_ok(dT, y_cl, nl, dy)
    ops.norm_bwd_small(dT, y_cl, nl, d * h * w, dy)
    torch.cuda.synchronize()
    pclose("one launch (leaky) vs autograd", ncdhw(dy), yr.grad, rel=2e-4, abs_=2e-6)


def _through_entry_points(nl_a, nl_b):
    """the same inputs through combine, the norm backward triple, the one-launch backward, a convolution (input and
    epilogue add transforms) and a weight gradient, once per descriptor: every output must be equal"""
    from multimodal_tta_amd import ops

    outs = []
    for make in (nl_a, nl_b):
        torch.manual_seed(11)
        shape = (1, 32, 8, 8, 8)
        y, gamma, beta, y_cl, rows, mean, rstd, scratch = _norm_setup("INSTANCE", 1, shape, True, seed=5)
        n, c, d, h, w = shape
        nl = make(mean, rstd, gamma.cuda(), beta.cuda())
        res = []
        out = torch.empty_like(y_cl)
        ops.combine(y_cl, nl, None, None, out)
        res.append(out)
        dT = cl(torch.randn(shape))
        bpart = torch.empty(n * rows * 2 * c, device="cuda")
        m1, m2 = torch.empty(n * c, device="cuda"), torch.empty(n * c, device="cuda")
        ops.norm_bwd_reduce(dT, y_cl, nl, bpart)
        ops.norm_bwd_finalize(ops.NORM_INSTANCE, 1, bpart, rows, n, c, d * h * w, nl.gamma, True, m1, m2, None, None,
                              False, scratch)
        dy = torch.empty_like(y_cl)
        ops.norm_bwd_apply(dT, y_cl, nl, m1, m2, dy)
        dys = torch.empty_like(y_cl)
        ops.norm_bwd_small(dT, y_cl, nl, d * h * w, dys)
        res += [bpart, dy, dys]
        mod = torch.nn.Conv3d(c, 32, 3, padding=1)
        op = ops.ConvOp(c, 32, 3, 1, False, "cuda")
        op.pack(mod.weight.detach().cuda().contiguous())
        yc = ops.new_cl(n, d, h, w, 32, "cuda")
        op.forward(y_cl, nl, mod.bias.detach().cuda(), yc, add=y_cl, add_nl=nl)
        dw = torch.empty(mod.weight.shape, device="cuda")
        op.wgrad(y_cl, nl, dT, dw, None)
        res += [yc, dw]
        torch.cuda.synchronize()
        outs.append(res)
    names = ["combine", "norm bwd reduce", "norm bwd apply", "norm bwd (one launch)", "conv forward", "conv wgrad"]
    differ = [n for n, a, b in zip(names, *outs) if not torch.equal(a, b)]
    # the one-launch backward is compiled per activation like every other kernel, and hipcc contracts its sums
    # (dz * xhat into fused multiply-adds) differently in the two builds: equal to its own fp32 rounding, not bit for bit
    assert differ in ([], ["norm bwd (one launch)"]), f"outputs that differ: {differ}"
    from test_hip_pointwise import close as pclose
    pclose("one launch", outs[0][3], outs[1][3], rel=2e-5, abs_=1e-6)


def test_leaky_slope_one_equals_no_activation_bitwise():
    from multimodal_tta_amd import ops
    _through_entry_points(lambda m, r, g, b: ops.NL(m, r, g, b, act=ops.ACT_LEAKY_RELU, negative_slope=1.0),
                          lambda m, r, g, b: ops.NL(m, r, g, b, act=ops.ACT_NONE))


def test_leaky_slope_zero_equals_relu_bitwise():
    from multimodal_tta_amd import ops
    _through_entry_points(lambda m, r, g, b: ops.NL(m, r, g, b, act=ops.ACT_LEAKY_RELU, negative_slope=0.0),
                          lambda m, r, g, b: ops.NL(m, r, g, b, relu=True))
