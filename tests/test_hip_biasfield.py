"""Bias-field adaptation on the GPU: the map ``mmtta_bias_field_apply`` and the reduced input gradient
``mmtta_bias_field_grad`` against the float64 restatement of ``biasfield_reference.py``, their bitwise properties
(pass-through, the anchor's fixed point, order 0 = the input normaliser's gain, absent channels, N items = N calls), the finish
(Adam's first step, the two clamps, the l2 term) and the plugin ``biasfield_tta`` against the oracle's adaptation loop with
the map in front of the model and a second Adam on theta.

Tolerances of the kernel comparisons (derived, not measured; every test prints the observed share of its bound).
  map, fp32 out   |y - y64| <= 2^-23 [(4 + (K + 3) A_F) E |x - a| + |y64|], A_F = sum_k |theta_k phi_k|, E = exp(F): two
                  roundings per phi_k and one per fmaf put (K + 2) 2^-24 A_F on F, an absolute error of the exponent; expf's
                  2 ulp = 2^-22, the difference, the product and the sum 2^-24 each.  Counted so, the first-order sum is
                  2^-24 [(6 + (K + 2) A_F) E |x - a| + |y64|]: the stated bound is that with a factor 2 for the second-order
                  terms and is what the test asserts.  The tables enter the reference as the SAME fp32 values, theta too.
  map, bf16 out   the fp32 result rounded once: bit-equal to the fp32 output's bf16 rounding.
  gradient        |G - G64| <= 2 (K_p + K + 8) 2^-24 A with K_p = 2 x 27 x c0 products per voxel, K the field's terms and A
                  the same sum over absolute values of W, dy and the derivative (``biasfield_reference.gradient_scale``); the
                  sums over voxels are fp64.  Random signs make |G| about A / sqrt(terms), so that bound alone would pass a
                  gradient of 0 at the larger shapes: the error is also held to 1e-5 of the item's largest component.
Shapes of the gradient cases, from the kernel's tile of 4 x 8 x 64 input voxels: (2, 2, 2) - every voxel a border voxel -,
(3, 6, 10) - smaller than the tile in every axis, odd along D - and (6, 10, 70): two tiles along every axis, a multiple of the
tile in none.  The map's vector is a pair of voxels (bf16 out): (2, 2, 2), (3, 5, 7) - 105 voxels per item, so item 1 starts on
an odd voxel - and (1, 4, 6): a single plane, t_z = 0."""
import copy
import functools

import pytest
import torch

import biasfield_reference as ref

pytestmark = pytest.mark.gpu

N, ROW = 2, 20


# ----------------------------------------------------------------------------- kernel inputs
@functools.lru_cache(maxsize=None)
def kernel_inputs(shape, C, c0, seed=0):
    """Raw volumes [N, C, D, H, W], theta [N, C, 20] = 0.2 randn (different per item; an order reads its first K), per-item
    weights of two branches and their dy, all float32 values; shared by the cases and never written."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * c0 + C)
    D, H, W = shape
    x = torch.randn(N, C, D, H, W, generator=g)
    theta = 0.2 * torch.randn(N, C, ROW, generator=g)
    out = tuple((e + 1) // 2 for e in shape)
    weights = [0.2 * torch.randn(N, c0, C, 3, 3, 3, generator=g) for _ in range(2)]
    dys = [torch.randn(N, c0, *out, generator=g) for _ in range(2)]
    return x, theta, weights, dys


def rows(a, dtype=torch.float32, ldc=4, sentinel=7.5):
    """NCDHW host tensor -> channels-last device view [N, D, H, W, C] in rows of ``ldc`` lanes whose pad lanes hold ``sentinel``
    (the view owns them, as the pool's buffers do) -> (view, base)."""
    n, c = a.shape[:2]
    base = torch.full((n, *a.shape[2:], ldc), sentinel, dtype=dtype, device="cuda")
    view = base[..., :c] if ldc != c else base
    view.copy_(a.permute(0, 2, 3, 4, 1).to(dtype))
    if ldc != c:
        view._mmtta_owns_pad = True
    return view, base


def device_tables(shape):
    """The three tables as the plugin builds them, on the device."""
    from multimodal_tta_amd import biasfield
    return tuple(torch.from_numpy(t).cuda() for t in biasfield.legendre_tables(shape))


def value_range(x_cl):
    from multimodal_tta_amd import ops
    n, c = x_cl.shape[0], x_cl.shape[-1]
    rng = torch.zeros(n, c, 2, device="cuda")
    ops.intensity_range(x_cl, torch.empty(ops.intensity_range_partials(x_cl), device="cuda"), rng)
    return rng


def tables64(shape):
    """The same fp32 table values as float64, for the references."""
    return [t.double() for t in ref.legendre_tables(shape, torch.float32)]


def nchw(base, C):
    return base[..., :C].permute(0, 4, 1, 2, 3).cpu()


# ----------------------------------------------------------------------------- the map
@pytest.mark.parametrize("anchor", ["min", "zero"])
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 7), (1, 4, 6)], ids=lambda s: "x".join(map(str, s)))
def test_map_matches_the_reference_formula(shape, C, order, anchor):
    from multimodal_tta_amd import ops
    x, theta, _, _ = kernel_inputs(shape, C, 4)
    K = len(ref.terms(order))
    x_cl, _ = rows(x)
    th, rng, tabs = theta.cuda(), value_range(x_cl), device_tables(shape)
    assert torch.equal(rng[..., 0].cpu(), ref.anchors(x, "min")), "the range's lo is the exact minimum"
    y, ybase = rows(torch.zeros_like(x))
    ops.bias_field_apply(x_cl, y, th, rng, tabs, order, anchor)
    yb, ybbase = rows(torch.zeros_like(x), dtype=torch.bfloat16)
    ops.bias_field_apply(x_cl, yb, th, rng, tabs, order, anchor)
    torch.cuda.synchronize()
    x64, t64, tb = x.double(), theta[..., :K].double(), tables64(shape)
    want = ref.apply_field(x64, t64, tb, order, anchor)
    E = torch.exp(ref.log_field(t64, tb, order))
    AF = torch.einsum("bck,kdhw->bcdhw", t64.abs(), ref.basis(tb, order, torch.float64).abs())
    a = ref.anchors(x64, anchor).reshape(N, C, 1, 1, 1)
    bound = 2.0 ** -23 * ((4 + (K + 3) * AF) * E * (x64 - a).abs() + want.abs())
    got = nchw(ybase, C).double()
    ratio = ((got - want).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"map {shape} C={C} order={order} anchor={anchor}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert not torch.equal(got, x64), "theta is not in the result"
    if shape[0] == 1 and order >= 1:          # t_z = 0: P_1 = P_3 = 0 and P_2 = -1/2 along z
        assert torch.equal(tabs[0].cpu()[:, 0], torch.tensor([1.0, 0.0, -0.5, 0.0]))
    # bf16 storage: the fp32 value rounded once; the pad lanes pass through
    assert torch.equal(ybbase.cpu(), ybase.cpu().to(torch.bfloat16))
    assert (ybase[..., C:].cpu() == 7.5).all()


@pytest.mark.parametrize("order", [0, 2])
def test_zero_theta_absent_channels_and_pad_lanes_pass_through(order):
    from multimodal_tta_amd import ops
    shape, C = (3, 5, 7), 4
    K = len(ref.terms(order))
    x, theta, _, _ = kernel_inputs(shape, C, 4)
    x_cl, xbase = rows(x)
    theta = theta.clone()
    theta[0, 2, :K] = 0          # (the coefficients past K stay non-zero: they are not the order's)
    theta[1, :, :K] = 0
    th, rng, tabs = theta.cuda(), value_range(x_cl), device_tables(shape)
    for dtype in (torch.float32, torch.bfloat16):
        for anchor in ("min", "zero"):
            y, ybase = rows(torch.zeros_like(x), dtype=dtype)
            ops.bias_field_apply(x_cl, y, th, rng, tabs, order, anchor, present=[True, False, True, True])
            torch.cuda.synchronize()
            same = xbase.to(dtype)              # the input's bits (fp32) or its single rounding (bf16)
            assert torch.equal(ybase[1], same[1]), "an item whose theta is all zero"
            assert torch.equal(ybase[0, ..., 1], same[0, ..., 1]), "an absent channel"
            assert torch.equal(ybase[0, ..., 2], same[0, ..., 2]), "a channel whose K coefficients are zero"
            assert not torch.equal(ybase[0, ..., 0], same[0, ..., 0]) and not torch.equal(ybase[0, ..., 3], same[0, ..., 3])
    assert torch.equal(x_cl.cpu(), x.permute(0, 2, 3, 4, 1)), "the raw volume was written"
    assert torch.equal(th.cpu(), theta), "theta was written"


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_order_zero_with_anchor_zero_is_the_input_normalisers_gain_bit_for_bit(shape):
    from multimodal_tta_amd import ops
    C = 4
    x, theta, _, _ = kernel_inputs(shape, C, 4)
    x_cl, _ = rows(x)
    rng, tabs = value_range(x_cl), device_tables(shape)
    th = theta.cuda()
    th_in = torch.zeros(N, C, 4, device="cuda")
    th_in[..., 0] = th[..., 0]
    for dtype in (torch.float32, torch.bfloat16):
        y, ybase = rows(torch.zeros_like(x), dtype=dtype)
        z, zbase = rows(torch.zeros_like(x), dtype=dtype)
        ops.bias_field_apply(x_cl, y, th, rng, tabs, 0, "zero")
        ops.input_norm_apply(x_cl, z, th_in, rng, gamma=False)
        torch.cuda.synchronize()
        assert torch.equal(ybase, zbase), dtype
        assert not torch.equal(ybase.float().cpu()[..., :C], x.permute(0, 2, 3, 4, 1)), "the gain is not in the result"


@pytest.mark.parametrize("order", [0, 3])
def test_anchor_min_leaves_the_channel_minimum_unchanged_bit_for_bit(order):
    from multimodal_tta_amd import ops
    shape, C = (3, 5, 7), 4
    x, theta, _, _ = kernel_inputs(shape, C, 4)
    x = x.clone()
    lo = ref.anchors(x, "min")
    x[:, :, 0, :, :3] = lo.reshape(N, C, 1, 1)          # a background corner at the channel's minimum: 15 voxels, next to the one drawn
    x_cl, _ = rows(x)
    y, ybase = rows(torch.zeros_like(x))
    ops.bias_field_apply(x_cl, y, theta.cuda(), value_range(x_cl), device_tables(shape), order, "min")
    torch.cuda.synchronize()
    got = nchw(ybase, C)
    at_min = x == lo.reshape(N, C, 1, 1, 1)
    assert at_min.sum() >= N * C * 15
    assert torch.equal(got[at_min], x[at_min]), "a voxel at the anchor moved"
    assert not torch.equal(got[~at_min], x[~at_min])


# ----------------------------------------------------------------------------- the reduced gradient
def device_branches(weights, dys, nbr, dtype):
    """[(dy, weight of item 0, set stride, k, stride)] for ``ops.bias_field_grad`` and the dy values as stored (float32): the
    first branch's dy is its own tensor, the second a channel slice of a tensor twice as wide."""
    out, stored, keep = [], [], []
    for r in range(nbr):
        c0 = dys[r].shape[1]
        wide = torch.full((N, *dys[r].shape[2:], 2 * c0 if r == 1 else c0), float("nan"), dtype=dtype, device="cuda")
        view = wide[..., :c0]
        view.copy_(dys[r].permute(0, 2, 3, 4, 1).to(dtype))
        wd = weights[r].cuda().contiguous()
        keep += [wide, wd]
        out.append((view, wd[0], wd[0].numel(), 3, 2))
        stored.append(view.float().permute(0, 4, 1, 2, 3).cpu())
    return out, stored, keep


def _next_set(w, stride, i):
    """The weights of item i as a tensor of its own (the sets of ``device_branches`` are ``stride`` elements apart)."""
    return torch.as_strided(w, w.shape, w.stride(), storage_offset=w.storage_offset() + i * stride)


def run_grad(x_cl, branches, th, rng, tabs, order, anchor="min", present=None, items=None, **step):
    """-> (grad [n, C, 20], theta after the call)."""
    from multimodal_tta_amd import ops
    th = th.clone()
    if items is not None:          # one item on its own: its volume, its tables, its weight set
        i = items
        x_cl, th, rng = x_cl[i:i + 1], th[i:i + 1].clone(), rng[i:i + 1].clone()
        branches = [(dy[i:i + 1], _next_set(w, s, i), s, k, st) for dy, w, s, k, st in branches]
    n, c = th.shape[:2]
    grad = torch.full((n, c, ROW), float("nan"), device="cuda")
    partial = torch.empty(ops.bias_field_grad_partials(x_cl, order), dtype=torch.float64, device="cuda")
    ops.bias_field_grad(x_cl, branches, th, rng, tabs, order, partial, grad, anchor=anchor, present=present, **step)
    torch.cuda.synchronize()
    return grad, th


@pytest.mark.parametrize("order", [0, 2, 3])
@pytest.mark.parametrize("nbr", [1, 2], ids=["one-branch", "two-branches"])
@pytest.mark.parametrize("c0", [4, 32])
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 6, 10), (6, 10, 70)], ids=lambda s: "x".join(map(str, s)))
def test_reduced_gradient_matches_autograd_in_float64(shape, c0, nbr, order):
    C, K = 4, len(ref.terms(order))
    x, theta, weights, dys = kernel_inputs(shape, C, c0)
    x_cl, _ = rows(x)
    th, rng, tabs = theta.cuda(), value_range(x_cl), device_tables(shape)
    tb = tables64(shape)
    keep = torch.ones(C, dtype=torch.float64)
    worst = 0.0
    for dtype in (torch.float32, torch.bfloat16):
        branches, stored, _keep = device_branches(weights, dys, nbr, dtype)
        for anchor in ("min", "zero"):
            got, after = run_grad(x_cl, branches, th, rng, tabs, order, anchor)
            args = (x.double(), theta[..., :K].double(), tb, order, anchor, [w.double() for w in weights[:nbr]],
                    [d.double() for d in stored], keep)
            want, A = ref.reduced_gradient(*args), ref.gradient_scale(*args)
            bound = 2 * (2 * 27 * c0 + K + 8) * 2.0 ** -24 * A
            err = (got[..., :K].cpu().double() - want).abs()
            ratio = (err / bound.clamp_min(1e-300))[bound > 0].max().item()
            worst = max(worst, ratio)
            print(f"grad {shape} c0={c0} branches={nbr} order={order} anchor={anchor} {dtype}: worst error / bound = {ratio:.3e}")
            assert (err <= bound).all(), (err / bound.clamp_min(1e-300)).max()
            rel = (err.flatten(1).max(1).values / want.abs().flatten(1).max(1).values).max().item()
            print(f"    error / largest component = {rel:.3e}")
            assert rel <= 1e-5
            assert (got[..., K:] == 0).all(), "the terms past the order's are written 0"
            assert torch.equal(after, th), "theta is only read with lr = 0"
    print(f"grad {shape} c0={c0} branches={nbr} order={order}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_absent_channel_is_exactly_zero_and_items_equal_calls(dtype):
    shape, C, c0, order = (6, 10, 70), 4, 32, 3
    x, theta, weights, dys = kernel_inputs(shape, C, c0)
    x_cl, _ = rows(x)
    th, rng, tabs = theta.cuda(), value_range(x_cl), device_tables(shape)
    branches, stored, _keep = device_branches(weights, dys, 2, dtype)
    present = [True, False, True, True]
    state = lambda: dict(exp_avg=torch.zeros(N, C, ROW, device="cuda"), exp_avg_sq=torch.zeros(N, C, ROW, device="cuda"),
                         step=torch.zeros(N, dtype=torch.int32, device="cuda"), lr=1e-2, bounds=(0.7, 0.2))
    th0 = th.clone()
    th0[:, 1] = 0          # an absent channel starts at 0 and keeps it
    both, after = run_grad(x_cl, branches, th0, rng, tabs, order, present=present, **state())
    assert (both[:, 1] == 0).all() and (both[:, [0, 2, 3]] != 0).all()
    assert (after[:, 1] == 0).all() and (after[:, [0, 2, 3]] != th0[:, [0, 2, 3]]).all(), "theta: absent stays 0, present moves"
    keep = torch.tensor([1.0, 0.0, 1.0, 1.0], dtype=torch.float64)
    t0 = theta.clone()
    t0[:, 1] = 0
    args = (x.double(), t0.double(), tables64(shape), order, "min", [w.double() for w in weights], [d.double() for d in stored], keep)
    want, A = ref.reduced_gradient(*args), ref.gradient_scale(*args)
    assert ((both.cpu().double() - want).abs() <= 2 * (2 * 27 * c0 + 20 + 8) * 2.0 ** -24 * A).all()
    for i in range(N):
        sep = state()
        sep["exp_avg"], sep["exp_avg_sq"], sep["step"] = sep["exp_avg"][:1], sep["exp_avg_sq"][:1], sep["step"][:1]
        alone, alone_after = run_grad(x_cl, branches, th0, rng, tabs, order, present=present, items=i, **sep)
        assert torch.equal(alone[0], both[i]), f"item {i} alone differs from item {i} of the joint call"
        assert torch.equal(alone_after[0], after[i]), f"theta of item {i} alone differs from the joint call's"
    again, again_after = run_grad(x_cl, branches, th0, rng, tabs, order, present=present, **state())
    assert torch.equal(again, both) and torch.equal(again_after, after), "two runs differ"


def test_the_finish_takes_adams_first_step_and_the_two_clamps():
    shape, C, c0, order = (3, 6, 10), 4, 4, 2
    K = len(ref.terms(order))
    x, theta, weights, dys = kernel_inputs(shape, C, c0)
    x_cl, _ = rows(x)
    th, rng, tabs = theta.cuda(), value_range(x_cl), device_tables(shape)
    branches, _, _keep = device_branches(weights, dys, 2, torch.float32)
    # the moment buffers hold nan: the step that finds step == 0 starts from zero moments whatever they hold
    state = dict(exp_avg=torch.full((N, C, ROW), float("nan"), device="cuda"), exp_avg_sq=torch.full((N, C, ROW), float("nan"), device="cuda"),
                 step=torch.zeros(N, dtype=torch.int32, device="cuda"))
    gain, field = 0.15, 0.05
    g, after = run_grad(x_cl, branches, th, rng, tabs, order, present=[True, True, False, True], lr=0.05, bounds=(gain, field), **state)
    # step 1 of Adam from zero moments: theta - lr g / (|g| + eps); then the box of the coefficient
    g64, t64 = g[..., :K].cpu().double(), theta[..., :K].double()
    box = torch.full((K,), field, dtype=torch.float64)
    box[0] = gain
    want = torch.minimum(torch.maximum(t64 - 0.05 * g64 / (g64.abs() + 1e-8), -box), box)
    want[:, 2] = t64[:, 2]                                          # an absent channel keeps its theta
    got = after[..., :K].cpu().double()
    assert (got - want).abs().max() <= 1e-6
    assert torch.equal(after[..., K:], th[..., K:]), "the coefficients past K are not the order's"
    assert state["step"].tolist() == [1, 1] and torch.isfinite(state["exp_avg"][:, [0, 1, 3], :K]).all()
    assert torch.equal(after[:, 2], th[:, 2]) and (g[:, 2] == 0).all()
    live, up = got[:, [0, 1, 3]], 1 + 2.0 ** -24          # (theta is the clamped fp64 value rounded to fp32)
    assert (live[..., 1:].abs() <= field * up).all() and (live[..., 1:].abs() >= field - 1e-7).any(), "the field clamp is not in the run"
    assert (live[..., 0].abs() <= gain * up).all() and (live[..., 0].abs() > field).any(), "the gain has the field's clamp"
    assert (live[..., 0].abs() >= gain - 1e-7).any(), "the gain clamp is not in the run"
    # a second step reads the moments the first one wrote
    g2, after2 = run_grad(x_cl, branches, after, rng, tabs, order, present=[True, True, False, True], lr=0.05, bounds=(gain, field), **state)
    assert state["step"].tolist() == [2, 2] and torch.isfinite(after2).all()


def test_l2_adds_its_term_to_the_non_constant_coefficients_only():
    shape, C, c0, order, l2 = (3, 6, 10), 4, 4, 3, 0.5
    x, theta, weights, dys = kernel_inputs(shape, C, c0)
    x_cl, _ = rows(x)
    th, rng, tabs = theta.cuda(), value_range(x_cl), device_tables(shape)
    branches, _, _keep = device_branches(weights, dys, 1, torch.float32)
    plain, _ = run_grad(x_cl, branches, th, rng, tabs, order)
    with_l2, _ = run_grad(x_cl, branches, th, rng, tabs, order, l2=l2)
    assert torch.equal(with_l2[..., 0], plain[..., 0]), "the gain is not penalised"
    diff = (with_l2[..., 1:] - plain[..., 1:]).cpu().double()
    want = 2 * l2 * theta[..., 1:].double()
    # both gradients are one fp32 rounding of (sum + term): the difference is the term to 2 half-ulps of the larger gradient
    tol = 2.0 ** -23 * torch.maximum(with_l2[..., 1:].abs(), plain[..., 1:].abs()).cpu().double()
    assert ((diff - want).abs() <= tol).all() and want.abs().min() > 0


# ----------------------------------------------------------------------------- the plugin
def field_cfg(model_cfg, steps, lr=1e-3, theta_lr=1e-2, order=2, anchor="min", l2=0.0, **method):
    from test_hip_tta import root_cfg
    cfg = root_cfg(model_cfg, steps=steps, lr=lr, **method)
    cfg["method"]["name"] = "biasfield_tta"
    cfg["method"]["biasfield"] = {"lr": theta_lr, "order": order, "anchor": anchor, "l2": l2, "bound": {"gain": 0.7, "field": 0.2}}
    return cfg


EXTRA = ("field_grad", "field_coeff")


def plugin_run(name, cfg, xs, model_cfg=None):
    """Adapt the volumes ``xs`` (one call each) with a fresh plugin -> (plugin, [logits NCDHW on the host], [records])."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair
    _, hip = build_pair(model_cfg or SMALL)
    plug = get_plugin(name)(cfg).setup(hip, "cuda")
    outs, results = [], []
    for x in xs:
        r = plug.adapt_volume(x.cuda())
        torch.cuda.synchronize()
        outs.append(plug.logits(r).cpu().clone())
        results.append({k: v.cpu().clone() for k, v in r.items() if torch.is_tensor(v) and k != "logits_cl"})
        results[-1]["field_terms"] = r.get("field_terms")
    return plug, outs, results


def records_close(res, rec):
    got = res["losses"].tolist()
    assert len(got) == len(rec["losses"])
    for t, (a, b) in enumerate(zip(got, rec["losses"])):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, f"step {t}: losses {a} vs the reference loop's {b}"


@functools.lru_cache(maxsize=None)
def reference_runs(volume_index, steps, order=2, anchor="min", l2=0.0, softmax=False, missing=(), params="all", theta_lr=1e-2,
                   nru=2, R=3):
    """The float32 and the float64 run of the reference loop on one volume, computed once and shared (never written)."""
    import oracle
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_res_units=nru, num_classes=R)
    cfg = field_cfg(mcfg, steps, theta_lr=theta_lr, order=order, anchor=anchor, l2=l2)
    if softmax:
        cfg["training"]["criterion"]["softmax"], cfg["training"]["criterion"]["sigmoid"] = True, False
    x = volume(volume_index, R=R)[0]
    torch.manual_seed(42)
    model = oracle.UNet(mcfg)
    kw = dict(softmax=softmax, missing=list(missing), params=list(params) if not isinstance(params, str) else params)
    z32, r32 = ref.adapt_reference(copy.deepcopy(model), x, cfg, steps, **kw)
    z64, r64 = ref.adapt_reference(copy.deepcopy(model).double(), x.double(), cfg, steps, **kw)
    return z32, r32, z64, r64


def close_to_float64(z_hip, res, runs, what=""):
    """``test_hip_innorm.py``'s rule - as close to the float64 loop as the fp32 loop x 3, or 2e-3 of the largest value - on the
    final logits and on step 0's ``field_grad``; the losses by ``records_close``."""
    z32, r32, z64, r64 = runs
    for name, hip, a32, a64 in (("logits", z_hip, z32, z64), ("field_grad[0]", res["field_grad"][0], r32["field_grad"][0], r64["field_grad"][0])):
        scale = a64.abs().max().item()
        e_ref = (a32.double() - a64).abs().max().item() / scale
        e_hip = (hip.double() - a64).abs().max().item() / scale
        print(f"{what} {name}: HIP vs fp64 loop {e_hip:.3e}; fp32 loop vs fp64 loop {e_ref:.3e}")
        assert e_hip <= max(2e-3, 3.0 * e_ref), f"{name}: HIP vs fp64 loop {e_hip:.3e}; fp32 loop vs fp64 loop {e_ref:.3e}"
    records_close(res, r32)


def gradient_is_resolved(runs, present=None):
    """Every component of step 0's gradient is at least 100 x its own fp32-vs-fp64 difference in the CPU reference: otherwise
    Adam's sign-like first step makes theta a coin flip."""
    _, r32, _, r64 = runs
    g32, g64 = r32["field_grad"][0].double(), r64["field_grad"][0]
    chans = [c for c in range(g64.shape[1]) if present is None or present[c]]
    margin = (g64[:, chans].abs() / (g32 - g64)[:, chans].abs().clamp_min(1e-300)).min().item()
    print(f"step 0 gradient: smallest |g| / |g32 - g64| = {margin:.1f}")
    assert margin >= 100.0, margin


VOLUME = 0


@pytest.mark.parametrize("order,anchor", [(2, "min"), (3, "zero"), (0, "min")])
def test_plugin_matches_the_reference_loop(order, anchor):
    from test_hip_tta import SMALL, volume
    K = len(ref.terms(order))
    runs = reference_runs(VOLUME, 3, order=order, anchor=anchor, l2=0.01)
    gradient_is_resolved(runs)
    x = volume(VOLUME)[0]
    cfg = field_cfg(SMALL, steps=3, order=order, anchor=anchor, l2=0.01, group=1)
    plug, outs, res = plugin_run("biasfield_tta", cfg, [x])
    assert type(plug).__name__ == "BiasFieldTTA"
    print("field_grad of the HIP run, step 0:", res[0]["field_grad"][0, 0].tolist())
    close_to_float64(outs[0], res[0], runs, f"order={order} anchor={anchor}")
    assert res[0]["field_grad"].shape == (3, 1, 4, K) and res[0]["field_coeff"].shape == (1, 4, K)
    assert res[0]["field_terms"] == ref.terms(order)
    t64 = runs[3]["theta"][-1]
    assert (res[0]["field_coeff"].double() - t64).abs().max() <= 1e-3
    assert (res[0]["field_coeff"] != 0).all(), "theta has not moved"


def test_frozen_network_stays_the_source_bit_for_bit_while_theta_moves():
    from test_hip_tta import SMALL, volume
    runs = reference_runs(VOLUME, 3, params=(), theta_lr=5e-2)
    losses = runs[1]["losses"]
    print("reference losses:", losses)
    assert losses[2] < losses[0], "the reference's loss does not fall on this input"
    x = volume(VOLUME)[0]
    cfg = field_cfg(SMALL, steps=3, theta_lr=5e-2, group=2, params=[], tune_volumes=1)
    plug, outs, res = plugin_run("biasfield_tta", cfg, [x])
    ar = plug.rt.arena
    assert ar.n_train == 0
    for g in range(ar.replicas):
        assert torch.equal(ar.params_all[g], ar.source), f"replica {g} is not the source model"
    assert (res[0]["field_coeff"] != 0).all(), "theta has not moved"
    got = res[0]["losses"].reshape(3, -1)[:, 0].tolist()
    print("HIP losses:", got)
    assert got[2] < got[0]
    records_close({"losses": torch.tensor(got)}, runs[1])


def test_lr_zero_is_entmin_bit_for_bit():
    from test_hip_tta import SMALL, volume
    xs = [volume(0)[0], volume(1)[0]]
    cfg = field_cfg(SMALL, steps=2, theta_lr=0.0, group=1)
    _, ent, ent_res = plugin_run("entmin_tta", cfg, xs)
    _, got, res = plugin_run("biasfield_tta", cfg, xs)
    for a, b, ra, rb in zip(ent, got, ent_res, res):
        assert torch.equal(a, b) and torch.equal(ra["losses"], rb["losses"])
        assert rb["field_grad"].shape == (2, 1, 4, 10) and (rb["field_grad"] == 0).all() and (rb["field_coeff"] == 0).all()


def test_plugin_group_equals_one_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair, volume
    G = 2
    keys = ("losses",) + EXTRA
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = field_cfg(SMALL, steps=3, order=3, group=group, tune_volumes=2, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("biasfield_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(),) + tuple(r[k].cpu() for k in keys)
        else:
            rs = []
            for v in vols:          # (the results are views of the plugin's buffers: read before the next volume)
                r = plug.adapt_volume(v.cuda())
                rs.append((plug.logits(r).cpu(),) + tuple(r[k].cpu().clone() for k in keys))
            runs[(group, use_graph)] = (torch.cat([r[0] for r in rs]), torch.stack([r[1] for r in rs], 1),
                                        torch.cat([r[2] for r in rs], 1), torch.cat([r[3] for r in rs]))
    assert runs[(G, True)][1].shape == (3, G) and runs[(G, True)][2].shape == (3, G, 4, 20)
    assert (runs[(G, True)][2] != 0).all(), "the field's gradient is not in the run"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"
    with pytest.raises(ValueError, match="method.group"):
        plug.adapt_volume(torch.cat(vols + vols[:1]).cuda())


MISSING_VOLUME = 3          # (the volume ``test_hip_innorm.py`` takes for this case, for the reason given there)


def test_plugin_with_a_missing_modality():
    from test_hip_tta import SMALL, volume
    present = [True, False, True, True]
    runs = reference_runs(MISSING_VOLUME, 2, missing=(1,))
    gradient_is_resolved(runs, present)
    x = volume(MISSING_VOLUME)[0]
    cfg = field_cfg(SMALL, steps=2, group=1, missing_modalities=[1])
    _, outs, res = plugin_run("biasfield_tta", cfg, [x])
    assert (res[0]["field_grad"][:, :, 1] == 0).all() and (res[0]["field_grad"][:, :, [0, 2, 3]] != 0).all()
    assert (res[0]["field_coeff"][0, 1] == 0).all() and (res[0]["field_coeff"][0, [0, 2, 3]] != 0).all()
    close_to_float64(outs[0], res[0], runs, "missing [1]")
    assert (res[0]["field_coeff"].double() - runs[3]["theta"][-1]).abs().max() <= 1e-3


def test_bf16_precision_tracks_the_fp32_loop():
    """The bound of ``test_hip_innorm.py``'s bf16 case on the losses, 1e-2 relative, at the reference's learning rate; the logits
    differ from the fp32 run's, so the bf16 path was taken."""
    from test_hip_tta import SMALL, volume
    x = volume(5)[0]
    cfg = field_cfg(SMALL, steps=3, lr=1e-5, group=1, precision="bf16")
    _, outs, res = plugin_run("biasfield_tta", cfg, [x])
    _, o32, _ = plugin_run("biasfield_tta", field_cfg(SMALL, steps=3, lr=1e-5, group=1), [x])
    import oracle
    torch.manual_seed(42)
    _, rec = ref.adapt_reference(oracle.UNet(SMALL), x, cfg, 3)
    for a, b in zip(res[0]["losses"].tolist(), rec["losses"]):
        assert abs(a - b) <= 1e-2 * abs(b), (a, b)
    err = (outs[0] - o32[0]).abs().max().item() / o32[0].abs().max().item()
    print(f"bf16: logits differ from the fp32 run by {err:.3e} of the maximum")
    assert err > 1e-6, "bf16 path not taken"
    assert (res[0]["field_coeff"] != 0).all()


def test_bf16_storage_at_the_shipped_width():
    """channels[0] = 32 in bf16 precision: x' and the first level's output gradients are stored as bf16 (8-byte input rows,
    c0 = 32).  The losses track the fp32 reference loop within 1e-2."""
    import oracle
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, channels=[32, 64, 128, 256, 512])
    x = volume(5)[0]
    cfg = field_cfg(mcfg, steps=2, lr=1e-5, group=1, precision="bf16")
    plug, outs, res = plugin_run("biasfield_tta", cfg, [x], model_cfg=mcfg)
    assert plug.rt.input_dtype() == torch.bfloat16 and plug.rt.input_branches()[0][0].dtype == torch.bfloat16
    torch.manual_seed(42)
    _, rec = ref.adapt_reference(oracle.UNet(mcfg), x, cfg, 2)
    for a, b in zip(res[0]["losses"].tolist(), rec["losses"]):
        assert abs(a - b) <= 1e-2 * abs(b), (a, b)
    assert (res[0]["field_coeff"] != 0).all() and torch.isfinite(outs[0]).all()


def test_plugin_on_the_softmax_head():
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_classes=4)
    runs = reference_runs(1, 2, softmax=True, R=4)
    cfg = field_cfg(mcfg, steps=2, group=1)
    cfg["training"]["criterion"]["softmax"], cfg["training"]["criterion"]["sigmoid"] = True, False
    plug, outs, res = plugin_run("biasfield_tta", cfg, [volume(1, R=4)[0]], model_cfg=mcfg)
    assert plug.softmax
    close_to_float64(outs[0], res[0], runs, "softmax")


def test_plugin_without_residual_units_takes_the_one_branch():
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_res_units=0)
    runs = reference_runs(VOLUME, 2, nru=0)
    cfg = field_cfg(mcfg, steps=2, group=1)
    plug, outs, res = plugin_run("biasfield_tta", cfg, [volume(VOLUME)[0]], model_cfg=mcfg)
    assert len(plug.rt.input_branches()) == 1
    close_to_float64(outs[0], res[0], runs, "num_res_units 0")


def test_a_batchnorm_model_adapts_through_the_group_fallback():
    """Norms with parameters fall back to group 1 (with the runtime's warning): the field adapts there as on any model."""
    import warnings
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, norm="BATCH")
    cfg = field_cfg(mcfg, steps=2, group=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plug, outs, res = plugin_run("biasfield_tta", cfg, [volume(VOLUME)[0]], model_cfg=mcfg)
    assert plug.rt.group == 1
    assert torch.isfinite(outs[0]).all() and (res[0]["field_coeff"] != 0).all() and (res[0]["field_grad"] != 0).all()
