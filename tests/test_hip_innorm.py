"""Input-normaliser adaptation on the GPU: the map ``mmtta_input_norm_apply`` and the reduced input gradient
``mmtta_input_norm_grad`` against the float64 restatement of ``innorm_reference.py``, their bitwise properties (pass-through,
absent channels, N items = N calls) and the plugin ``innorm_tta`` against the oracle's adaptation loop with the map in front
of the model and a second Adam on theta.

Tolerances of the kernel comparisons (derived, not measured; every test prints the observed share of its bound).
  map, fp32 out   |y - y64| <= 2^-23 [4 |y64| + 4 exp(s) |lo| + (8 + 4 gamma + 2 gamma |log2 t|) exp(s) (hi - lo) t^gamma]: one
                  rounding each for exp(s), the product and the sum; with the power t's two roundings enter gamma-fold, the
                  hardware log2 and exp2 are 1 ulp each and the error of gamma log2 t is an absolute error of the exponent.
  map, bf16 out   the fp32 result rounded once: bit-equal to the fp32 output's bf16 rounding.
  gradient        |G - G64| <= 2 (K + 8) 2^-24 A with K = 2 x 27 x c0 products per voxel and A the same sum over absolute
                  values of W, dy and the derivative (``innorm_reference.gradient_scale``); the sums over voxels are fp64.
                  Random signs make |G| about A / sqrt(terms), so that bound alone would pass a gradient of 0 at the larger
                  shapes: the error is also held to 1e-5 of the item's largest component (the random-walk estimate is 1e-7).
Shapes of the gradient cases, from the kernel's tile of 4 x 8 x 64 input voxels: (2, 2, 2) - every voxel a border voxel -,
(3, 6, 10) - smaller than the tile in every axis, odd along D - and (6, 10, 70): two tiles along every axis, a multiple of the
tile in none.  The map's vector is a pair of voxels (bf16 out): (2, 2, 2) and (3, 5, 7), 105 voxels per item, so item 1
starts on an odd voxel."""
import copy
import functools

import pytest
import torch

from innorm_reference import adapt_reference, apply_map, channel_range, gradient_scale, reduced_gradient

pytestmark = pytest.mark.gpu

N = 2


# ----------------------------------------------------------------------------- kernel inputs
@functools.lru_cache(maxsize=None)
def kernel_inputs(shape, C, c0, gamma, seed=0):
    """Raw volumes [N, C, D, H, W], theta [N, C, 3] (different per item), per-item weights of two branches and their dy, all
    float32 values; shared by the cases and never written."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * c0 + C)
    D, H, W = shape
    x = torch.randn(N, C, D, H, W, generator=g)
    theta = 0.4 * torch.randn(N, C, 3, generator=g)
    if not gamma:
        theta[..., 2] = 0
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


def tables(x_cl, theta):
    """theta [N, C, 4] and the range [N, C, 2] on the device, the range from ``ops.intensity_range`` as the plugin takes it."""
    from multimodal_tta_amd import ops
    n, c = theta.shape[:2]
    th = torch.zeros(n, c, 4, device="cuda")
    th[..., :3] = theta.cuda()
    rng = torch.zeros(n, c, 2, device="cuda")
    ops.intensity_range(x_cl, torch.empty(ops.intensity_range_partials(x_cl), device="cuda"), rng)
    return th, rng


# ----------------------------------------------------------------------------- the map
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 7)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("gamma", [False, True], ids=["affine", "gamma"])
def test_map_matches_the_reference_formula(shape, C, gamma):
    from multimodal_tta_amd import ops
    x, theta, _, _ = kernel_inputs(shape, C, 4, gamma)
    x_cl, _ = rows(x)
    th, rng = tables(x_cl, theta)
    lo, hi = channel_range(x)
    assert torch.equal(rng.cpu(), torch.stack([lo, hi], -1)), "the range is the exact min / max"
    y, ybase = rows(torch.zeros_like(x))
    ops.input_norm_apply(x_cl, y, th, rng, gamma=gamma)
    yb, ybbase = rows(torch.zeros_like(x), dtype=torch.bfloat16)
    ops.input_norm_apply(x_cl, yb, th, rng, gamma=gamma)
    torch.cuda.synchronize()
    x64, t64 = x.double(), theta.double()
    want = apply_map(x64, t64, lo.double(), hi.double(), gamma)
    es = torch.exp(t64[..., 0]).reshape(N, C, 1, 1, 1)
    w = (hi - lo).double().reshape(N, C, 1, 1, 1)
    bound = 4 * want.abs() + 4 * es * lo.double().abs().reshape(N, C, 1, 1, 1)
    if gamma:
        gam = torch.exp(t64[..., 2]).reshape(N, C, 1, 1, 1)
        t = (x64 - lo.double().reshape(N, C, 1, 1, 1)) / w
        l2 = torch.log2(t.clamp_min(1e-300))
        bound = bound + (8 + 4 * gam + 2 * gam * l2.abs()) * es * w * torch.where(t > 0, t ** gam, torch.zeros_like(t))
    bound = bound * 2.0 ** -23
    got = y.permute(0, 4, 1, 2, 3).cpu().double()
    ratio = ((got - want).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"map {shape} C={C} gamma={gamma}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert not torch.equal(got, x64), "theta is not in the result"
    # bf16 storage: the fp32 value rounded once; the pad lanes pass through
    assert torch.equal(ybbase.cpu(), ybase.cpu().to(torch.bfloat16))
    assert (ybase[..., C:].cpu() == 7.5).all()


@pytest.mark.parametrize("gamma", [False, True], ids=["affine", "gamma"])
def test_zero_theta_and_absent_channels_pass_through(gamma):
    from multimodal_tta_amd import ops
    shape, C = (3, 5, 7), 4
    x, theta, _, _ = kernel_inputs(shape, C, 4, gamma)
    x_cl, xbase = rows(x)
    theta = theta.clone()
    theta[0, 2] = 0
    theta[1] = 0
    th, rng = tables(x_cl, theta)
    for dtype in (torch.float32, torch.bfloat16):
        y, ybase = rows(torch.zeros_like(x), dtype=dtype)
        ops.input_norm_apply(x_cl, y, th, rng, present=[True, False, True, True], gamma=gamma)
        torch.cuda.synchronize()
        same = xbase.to(dtype)              # the input's bits (fp32) or its single rounding (bf16)
        assert torch.equal(ybase[1], same[1]), "an item whose theta is all zero"
        assert torch.equal(ybase[0, ..., 1], same[0, ..., 1]), "an absent channel"
        assert torch.equal(ybase[0, ..., 2], same[0, ..., 2]), "a channel whose theta row is zero"
        assert not torch.equal(ybase[0, ..., 0], same[0, ..., 0]) and not torch.equal(ybase[0, ..., 3], same[0, ..., 3])
    assert torch.equal(x_cl.cpu(), x.permute(0, 2, 3, 4, 1)), "the raw volume was written"


# ----------------------------------------------------------------------------- the reduced gradient
def device_branches(weights, dys, nbr, dtype):
    """[(dy, weight of item 0, set stride, k, stride)] for ``ops.input_norm_grad`` and the dy values as stored (float32): the
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


def run_grad(x_cl, branches, th, rng, present=None, gamma=False, items=None, **step):
    from multimodal_tta_amd import ops
    if items is not None:          # one item on its own: its volume, its tables, its weight set
        i = items
        x_cl, th, rng = x_cl[i:i + 1], th[i:i + 1].clone(), rng[i:i + 1].clone()
        branches = [(dy[i:i + 1], _next_set(w, s, i), s, k, st) for dy, w, s, k, st in branches]
    n, c = th.shape[:2]
    grad = torch.full((n, c, 4), float("nan"), device="cuda")
    partial = torch.empty(ops.input_norm_grad_partials(x_cl), dtype=torch.float64, device="cuda")
    ops.input_norm_grad(x_cl, branches, th, rng, partial, grad, present=present, gamma=gamma, **step)
    torch.cuda.synchronize()
    return grad


def _next_set(w, stride, i):
    """The weights of item i as a tensor of its own (the sets of ``device_branches`` are ``stride`` elements apart)."""
    return torch.as_strided(w, w.shape, w.stride(), storage_offset=w.storage_offset() + i * stride)


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 6, 10), (6, 10, 70)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c0", [4, 32, 64])
@pytest.mark.parametrize("nbr", [1, 2], ids=["one-branch", "two-branches"])
def test_reduced_gradient_matches_autograd_in_float64(shape, c0, nbr):
    C = 4
    worst = 0.0
    for gamma in (False, True):
        x, theta, weights, dys = kernel_inputs(shape, C, c0, gamma)
        x_cl, _ = rows(x)
        th, rng = tables(x_cl, theta)
        lo, hi = channel_range(x)
        for dtype in (torch.float32, torch.bfloat16):
            branches, stored, _keep = device_branches(weights, dys, nbr, dtype)
            got = run_grad(x_cl, branches, th, rng, gamma=gamma)
            keep = torch.ones(C, dtype=torch.float64)
            args = (x.double(), theta.double(), lo.double(), hi.double(), gamma, [w.double() for w in weights[:nbr]],
                    [d.double() for d in stored], keep)
            want, A = reduced_gradient(*args), gradient_scale(*args)
            bound = 2 * (2 * 27 * c0 + 8) * 2.0 ** -24 * A
            err = (got[..., :3].cpu().double() - want).abs()
            ratio = (err / bound.clamp_min(1e-300))[bound > 0].max().item()
            worst = max(worst, ratio)
            print(f"grad {shape} c0={c0} branches={nbr} gamma={gamma} {dtype}: worst error / bound = {ratio:.3e}")
            assert (err <= bound).all(), (err / bound.clamp_min(1e-300)).max()
            # the worst-case bound is far above a gradient whose terms cancel; rounding errors add as a random walk, like the
            # terms themselves: sqrt(terms) 2^-24 against sqrt(terms), so 1e-5 of the largest component leaves two decades
            rel = (err.flatten(1).max(1).values / want.abs().flatten(1).max(1).values).max().item()
            print(f"    error / largest component = {rel:.3e}")
            assert rel <= 1e-5
            assert (got[..., 3] == 0).all()
            if not gamma:
                assert (got[..., 2] == 0).all(), "the gamma column is 0 with gamma off"
            # theta is only read with lr = 0
            assert torch.equal(th[..., :3].cpu(), theta)
    print(f"grad {shape} c0={c0} branches={nbr}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_absent_channel_is_exactly_zero_and_items_equal_calls(dtype):
    shape, C, c0, gamma = (6, 10, 70), 4, 32, True
    x, theta, weights, dys = kernel_inputs(shape, C, c0, gamma)
    x_cl, _ = rows(x)
    th, rng = tables(x_cl, theta)
    branches, stored, _keep = device_branches(weights, dys, 2, dtype)
    present = [True, False, True, True]
    both = run_grad(x_cl, branches, th, rng, present=present, gamma=gamma)
    assert (both[:, 1] == 0).all() and (both[:, [0, 2, 3], :3] != 0).all()
    lo, hi = channel_range(x)
    keep = torch.tensor([1.0, 0.0, 1.0, 1.0], dtype=torch.float64)
    args = (x.double(), theta.double(), lo.double(), hi.double(), gamma, [w.double() for w in weights], [d.double() for d in stored], keep)
    want, A = reduced_gradient(*args), gradient_scale(*args)
    assert ((both[..., :3].cpu().double() - want).abs() <= 2 * (2 * 27 * c0 + 8) * 2.0 ** -24 * A).all()
    for i in range(N):
        alone = run_grad(x_cl, branches, th, rng, present=present, gamma=gamma, items=i)
        assert torch.equal(alone[0], both[i]), f"item {i} alone differs from item {i} of the joint call"
    again = run_grad(x_cl, branches, th, rng, present=present, gamma=gamma)
    assert torch.equal(again, both), "two runs differ"


def test_the_finish_takes_adams_first_step_and_clamps():
    shape, C, c0 = (3, 6, 10), 4, 4
    x, theta, weights, dys = kernel_inputs(shape, C, c0, True)
    x_cl, _ = rows(x)
    th, rng = tables(x_cl, theta)
    branches, _, _keep = device_branches(weights, dys, 2, torch.float32)
    state = dict(exp_avg=torch.full((N, C, 4), float("nan"), device="cuda"), exp_avg_sq=torch.full((N, C, 4), float("nan"), device="cuda"),
                 step=torch.zeros(N, dtype=torch.int32, device="cuda"))
    g = run_grad(x_cl, branches, th, rng, present=[True, True, False, True], gamma=True, lr=0.05, bounds=(0.3, 1.0, 0.3), **state)
    # step 1 of Adam from zero moments: theta - lr g / (|g| + eps (1 - beta2)^(1/2) ...) = theta - lr sign(g) to 1e-6; then the box
    g64, t64 = g[..., :3].cpu().double(), theta.double()
    step = 0.05 * g64 / (g64.abs() + 1e-8)
    box = torch.tensor([0.3, 1.0, 0.3], dtype=torch.float64)
    want = torch.minimum(torch.maximum(t64 - step, -box), box)
    want[:, 2] = t64[:, 2]                                          # an absent channel keeps its theta
    assert (th[..., :3].cpu().double() - want).abs().max() <= 1e-6
    assert (th[..., 3] == 0).all() and state["step"].tolist() == [1, 1]
    assert torch.equal(th[:, 2, :3].cpu(), theta[:, 2]) and (g[:, 2] == 0).all()
    live = th[:, [0, 1, 3], 0].abs().cpu()
    assert (live <= 0.3).all() and (live >= 0.3 - 1e-7).any(), "the clamp is not in the run"


# ----------------------------------------------------------------------------- the plugin
def innorm_cfg(model_cfg, steps, lr=1e-3, theta_lr=1e-2, gamma=False, **method):
    from test_hip_tta import root_cfg
    cfg = root_cfg(model_cfg, steps=steps, lr=lr, **method)
    cfg["method"]["name"] = "innorm_tta"
    cfg["method"]["innorm"] = {"lr": theta_lr, "gamma": gamma, "bound": {"log_scale": 0.7, "shift": 1.0, "log_gamma": 0.7}}
    return cfg


EXTRA = ("input_grad", "input_scale", "input_shift", "input_gamma")


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
        results.append({k: v.cpu().clone() for k, v in r.items() if k != "logits_cl"})
    return plug, outs, results


def records_close(res, rec):
    got = res["losses"].tolist()
    assert len(got) == len(rec["losses"])
    for t, (a, b) in enumerate(zip(got, rec["losses"])):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, f"step {t}: losses {a} vs the reference loop's {b}"


@functools.lru_cache(maxsize=None)
def reference_runs(volume_index, steps, gamma, softmax=False, missing=(), params="all", theta_lr=1e-2, nru=2, R=3):
    """The float32 and the float64 run of the reference loop on one volume, computed once and shared (never written)."""
    import oracle
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_res_units=nru, num_classes=R)
    cfg = innorm_cfg(mcfg, steps, theta_lr=theta_lr, gamma=gamma)
    if softmax:
        cfg["training"]["criterion"]["softmax"], cfg["training"]["criterion"]["sigmoid"] = True, False
    x = volume(volume_index, R=R)[0]
    torch.manual_seed(42)
    ref = oracle.UNet(mcfg)
    kw = dict(softmax=softmax, missing=list(missing), params=list(params) if not isinstance(params, str) else params)
    z32, r32 = adapt_reference(copy.deepcopy(ref), x, cfg, steps, **kw)
    z64, r64 = adapt_reference(copy.deepcopy(ref).double(), x.double(), cfg, steps, **kw)
    return z32, r32, z64, r64


def close_to_float64(z_hip, res, runs, what=""):
    """``logits_close_to_float64``'s rule - as close to the float64 loop as the fp32 loop x 3, or 2e-3 of the largest value - on
    the final logits and on step 0's ``input_grad``; the losses by ``records_close``."""
    z32, r32, z64, r64 = runs
    for name, hip, a32, a64 in (("logits", z_hip, z32, z64), ("input_grad[0]", res["input_grad"][0], r32["input_grad"][0], r64["input_grad"][0])):
        scale = a64.abs().max().item()
        e_ref = (a32.double() - a64).abs().max().item() / scale
        e_hip = (hip.double() - a64).abs().max().item() / scale
        print(f"{what} {name}: HIP vs fp64 loop {e_hip:.3e}; fp32 loop vs fp64 loop {e_ref:.3e}")
        assert e_hip <= max(2e-3, 3.0 * e_ref), f"{name}: HIP vs fp64 loop {e_hip:.3e}; fp32 loop vs fp64 loop {e_ref:.3e}"
    records_close(res, r32)


def gradient_is_resolved(runs, gamma, present=None):
    """Every component of step 0's gradient is at least 100 x its own fp32-vs-fp64 difference in the CPU reference: otherwise
    Adam's sign-like first step makes theta a coin flip."""
    _, r32, _, r64 = runs
    g32, g64 = r32["input_grad"][0].double(), r64["input_grad"][0]
    cols = 3 if gamma else 2
    chans = [c for c in range(g64.shape[1]) if present is None or present[c]]
    margin = (g64[:, chans, :cols].abs() / (g32 - g64)[:, chans, :cols].abs().clamp_min(1e-300)).min().item()
    print(f"step 0 gradient: smallest |g| / |g32 - g64| = {margin:.1f}")
    assert margin >= 100.0, margin


VOLUME = 0


@pytest.mark.parametrize("gamma", [False, True], ids=["affine", "gamma"])
def test_plugin_matches_the_reference_loop(gamma):
    from test_hip_tta import SMALL, volume
    runs = reference_runs(VOLUME, 3, gamma)
    gradient_is_resolved(runs, gamma)
    x = volume(VOLUME)[0]
    cfg = innorm_cfg(SMALL, steps=3, gamma=gamma, group=1)
    plug, outs, res = plugin_run("innorm_tta", cfg, [x])
    assert type(plug).__name__ == "InputNormTTA"
    print("theta of the fp64 loop after every step:", runs[3]["theta"][:, 0].tolist())
    print("input_grad of the HIP run per step:", res[0]["input_grad"][:, 0].tolist())
    print("final exp(s), b, exp(g):", res[0]["input_scale"].tolist(), res[0]["input_shift"].tolist(), res[0]["input_gamma"].tolist())
    close_to_float64(outs[0], res[0], runs, f"gamma={gamma}")
    assert res[0]["input_grad"].shape == (3, 1, 4, 3)
    t64 = runs[3]["theta"][-1]
    assert (torch.log(res[0]["input_scale"]).double() - t64[..., 0]).abs().max() <= 1e-3
    assert (res[0]["input_shift"].double() - t64[..., 1]).abs().max() <= 1e-3
    if gamma:
        assert (torch.log(res[0]["input_gamma"]).double() - t64[..., 2]).abs().max() <= 1e-3
    else:
        assert (res[0]["input_grad"][..., 2] == 0).all() and (res[0]["input_gamma"] == 1).all()


def test_frozen_network_stays_the_source_bit_for_bit_while_theta_moves():
    from test_hip_tta import SMALL, volume
    runs = reference_runs(VOLUME, 3, False, params=(), theta_lr=5e-2)
    losses = runs[1]["losses"]
    print("reference losses:", losses)
    assert losses[2] < losses[0], "the reference's loss does not fall on this input"
    x = volume(VOLUME)[0]
    cfg = innorm_cfg(SMALL, steps=3, theta_lr=5e-2, group=2, params=[], tune_volumes=1)
    plug, outs, res = plugin_run("innorm_tta", cfg, [x])
    ar = plug.rt.arena
    assert ar.n_train == 0
    for g in range(ar.replicas):
        assert torch.equal(ar.params_all[g], ar.source), f"replica {g} is not the source model"
    assert (res[0]["input_scale"] != 1).all() and (res[0]["input_shift"] != 0).all(), "theta has not moved"
    got = res[0]["losses"].reshape(3, -1)[:, 0].tolist()
    print("HIP losses:", got)
    assert got[2] < got[0]
    records_close({"losses": torch.tensor(got)}, runs[1])


def test_lr_zero_is_entmin_bit_for_bit():
    from test_hip_tta import SMALL, volume
    xs = [volume(0)[0], volume(1)[0]]
    cfg = innorm_cfg(SMALL, steps=2, theta_lr=0.0, group=1)
    _, ent, ent_res = plugin_run("entmin_tta", cfg, xs)
    _, got, res = plugin_run("innorm_tta", cfg, xs)
    for a, b, ra, rb in zip(ent, got, ent_res, res):
        assert torch.equal(a, b) and torch.equal(ra["losses"], rb["losses"])
        assert (rb["input_grad"] == 0).all() and (rb["input_scale"] == 1).all() and (rb["input_shift"] == 0).all()


def test_plugin_group_equals_one_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair, volume
    G = 2
    keys = ("losses",) + EXTRA
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = innorm_cfg(SMALL, steps=3, gamma=True, group=group, tune_volumes=2, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("innorm_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(),) + tuple(r[k].cpu() for k in keys)
        else:
            rs = []
            for v in vols:          # (the results are views of the plugin's buffers: read before the next volume)
                r = plug.adapt_volume(v.cuda())
                rs.append((plug.logits(r).cpu(),) + tuple(r[k].cpu().clone() for k in keys))
            runs[(group, use_graph)] = (torch.cat([r[0] for r in rs]), torch.stack([r[1] for r in rs], 1),
                                        torch.cat([r[2] for r in rs], 1)) + tuple(torch.cat([r[i] for r in rs]) for i in (3, 4, 5))
    assert runs[(G, True)][1].shape == (3, G) and runs[(G, True)][2].shape == (3, G, 4, 3)
    assert (runs[(G, True)][2] != 0).all(), "the input gradient is not in the run"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"
    with pytest.raises(ValueError, match="method.group"):
        plug.adapt_volume(torch.cat(vols + vols[:1]).cuda())


MISSING_VOLUME = 3


def test_plugin_with_a_missing_modality():
    """Volume 3, the one ``test_hip_nuclear.py`` and ``test_hip_crf.py`` take for this case: on volume 0 the parent's own
    two-step run (``entmin_tta``, or this plugin with lr 1e-30) already sits 1.3e-2 from the oracle's loop with channel 1
    absent - Adam's second step on weights whose gradient is rounding noise -, which says nothing about theta."""
    from test_hip_tta import SMALL, volume
    present = [True, False, True, True]
    runs = reference_runs(MISSING_VOLUME, 2, False, missing=(1,))
    gradient_is_resolved(runs, False, present)
    x = volume(MISSING_VOLUME)[0]
    cfg = innorm_cfg(SMALL, steps=2, group=1, missing_modalities=[1])
    _, outs, res = plugin_run("innorm_tta", cfg, [x])
    assert (res[0]["input_grad"][:, :, 1] == 0).all() and (res[0]["input_grad"][:, :, [0, 2, 3], :2] != 0).all()
    assert res[0]["input_scale"][0, 1] == 1 and res[0]["input_shift"][0, 1] == 0 and res[0]["input_gamma"][0, 1] == 1
    close_to_float64(outs[0], res[0], runs, "missing [1]")


def test_bf16_precision_tracks_the_fp32_loop():
    """The bound of ``test_bf16_precision_tracks_the_fp32_oracle`` on the losses, 1e-2 relative, at the reference's learning
    rate; the logits differ from the fp32 run's, so the bf16 path was taken."""
    from test_hip_tta import SMALL, volume
    x = volume(5)[0]
    cfg = innorm_cfg(SMALL, steps=3, lr=1e-5, group=1, precision="bf16")
    _, outs, res = plugin_run("innorm_tta", cfg, [x])
    _, o32, _ = plugin_run("innorm_tta", innorm_cfg(SMALL, steps=3, lr=1e-5, group=1), [x])
    import oracle
    torch.manual_seed(42)
    _, rec = adapt_reference(oracle.UNet(SMALL), x, cfg, 3)
    for a, b in zip(res[0]["losses"].tolist(), rec["losses"]):
        assert abs(a - b) <= 1e-2 * abs(b), (a, b)
    err = (outs[0] - o32[0]).abs().max().item() / o32[0].abs().max().item()
    print(f"bf16: logits differ from the fp32 run by {err:.3e} of the maximum")
    assert err > 1e-6, "bf16 path not taken"
    assert (res[0]["input_scale"] != 1).all()


def test_bf16_storage_at_the_shipped_width():
    """channels[0] = 32 in bf16 precision: x' and the first level's output gradients are stored as bf16 (8-byte input rows,
    c0 = 32).  The losses track the fp32 reference loop within 1e-2."""
    import oracle
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, channels=[32, 64, 128, 256, 512])
    x = volume(5)[0]
    cfg = innorm_cfg(mcfg, steps=2, lr=1e-5, group=1, precision="bf16")
    plug, outs, res = plugin_run("innorm_tta", cfg, [x], model_cfg=mcfg)
    assert plug.rt.input_dtype() == torch.bfloat16 and plug.rt.input_branches()[0][0].dtype == torch.bfloat16
    torch.manual_seed(42)
    _, rec = adapt_reference(oracle.UNet(mcfg), x, cfg, 2)
    for a, b in zip(res[0]["losses"].tolist(), rec["losses"]):
        assert abs(a - b) <= 1e-2 * abs(b), (a, b)
    assert (res[0]["input_scale"] != 1).all() and torch.isfinite(outs[0]).all()


def test_plugin_on_the_softmax_head():
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_classes=4)
    runs = reference_runs(1, 2, False, softmax=True, R=4)
    cfg = innorm_cfg(mcfg, steps=2, group=1)
    cfg["training"]["criterion"]["softmax"], cfg["training"]["criterion"]["sigmoid"] = True, False
    plug, outs, res = plugin_run("innorm_tta", cfg, [volume(1, R=4)[0]], model_cfg=mcfg)
    assert plug.softmax
    close_to_float64(outs[0], res[0], runs, "softmax")


def test_plugin_without_residual_units_takes_the_one_branch():
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_res_units=0)
    runs = reference_runs(VOLUME, 2, False, nru=0)
    cfg = innorm_cfg(mcfg, steps=2, group=1)
    plug, outs, res = plugin_run("innorm_tta", cfg, [volume(VOLUME)[0]], model_cfg=mcfg)
    assert len(plug.rt.input_branches()) == 1
    close_to_float64(outs[0], res[0], runs, "num_res_units 0")
