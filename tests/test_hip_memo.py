"""MEMO adaptation (``memo_tta``) on the GPU: the mirrored-view layout against ``torch.flip``, the marginal-entropy loss
and the ensemble against float64 torch restatements (autograd over flipped views, log-sum-exp form), the plugin against a
MEMO restatement on the oracle networks, and the bitwise properties (no mirror axes = Tent, grouped = one volume at a
time, graph replay = eager, the returned logits = a plain eval forward of the adapted replica)."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_hip_tta import SMALL, build_pair, root_cfg, volume

pytestmark = pytest.mark.gpu

CLAMP = 87.33654          # -ln(smallest normal fp32): as far as the ensemble's logit goes


def dims_of(mask, channels_last=False):
    """The dimensions torch.flip takes for a mirror mask (bit 0 = W, 1 = H, 2 = D) on [N,C,D,H,W] (or [N,D,H,W,C])."""
    d, h, w = (1, 2, 3) if channels_last else (2, 3, 4)
    return [dim for bit, dim in ((4, d), (2, h), (1, w)) if mask & bit]


def masks_for(V):
    from multimodal_tta_amd.memo import view_masks
    return view_masks(["d", "h", "w"][:int(math.log2(V))])


# ----------------------------------------------------------------------------- float64 restatements
def marginal_log(z, masks, softmax):
    """z [G*V,R,D,H,W], view v of volume g at item g*V+v in its own mirrored frame -> log pbar (and log qbar for the
    sigmoid head) [G,R,D,H,W] in the volumes' frame, by log-sum-exp over the views."""
    V = len(masks)
    G = z.shape[0] // V
    zs = z.reshape(G, V, *z.shape[1:])
    u = torch.stack([torch.flip(zs[:, v], dims_of(m)) if m else zs[:, v] for v, m in enumerate(masks)], 1)
    if softmax:
        return torch.logsumexp(F.log_softmax(u, dim=2), 1) - math.log(V), None
    return torch.logsumexp(F.logsigmoid(u), 1) - math.log(V), torch.logsumexp(F.logsigmoid(-u), 1) - math.log(V)


def memo_loss(z, masks, softmax):
    """Per-volume MEMO loss [G] (differentiable)."""
    lp, lq = marginal_log(z, masks, softmax)
    if softmax:
        return (-(lp.exp() * lp).sum(1)).flatten(1).mean(1)
    return (-(lp.exp() * lp + lq.exp() * lq)).flatten(1).mean(1)


def loss_reference(z, masks, softmax):
    z = z.double().detach().requires_grad_(True)
    loss = memo_loss(z, masks, softmax)
    loss.sum().backward()
    return loss.detach(), z.grad


def stage(z, generic):
    from multimodal_tta_amd import ops
    n, r, d, h, w = z.shape
    ldc = (r + 3) // 4 * 4 if not generic else (r if r % 4 else r + 1)
    return ops.to_cl(z.cuda(), ldc=ldc)


def grad_buffer(z_cl, dtype):
    from multimodal_tta_amd import ops
    n, d, h, w, r = z_cl.shape
    g = ops.new_cl(n, d, h, w, r, "cuda", ldc=z_cl.stride(3) if dtype == torch.float32 else 4, dtype=dtype)
    (g if g._base is None else g._base).fill_(float("nan"))
    return g


def run_loss(z_cl, masks, softmax, dtype=torch.float32):
    from multimodal_tta_amd import ops
    g = grad_buffer(z_cl, dtype)
    G = z_cl.shape[0] // len(masks)
    partial = torch.empty(ops.memo_partials(z_cl, len(masks)), dtype=torch.float64, device="cuda")
    loss = torch.full((G,), 123.0, device="cuda")
    ops.memo_loss_items(z_cl, g, masks, partial, loss, softmax=softmax)
    torch.cuda.synchronize()
    return loss.cpu(), ops.from_cl(g.float()).cpu()


HEADS = [(False, 1, False), (False, 3, False), (False, 4, False), (False, 3, True), (False, 4, True), (False, 1, True),
         (True, 3, False), (True, 4, False)]
SATURATED = torch.tensor([0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4])


def check_loss(z, masks, softmax, generic):
    l_ref, g_ref = loss_reference(z, masks, softmax)
    assert torch.isfinite(l_ref).all() and torch.isfinite(g_ref).all()
    z_cl = stage(z, generic)
    for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
        loss, g = run_loss(z_cl, masks, softmax, dtype)
        assert torch.isfinite(loss).all() and torch.isfinite(g).all()
        for a, b in zip(loss.tolist(), l_ref.tolist()):
            print(f"V={len(masks)} {dtype}: loss {a} vs {b}")
            assert abs(a - b) <= 1e-5 * abs(b), (a, b)
        gmax = g_ref.abs().max().item()
        if dtype == torch.float32:
            err = (g.double() - g_ref).abs().max().item()
            print(f"gradient error {err / gmax:.2e} of the maximum")
            assert err <= 2e-5 * gmax
        else:
            # the fp32 result rounded to bf16, bit-exact or 1 ulp of bf16 (2^-7 relative)
            g32 = run_loss(z_cl, masks, softmax, torch.float32)[1]
            want = g32.to(torch.bfloat16).float()
            assert ((g - want).abs() <= want.abs() * 2.0 ** -7).all()


# ----------------------------------------------------------------------------- 1. mirrored views
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("G", [1, 3])
def test_mirror_views_is_bit_exact_against_torch_flip(dtype, C, G):
    from multimodal_tta_amd import ops
    gen = torch.Generator().manual_seed(17 + C + G)
    D, H, W = 5, 6, 7
    for V in (1, 2, 4, 8):
        masks = masks_for(V)
        x = ops.new_cl(G, D, H, W, C, "cuda", ldc=4, dtype=dtype)
        base = x if x._base is None else x._base
        base.copy_(torch.randn(base.shape, generator=gen).to(dtype))          # pad lanes carry values too
        y = ops.new_cl(G * V, D, H, W, C, "cuda", ldc=4, dtype=dtype)
        ybase = y if y._base is None else y._base
        ybase.fill_(float("nan"))
        ops.mirror_views(x, y, masks)
        torch.cuda.synchronize()
        for g in range(G):
            for v, m in enumerate(masks):
                want = torch.flip(base[g], [d - 1 for d in dims_of(m, channels_last=True)]) if m else base[g]
                assert torch.equal(ybase[g * V + v].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (V, g, v)


# ----------------------------------------------------------------------------- 2. the loss against float64
@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("V", [2, 4, 8])
@pytest.mark.parametrize("G", [1, 3])
def test_memo_loss_matches_float64(softmax, R, generic, V, G):
    gen = torch.Generator().manual_seed(200 + 7 * R + V + G)
    z = torch.randn((G * V, R, 5, 6, 7), generator=gen) * 3.0          # independent logits per view
    check_loss(z, masks_for(V), softmax, generic)


# The second trip of the voxel walk: the loss kernels launch at most 2048 workgroups of 256 threads per volume and walk the
# rest in a grid-stride loop; 81^3 is the smallest cube (H == W) with more voxels (531 441) than that (524 288), so the
# thread-per-voxel kernels take a ragged second trip of 7 153 voxels and the generic Bernoulli kernel four trips at R = 3.
# (softmax, generic, dtype): the Bernoulli fast path with fp32 and bf16 gradients, the generic kernel, the categorical head.
SECOND_TRIP_SHAPE = (2, 3, 81, 81, 81)
SECOND_TRIP = [pytest.param(False, False, torch.float32, id="bernoulli-fast-fp32"),
               pytest.param(False, False, torch.bfloat16, id="bernoulli-fast-bf16"),
               pytest.param(False, True, torch.float32, id="bernoulli-generic"),
               pytest.param(True, False, torch.float32, id="categorical")]


@functools.lru_cache(maxsize=None)
def second_trip_logits(seed):
    return torch.randn(SECOND_TRIP_SHAPE, generator=torch.Generator().manual_seed(seed)) * 3.0


@functools.lru_cache(maxsize=None)
def second_trip_memo_reference(softmax):
    return loss_reference(second_trip_logits(81), masks_for(2), softmax)


def check_second_trip(loss, g, g32, l_ref, g_ref, dtype):
    """check_loss's bounds: loss 1e-5 relative, the fp32 gradient 2e-5 of its maximum, a bf16 gradient the rounded fp32 one."""
    assert torch.isfinite(loss).all() and torch.isfinite(g).all()
    for a, b in zip(loss.tolist(), l_ref.tolist()):
        print(f"{dtype}: loss {a} vs {b}")
        assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    if dtype == torch.float32:
        err = (g.double() - g_ref).abs().max().item() / g_ref.abs().max().item()
        print(f"gradient error {err:.2e} of the maximum")
        assert err <= 2e-5
    else:
        want = g32.to(torch.bfloat16).float()
        assert ((g - want).abs() <= want.abs() * 2.0 ** -7).all()


@pytest.mark.parametrize("softmax,generic,dtype", SECOND_TRIP)
def test_memo_loss_on_the_second_trip_of_the_walk(softmax, generic, dtype):
    """test_memo_loss_matches_float64 at SECOND_TRIP_SHAPE: the two items are the V = 2 views (the second mirrored along D)
    of one volume."""
    masks = masks_for(2)
    l_ref, g_ref = second_trip_memo_reference(softmax)
    z_cl = stage(second_trip_logits(81), generic)
    loss, g = run_loss(z_cl, masks, softmax, dtype)
    g32 = run_loss(z_cl, masks, softmax, torch.float32)[1] if dtype != torch.float32 else g
    check_second_trip(loss, g, g32, l_ref, g_ref, dtype)


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("V", [2, 8])
def test_memo_loss_is_finite_on_saturated_logits(softmax, R, generic, V):
    gen = torch.Generator().manual_seed(300 + R + V)
    G = 2
    z = SATURATED[torch.randint(0, len(SATURATED), (G * V, R, 5, 6, 7), generator=gen)]
    z[:, :, 0, 0, :] = 1e4 if not softmax else 0.0       # every view saturated the same way: pbar -> 1 resp. 1 - pbar -> 0
    z[:, :, 0, 1, :] = -1e4 if not softmax else 0.0
    if softmax:
        z[:, 0, 0, 0, :] = 1e4
        z[:, 1, 0, 1, :] = -1e4
    check_loss(z, masks_for(V), softmax, generic)


# ----------------------------------------------------------------------------- 3. consistency
@pytest.mark.parametrize("softmax,R,generic,dtype", [(False, 3, False, torch.float32), (False, 3, False, torch.bfloat16),
                                                     (False, 3, True, torch.float32), (True, 4, False, torch.float32)])
def test_g_volumes_equal_g_single_volume_calls(softmax, R, generic, dtype):
    gen = torch.Generator().manual_seed(5)
    G, V = 3, 4
    masks = masks_for(V)
    z = torch.randn((G * V, R, 9, 8, 7), generator=gen) * 3.0
    loss, g = run_loss(stage(z, generic), masks, softmax, dtype)
    for k in range(G):
        one = run_loss(stage(z[k * V:(k + 1) * V], generic), masks, softmax, dtype)
        assert torch.equal(one[0], loss[k:k + 1]) and torch.equal(one[1], g[k * V:(k + 1) * V])


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_one_view_is_the_entropy_objective(softmax, R, generic):
    """V = 1 against mmtta_entropy_loss_items on the same logits, every head: loss within 1e-6 relative, gradient within
    2e-6 of its maximum.  (With one view nothing is mirrored and the marginal is that view's prediction, so the entry point
    hands the call to the entropy objective's own kernels; the figures printed below say how far both sit from float64.)"""
    from multimodal_tta_amd import ops
    gen = torch.Generator().manual_seed(11 + R)
    N = 3
    z = torch.randn((N, R, 5, 6, 7), generator=gen) * 3.0
    z_cl = stage(z, generic)
    loss, g = run_loss(z_cl, [0], softmax)
    g0 = grad_buffer(z_cl, torch.float32)
    partial = torch.empty(ops.entropy_partials_items(z_cl), dtype=torch.float64, device="cuda")
    loss0 = torch.empty(N, device="cuda")
    ops.entropy_loss_items(z_cl, g0, partial, loss0, softmax=softmax)
    torch.cuda.synchronize()
    g0, loss0 = ops.from_cl(g0).cpu(), loss0.cpu()
    gmax = g0.abs().max().item()
    print(f"V=1 vs entropy_loss_items: loss {((loss - loss0).abs() / loss0.abs()).max().item():.2e}, "
          f"gradient {(g - g0).abs().max().item() / gmax:.2e} of its maximum")
    assert ((loss - loss0).abs() <= 1e-6 * loss0.abs()).all(), (loss, loss0)
    g64 = loss_reference(z, [0], softmax)[1]
    print(f"against float64: entropy_loss_items {(g0.double() - g64).abs().max().item() / gmax:.2e}, "
          f"memo_loss_items {(g.double() - g64).abs().max().item() / gmax:.2e} of the maximum")
    assert (g - g0).abs().max().item() <= 2e-6 * gmax


# ----------------------------------------------------------------------------- 4. the ensemble
def run_ensemble(z_cl, masks, softmax):
    from multimodal_tta_amd import ops
    n, d, h, w, r = z_cl.shape
    out = ops.new_cl(n // len(masks), d, h, w, r, "cuda", ldc=z_cl.stride(3))
    (out if out._base is None else out._base).fill_(float("nan"))
    ops.memo_ensemble(z_cl, out, masks, softmax=softmax)
    torch.cuda.synchronize()
    return ops.from_cl(out).cpu()


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("V", [1, 2, 4, 8])
def test_memo_ensemble_matches_float64(softmax, R, generic, V):
    gen = torch.Generator().manual_seed(400 + R + V)
    G = 2
    masks = masks_for(V)
    for saturated in (False, True):
        if saturated:
            z = SATURATED[torch.randint(0, len(SATURATED), (G * V, R, 5, 6, 7), generator=gen)]
        else:
            z = torch.randn((G * V, R, 5, 6, 7), generator=gen) * 3.0
        lp, lq = marginal_log(z.double(), masks, softmax)
        ref = lp if softmax else lp - lq
        got = run_ensemble(stage(z, generic), masks, softmax)
        assert torch.isfinite(got).all()
        if V == 1 and not softmax:
            # logit(sigmoid(z)) = z: the input, to 1 ulp
            assert ((got - z).abs() <= z.abs() * 2.0 ** -23).all()
            continue
        inside = ref.abs() < CLAMP if not softmax else torch.ones_like(ref, dtype=torch.bool)          # (log pbar is not clamped)
        scale = ref[inside].abs().max().item()
        err = (got.double() - ref)[inside].abs().max().item()
        print(f"ensemble V={V} saturated={saturated}: {err / scale:.2e} of max|result|")
        assert err <= 2e-5 * scale
        assert (got[~inside].abs() <= CLAMP * (1 + 1e-6)).all() and (got[~inside].sign() == ref[~inside].sign()).all()


# ----------------------------------------------------------------------------- the plugin against a MEMO restatement
def memo_views(x, masks):
    """x [G,C,D,H,W] -> [G*V,C,D,H,W], item g*V+v = volume g mirrored along view v's axes."""
    vs = torch.stack([torch.flip(x, dims_of(m)) if m else x for m in masks], 1)
    return vs.reshape(-1, *x.shape[1:])


def memo_reference(model, x, train_cfg, steps, masks, params="all", softmax=False, ensemble=False, missing=()):
    """MEMO over the mirror views with torch autograd, one volume: the views are one batch on the one weight set."""
    import oracle
    from oracle.tta import apply_modality_mask, modality_mask, select_params
    named = select_params(model, params)
    chosen = {id(p) for _, p in named}
    for p in model.parameters():
        p.requires_grad_(id(p) in chosen)
    opt = oracle.adam.build_optimizer(named, train_cfg)
    x = apply_modality_mask(x, modality_mask(x.shape[1], missing, 0.0, None))
    xv = memo_views(x, masks)
    losses = []
    model.train()
    for _ in range(steps):
        opt.zero_grad()
        loss = memo_loss(model(xv), masks, softmax)[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    model.eval()
    with torch.no_grad():
        if ensemble:
            lp, lq = marginal_log(model(xv), masks, softmax)
            logits = lp if softmax else lp - lq
        else:
            logits = model(x)
    for p in model.parameters():
        p.requires_grad_(True)
    return {"logits": logits, "losses": losses}


def memo_cfg(model_cfg, axes, steps=3, lr=None, ensemble=False, **method):
    """``lr=None``: the configured learning rate (the reference's)."""
    from multimodal_tta_amd.config import compose
    cfg = root_cfg(model_cfg, steps=steps, lr=1e-3 if lr is None else lr, **method)
    if lr is None:
        cfg["training"]["optimizers"]["adam"]["lr"] = compose(overrides=["task=brats", "model=unet"])["training"]["optimizers"]["adam"]["lr"]
    cfg["method"]["name"] = "memo_tta"
    cfg["method"]["memo"] = {"mirror_axes": list(axes), "ensemble": ensemble}
    return cfg


def check_against_reference(z_hip, losses, out_ref, ref0, x, y, cfg, masks, softmax=False, bf16=False, **kw):
    """Tent's bounds.  fp32, against a float64 run of the restatement: per-step loss 1e-4 relative,
    final logits within max(2e-3 of max|logits|, 3x the fp32 restatement's own distance from that run), mask voxels differing
    only where the float64 logit (softmax head: the float64 top-2 margin) lies within that bound of the threshold, Dice 1e-3.
    bf16, against the fp32 restatement: loss 1e-2, logits 3e-2 of max|logits|, masks 1e-2, Dice 2e-2, and the bf16 path must
    have been taken."""
    import oracle
    steps = len(out_ref["losses"])
    losses = losses.cpu().reshape(-1).tolist()

    def masks_of(z):
        if softmax:
            return F.one_hot(z.argmax(1), z.shape[1]).permute(0, 4, 1, 2, 3)
        return torch.sigmoid(z) >= 0.5

    def dice(m):
        return oracle.binary_dice_iou(m.to(torch.uint8), (y > 0.5).to(torch.uint8))[0]

    z_ref = out_ref["logits"]
    if bf16:
        for t, (a, b) in enumerate(zip(losses, out_ref["losses"])):
            assert abs(a - b) <= 1e-2 * abs(b), f"step {t}: loss {a} vs reference {b}"
        err = (z_hip - z_ref).abs().max().item() / z_ref.abs().max().item()
        mism = (masks_of(z_hip) != masks_of(z_ref)).float().mean().item()
        ddice = (dice(masks_of(z_hip)) - dice(masks_of(z_ref))).abs().max().item()
        print(f"bf16: losses {losses}; logits {err:.2e}, masks {mism:.2e}, Dice {ddice:.2e}")
        assert err > 1e-6, "bf16 path not taken"
        assert err <= 3e-2 and mism <= 1e-2 and ddice <= 2e-2, (err, mism, ddice)
        return
    o64 = memo_reference(copy.deepcopy(ref0).double(), x.double(), cfg["training"], steps, masks, softmax=softmax, **kw)
    for t in range(steps):
        a, b, c = losses[t], out_ref["losses"][t], o64["losses"][t]
        print(f"step {t}: loss {a}, fp32 restatement {b}, float64 {c}")
        assert abs(a - c) <= 1e-4 * abs(c) + 1e-6, f"step {t}: loss {a}, fp32 {b}, fp64 {c}"
    z64 = o64["logits"]
    scale = z64.abs().max().item()
    e_ref = (z_ref.double() - z64).abs().max().item() / scale
    e_hip = (z_hip.double() - z64).abs().max().item() / scale
    bound = max(2e-3, 3.0 * e_ref)
    print(f"losses {losses}; logits {e_hip:.2e} (fp32 restatement {e_ref:.2e})")
    assert e_hip <= bound, f"HIP vs fp64 MEMO {e_hip:.3e}; fp32 MEMO vs fp64 MEMO {e_ref:.3e}"
    m_hip, m_ref, m64 = masks_of(z_hip), masks_of(z_ref), masks_of(z64)
    if softmax:
        # the argmax may differ only where the float64 top-2 margin lies within the logit bound
        top2 = z64.topk(2, dim=1).values
        near = ((top2[:, 0] - top2[:, 1]) <= bound * scale).unsqueeze(1)
    else:
        near = z64.abs() <= bound * scale
    assert not torch.any((m_hip != m64) & ~near), "a mask voxel differs away from the threshold"
    d64 = dice(m64)
    dd_hip, dd_ref = (dice(m_hip) - d64).abs().max().item(), (dice(m_ref) - d64).abs().max().item()
    print(f"Dice {dd_hip:.2e} (fp32 restatement {dd_ref:.2e}), mask voxels differing {(m_hip != m64).float().mean().item():.2e}")
    assert dd_hip <= 1e-3, (dd_hip, dd_ref)


BATCH = dict(SMALL, norm="BATCH")
RUNNING_TOL = 5e-5


def bn_twins(plug, hip, ref):
    names = {id(m): n for n, m in hip.named_modules()}
    return [ref.get_submodule(names[id(mod)]) for mod in plug.rt.buffers]


def check_running_stats(plug, hip, ref, g, steps):
    for (rm, rv, nb), mod in zip(plug.rt.replica_buffers(g), bn_twins(plug, hip, ref)):
        assert (rm.cpu() - mod.running_mean).abs().max().item() <= RUNNING_TOL
        assert (rv.cpu() - mod.running_var).abs().max().item() <= RUNNING_TOL * max(1.0, mod.running_var.abs().max().item())
        assert nb is None or int(nb) == int(mod.num_batches_tracked) == steps


# ----------------------------------------------------------------------------- 5. one step, stage by stage
@pytest.mark.parametrize("axes", [["h", "w"], ["d"]])
def test_one_memo_step_matches_torch_stage_by_stage(monkeypatch, axes):
    """One eager step of the plugin read at every stage against torch on the same weights: the V views' logits (5e-4 of
    their maximum), the loss (1e-5 relative) and every parameter's gradient summed over the views (2e-3 of its tensor's
    maximum) - the whole-network bounds of DESIGN.md section 6."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    masks = view_masks(axes)
    cfg = memo_cfg(SMALL, axes, steps=1, lr=1e-3, group=1, use_graph=False)
    ref, hip = build_pair(SMALL)
    x, _ = volume(0)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    assert plug.views == len(masks) and not plug.rt.fused_layers
    rec = {}
    loss_items, step = ops.memo_loss_items, plug.optimizer_step

    def spy_loss(logits, dlogits, view_axes, partial, loss, softmax=False):
        loss_items(logits, dlogits, view_axes, partial, loss, softmax=softmax)
        rec["z"], rec["loss"], rec["axes"] = ops.from_cl(logits).cpu(), loss.cpu().clone(), list(view_axes)

    def spy_step(volumes=1, fused=False):
        ar = plug.rt.arena
        rec["g"], rec["volumes"] = ar.grads_all[0, :ar.n_train].cpu(), volumes
        step(volumes, fused=fused)

    monkeypatch.setattr(ops, "memo_loss_items", spy_loss)
    monkeypatch.setattr(plug, "optimizer_step", spy_step)
    plug.adapt_volume(x.cuda())
    assert rec["axes"] == masks and rec["volumes"] == 1
    ref.train()
    z = ref(memo_views(x, masks))
    loss = memo_loss(z, masks, False)[0]
    loss.backward()
    assert (rec["z"] - z.detach()).abs().max().item() <= 5e-4 * z.abs().max().item()
    assert abs(rec["loss"].item() - loss.item()) <= 1e-5 * abs(loss.item())
    ar = plug.rt.arena
    named = dict(ref.named_parameters())
    from test_hip_unet import feeds_norm
    for r in ar.refs:
        if r.trainable:
            want = named[r.name].grad.reshape(-1)
            got = rec["g"][r.offset:r.offset + r.numel]
            if feeds_norm(ref, r.name):
                # a bias in front of a norm layer has an analytically zero gradient: both sides hold the rounding residue
                # of sum(dy), bounded against the weight gradient
                wscale = named[r.name[:-len("bias")] + "weight"].grad.abs().max().item()
                assert got.abs().max().item() <= 2e-3 * wscale and want.abs().max().item() <= 2e-3 * wscale, r.name
                continue
            assert (got - want).abs().max().item() <= 2e-3 * want.abs().max().item(), r.name


# ----------------------------------------------------------------------------- 6. S steps against the restatement
@pytest.mark.parametrize("model_cfg,axes,ensemble", [(SMALL, ["h", "w"], False), (BATCH, ["w"], False),
                                                     (SMALL, ["d", "w"], True)])
def test_memo_matches_the_restatement(model_cfg, axes, ensemble):
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    masks = view_masks(axes)
    cfg = memo_cfg(model_cfg, axes, steps=3, ensemble=ensemble, group=1)
    ref, hip = build_pair(model_cfg)
    ref0 = copy.deepcopy(ref)
    x, y = volume(0)
    out_ref = memo_reference(ref, x, cfg["training"], 3, masks, ensemble=ensemble)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    res = plug.adapt_volume(x.cuda())
    assert res["losses"].shape == (3,)
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, masks, ensemble=ensemble)
    if model_cfg is BATCH:
        check_running_stats(plug, hip, ref, 0, 3)


def test_memo_batchnorm_norm_sets_group_matches_the_restatement():
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    G, axes = 3, ["h"]
    masks = view_masks(axes)
    cfg = memo_cfg(BATCH, axes, steps=3, group=G, norm_sets=True)
    ref, hip = build_pair(BATCH)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    assert plug.group == G
    vols = [volume(i) for i in range(G)]
    res = plug.adapt_volume(torch.cat([v[0] for v in vols]).cuda())
    assert res["losses"].shape == (3, G)
    z = plug.logits(res).cpu()
    for g in range(G):
        x, y = vols[g]
        m = copy.deepcopy(ref)
        out_ref = memo_reference(m, x, cfg["training"], 3, masks)
        check_against_reference(z[g:g + 1], res["losses"][:, g], out_ref, ref, x, y, cfg, masks)
        check_running_stats(plug, hip, m, g, 3)


def test_memo_softmax_head_matches_the_restatement():
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    axes = ["h", "w"]
    mcfg = dict(SMALL, num_classes=4)
    cfg = memo_cfg(mcfg, axes, steps=3, group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    ref, hip = build_pair(mcfg)
    ref0 = copy.deepcopy(ref)
    x, y = volume(1, R=4)
    out_ref = memo_reference(ref, x, cfg["training"], 3, view_masks(axes), softmax=True)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    assert plug.softmax
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, view_masks(axes), softmax=True)


def test_memo_hecktor_shaped_head_and_missing_modality():
    """One region, two modalities, a ragged-aspect volume; then the same with a missing modality (mask, then mirror)."""
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    axes = ["h", "w"]
    mcfg = dict(SMALL, in_channels=2, num_classes=1)
    for missing in ([], [1]):
        cfg = memo_cfg(mcfg, axes, steps=3, group=1, missing_modalities=missing)
        ref, hip = build_pair(mcfg, seed=7)
        ref0 = copy.deepcopy(ref)
        x, y = volume(2, shape=(16, 48, 48), C=2, R=1)
        out_ref = memo_reference(ref, x, cfg["training"], 3, view_masks(axes), missing=missing)
        plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
        res = plug.adapt_volume(x.cuda())
        check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, view_masks(axes),
                                missing=missing)


def test_memo_deepfusion_matches_the_restatement():
    import oracle
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    axes = ["w"]
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = memo_cfg(mcfg, axes, steps=3, group=2)
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(mcfg)
    hip = MultimodalUNetDeepFusion(mcfg)
    hip.load_state_dict(ref.state_dict())
    ref0 = copy.deepcopy(ref)
    x, y = volume(2)
    out_ref = memo_reference(ref, x, cfg["training"], 3, view_masks(axes))
    with pytest.warns(UserWarning, match="method.group = 2 -> 1"):
        plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    assert plug.group == 1
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, view_masks(axes))


def test_views_do_not_stick_to_the_model():
    """A deep-fusion model that memo_tta set up (views at group 1 only) takes its volume group again under entmin_tta."""
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    torch.manual_seed(42)
    hip = MultimodalUNetDeepFusion(mcfg)
    with pytest.warns(UserWarning, match="method.group = 2 -> 1"):
        plug = get_plugin("memo_tta")(memo_cfg(mcfg, ["w"], steps=1, group=2)).setup(hip, "cuda")
    assert plug.group == 1 and hip.views == 2
    cfg = memo_cfg(mcfg, [], steps=1, group=2)
    cfg["method"]["name"] = "entmin_tta"
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    assert plug.group == 2 and hip.views == 1 and plug.rt.views == 1


def test_memo_bf16_tracks_the_restatement():
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    axes = ["h", "w"]
    cfg = memo_cfg(SMALL, axes, steps=3, group=1, precision="bf16")
    ref, hip = build_pair(SMALL)
    x, y = volume(5)
    out_ref = memo_reference(ref, x, cfg["training"], 3, view_masks(axes))
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, None, x, y, cfg, view_masks(axes), bf16=True)


# ----------------------------------------------------------------------------- 7. bit for bit
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_no_mirror_axes_is_bitwise_entmin(precision):
    """``mirror_axes: []``: the plugin runs entmin_tta's own step - its loss kernel, its fused update."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_groups import WIDE
    model_cfg = SMALL if precision == "fp32" else WIDE          # (wide enough for the fused weight update)
    for G in (1, 3):
        xs = torch.cat([volume(i)[0] for i in range(G)]).cuda()
        out = {}
        for name in ("entmin_tta", "memo_tta"):
            cfg = memo_cfg(model_cfg, [], steps=3, lr=1e-3, group=G, tune_volumes=4, precision=precision)
            cfg["method"]["name"] = name
            _, hip = build_pair(model_cfg)
            plug = get_plugin(name)(cfg).setup(hip, "cuda")
            res = plug.adapt_volume(xs)
            out[name] = (plug.logits(res).cpu(), res["losses"].cpu(), len(plug.rt.fused_layers))
        assert out["entmin_tta"][2] == out["memo_tta"][2], "the fused update was not kept"
        if precision == "bf16":
            assert out["memo_tta"][2] > 0
        for a, b in zip(out["entmin_tta"][:2], out["memo_tta"][:2]):
            assert torch.equal(a, b)


def test_memo_group_equals_one_volume_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    G = 3
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = memo_cfg(SMALL, ["w"], steps=3, lr=1e-3, group=group, tune_volumes=4, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(), r["losses"].cpu())
        else:
            zs, ls = [], []
            for v in vols:
                r = plug.adapt_volume(v.cuda())
                zs.append(plug.logits(r).cpu())
                ls.append(r["losses"].cpu())
            runs[(group, use_graph)] = (torch.cat(zs), torch.stack(ls, 1))
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


@pytest.mark.parametrize("group", [1, 2])
def test_returned_logits_are_the_plain_eval_forward_of_the_adapted_replica(group):
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_plugin
    cfg = memo_cfg(SMALL, ["h", "w"], steps=2, lr=1e-3, group=group)
    _, hip = build_pair(SMALL)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    xs = torch.cat([volume(i)[0] for i in range(group)]).cuda()
    z = plug.logits(plug.adapt_volume(xs)).clone()
    rt = plug.rt
    source = rt.arena.source.clone()
    assert not torch.equal(rt.arena.params_all[0], source), "nothing adapted"
    for g in range(group):
        # replica g's adapted weights as the one weight set of a plain eval forward
        _, twin = build_pair(SMALL)
        twin.configure_training(None, plug.no_decay_keys, plug.treat_1d)          # the plugin's arena layout
        twin.cuda()
        rt2 = twin.runtime(torch.device("cuda"))
        assert rt2.arena.total == rt.arena.total
        rt2.arena.params.copy_(rt.arena.params_all[g])
        twin.eval()
        with torch.no_grad():
            want = twin(xs[g:g + 1])
        assert torch.equal(z[g:g + 1], want)


# ----------------------------------------------------------------------------- 8. end to end
def test_seg_tta_eval_with_tta_memo():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_memo", "method.steps=2"])
    cfg["model"] = dict(SMALL)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    _, hip = build_pair(SMALL)
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "MarginalEntropyTTA" and strat.plugin.views == 4
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "loss"} <= set(m)
    assert 0.0 <= m["avg_dc"] <= 1.0


# ----------------------------------------------------------------------------- 9. full width
FULL = dict(name="unet", in_channels=4, num_classes=3, spatial_dims=3, channels=[32, 64, 128, 256, 512],
            strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)


def test_memo_full_width_bf16_tracks_the_restatement():
    """unet 4x128^3 at the width the bench runs, bf16, S = 2, V = 2, against the restatement on the host cores."""
    import oracle
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.models import UNet
    from multimodal_tta_amd.registry import get_plugin
    from multimodal_tta_amd.synth import synth_volume
    axes = ["w"]
    cfg = memo_cfg(FULL, axes, steps=2, group=1, lanes=1, precision="bf16")
    torch.manual_seed(42)
    ref = oracle.UNet(FULL)
    hip = UNet(FULL)
    hip.load_state_dict(ref.state_dict())
    v = synth_volume(0, 4, (128, 128, 128), 3)
    x, y = v["image"].unsqueeze(0), v["label"].unsqueeze(0)
    out_ref = memo_reference(ref, x, cfg["training"], 2, view_masks(axes))
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    assert plug.rt.input_bf16 and plug.rt.thin_grad_dtype() == torch.bfloat16
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, None, x, y, cfg, view_masks(axes), bf16=True)
