"""Modality-consistency adaptation (``modcons_tta``) on the GPU: the modality-subset views against a torch masked copy, the
loss, its terms and its gradient against float64 autograd of the restatement (``modcons_reference.py``), the plugin against
the restatement on the oracle networks, and the bitwise properties (``weight: 0`` = Tent, grouped = one volume at a time,
graph replay = eager, the returned logits = a plain eval forward of the adapted replica)."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from modcons_reference import loss_reference, masked_views, modcons_loss, modcons_reference
from test_hip_tta import SMALL, build_pair, root_cfg, volume

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- 1. the views
def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def filled_rows(G, D, H, W, C, ldc, dtype, gen):
    """A staged input whose every lane (pad lanes too) carries a value, with NaN, -0 and an infinity in every channel."""
    from multimodal_tta_amd import ops
    x = ops.new_cl(G, D, H, W, C, "cuda", ldc=ldc, dtype=dtype)
    base = x if x._base is None else x._base
    host = torch.randn(base.shape, generator=gen)
    host[:, 0, 0, 0, :] = float("nan")
    host[:, 0, 0, 1, :] = -0.0
    host[:, 0, 0, 2, :] = float("-inf")
    base.copy_(host.to(dtype))
    return x, base


def check_views(G, C, ldc, dtype, masks, gen):
    from multimodal_tta_amd import ops
    D, H, W, V = 5, 6, 7, len(masks)
    x, base = filled_rows(G, D, H, W, C, ldc, dtype, gen)
    y = ops.new_cl(G * V, D, H, W, C, "cuda", ldc=ldc, dtype=dtype)
    ybase = y if y._base is None else y._base
    ybase.fill_(float("nan"))
    ops.modality_views(x, y, masks)
    torch.cuda.synchronize()
    xb, yb = bits(base).cpu(), bits(ybase).cpu()
    for g in range(G):
        for v, m in enumerate(masks):
            want = torch.zeros_like(xb[g])          # +0 in the dropped channels and in the pad lanes
            for c in range(C):
                if (m >> c) & 1:
                    want[..., c] = xb[g][..., c]
            assert torch.equal(yb[g * V + v], want), (G, C, ldc, dtype, g, v, m)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("G", [1, 3])
def test_modality_views_are_bit_exact_against_a_masked_copy(dtype, C, G):
    """Dense rows of 4 lanes: kept values bit for bit (NaN payloads included), dropped channels +0 whatever they held (NaN,
    -0, -inf), pad lanes 0; leave-one-out, single, and masks that keep non-adjacent channels, V = 1 .. 8."""
    gen = torch.Generator().manual_seed(31 + C + G)
    full = (1 << C) - 1
    sets = [[full], [full] + [full & ~(1 << c) for c in range(C)], [full] + [1 << c for c in range(C)],
            [full, 0b0101 & full, 0b1010 & full, 0b1001 & full, 0, full, 0b0110 & full, 0b0001]]
    for masks in sets:
        check_views(G, C, 4, dtype, masks, gen)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,ldc", [(3, 3), (5, 8), (2, 2), (6, 6)])
def test_modality_views_on_the_generic_path(dtype, C, ldc):
    gen = torch.Generator().manual_seed(57 + C)
    full = (1 << C) - 1
    for G, masks in ((1, [full, full & ~1, 0b101 & full]), (3, [full] + [full & ~(1 << c) for c in range(C)])):
        check_views(G, C, ldc, dtype, masks, gen)


# ----------------------------------------------------------------------------- 2. the loss against float64
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


def run_loss(z_cl, V, softmax, dtype=torch.float32, weight=0.7, entropy_weight=1.3, detach=True):
    from multimodal_tta_amd import ops
    g = grad_buffer(z_cl, dtype)
    G = z_cl.shape[0] // V
    partial = torch.full((ops.modcons_partials(z_cl, V),), float("nan"), dtype=torch.float64, device="cuda")
    out = {k: torch.full((G,), 123.0, device="cuda") for k in ("loss", "entropy", "consistency")}
    out["view_kl"] = torch.full((G, V - 1), 123.0, device="cuda")
    out["disagree"] = torch.full((G, V - 1), -7, dtype=torch.int64, device="cuda")
    ops.modcons_loss_items(z_cl, g, V, partial, out["loss"], out["entropy"], out["consistency"], out["view_kl"], out["disagree"],
                           weight=weight, entropy_weight=entropy_weight, detach=detach, softmax=softmax)
    torch.cuda.synchronize()
    out = {k: t.cpu() for k, t in out.items()}
    out["grad"] = ops.from_cl(g.float()).cpu()
    return out


HEADS = [(False, 1, False), (False, 3, False), (False, 4, False), (False, 3, True), (False, 4, True), (False, 1, True),
         (True, 3, False), (True, 4, False)]
SATURATED = torch.tensor([0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4])
WEIGHTS = dict(weight=0.7, entropy_weight=1.3)


def check_terms(got, ref, what=""):
    """The project's bounds (check_loss of test_hip_memo.py): every reported mean within 1e-5 relative of float64; the counts
    exact."""
    for key in ("loss", "entropy", "consistency", "view_kl"):
        assert torch.isfinite(got[key]).all(), key
        for a, b in zip(got[key].reshape(-1).tolist(), ref[key].reshape(-1).tolist()):
            print(f"{what}{key} {a} vs {b}")
            assert abs(a - b) <= 1e-5 * abs(b), (key, a, b)
    assert (got["view_kl"] >= 0).all() and (got["consistency"] >= 0).all()
    assert torch.equal(got["disagree"], ref["disagree"]), (got["disagree"], ref["disagree"])


def check_grad(got, g32, ref, dtype):
    assert torch.isfinite(got["grad"]).all()
    gmax = ref["grad"].abs().max().item()
    if dtype == torch.float32:
        err = (got["grad"].double() - ref["grad"]).abs().max().item()
        print(f"gradient error {err / gmax:.2e} of the maximum")
        assert err <= 2e-5 * gmax
    else:
        # the fp32 result rounded to bf16, bit-exact or 1 ulp of bf16 (2^-7 relative)
        want = g32.to(torch.bfloat16).float()
        assert ((got["grad"] - want).abs() <= want.abs() * 2.0 ** -7).all()


def check_loss(z, V, softmax, generic, detach):
    ref = loss_reference(z, V, softmax, detach=detach, **WEIGHTS)
    assert all(torch.isfinite(ref[k]).all() for k in ("loss", "view_kl", "grad"))
    z_cl = stage(z, generic)
    g32 = None
    for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
        got = run_loss(z_cl, V, softmax, dtype, detach=detach, **WEIGHTS)
        check_terms(got, ref, f"V={V} {dtype}: ")
        check_grad(got, g32, ref, dtype)
        g32 = got["grad"]


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("V", [2, 3, 5, 8])
@pytest.mark.parametrize("G", [1, 3])
def test_modcons_loss_matches_float64(softmax, R, generic, V, G):
    gen = torch.Generator().manual_seed(500 + 7 * R + V + G)
    z = torch.randn((G * V, R, 5, 6, 7), generator=gen) * 3.0          # independent logits per view
    for detach in (True, False):
        check_loss(z, V, softmax, generic, detach)


# The second trip of the voxel walk: at most 2048 workgroups of 256 threads per volume, the rest in a grid-stride loop; 81^3
# is the smallest cube with more voxels (531 441) than that (524 288).  The two items are the V = 2 views of one volume.
SECOND_TRIP_SHAPE = (2, 3, 81, 81, 81)
SECOND_TRIP = [pytest.param(False, False, torch.float32, id="bernoulli-fast-fp32"),
               pytest.param(False, False, torch.bfloat16, id="bernoulli-fast-bf16"),
               pytest.param(False, True, torch.float32, id="bernoulli-generic"),
               pytest.param(True, False, torch.float32, id="categorical")]


@functools.lru_cache(maxsize=None)
def second_trip_logits():
    return torch.randn(SECOND_TRIP_SHAPE, generator=torch.Generator().manual_seed(81)) * 3.0


@functools.lru_cache(maxsize=None)
def second_trip_reference(softmax):
    return loss_reference(second_trip_logits(), 2, softmax, detach=False, **WEIGHTS)


@pytest.mark.parametrize("softmax,generic,dtype", SECOND_TRIP)
def test_modcons_loss_on_the_second_trip_of_the_walk(softmax, generic, dtype):
    ref = second_trip_reference(softmax)
    z_cl = stage(second_trip_logits(), generic)
    got = run_loss(z_cl, 2, softmax, dtype, detach=False, **WEIGHTS)
    g32 = run_loss(z_cl, 2, softmax, torch.float32, detach=False, **WEIGHTS)["grad"] if dtype != torch.float32 else None
    check_terms(got, ref, f"{dtype}: ")
    check_grad(got, g32, ref, dtype)


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("V", [2, 5])
def test_modcons_loss_is_finite_and_non_negative_on_saturated_logits(softmax, R, generic, V):
    gen = torch.Generator().manual_seed(600 + R + V)
    G = 2
    z = SATURATED[torch.randint(0, len(SATURATED), (G * V, R, 5, 6, 7), generator=gen)]
    z[:, :, 0, 0, :] = 1e4 if not softmax else 0.0       # every view saturated the same way
    z[:, :, 0, 1, :] = -1e4 if not softmax else 0.0
    if softmax:
        z[:, 0, 0, 0, :] = 1e4
        z[:, 1, 0, 1, :] = -1e4
    for detach in (True, False):
        check_loss(z, V, softmax, generic, detach)


# ----------------------------------------------------------------------------- 3. consistency
@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_identical_views_cost_nothing_and_leave_the_entropy_objective(softmax, R, generic):
    """z_v bitwise equal to z_0: consistency, every view_kl, disagree and the gradient of the views v >= 1 are exactly 0 (the
    teacher's share too: detach is off), and with w_e = 1 view 0 carries mmtta_entropy_loss_items' loss (1e-6 relative) and
    gradient (2e-6 of its maximum) - the bound of test_one_view_is_the_entropy_objective."""
    from multimodal_tta_amd import ops
    gen = torch.Generator().manual_seed(21 + R)
    G, V = 2, 3
    z0 = torch.randn((G, R, 5, 6, 7), generator=gen) * 3.0
    if not softmax:
        z0[:, :, 0, 0, :3] = torch.tensor([90.0, -1e4, 0.0])
    z = z0.unsqueeze(1).repeat(1, V, 1, 1, 1, 1).reshape(G * V, R, 5, 6, 7)
    got = run_loss(stage(z, generic), V, softmax, weight=1.0, entropy_weight=1.0, detach=False)
    assert (got["consistency"] == 0).all() and (got["view_kl"] == 0).all() and (got["disagree"] == 0).all()
    g = got["grad"].reshape(G, V, R, 5, 6, 7)
    assert (g[:, 1:] == 0).all()
    assert torch.equal(got["loss"], got["entropy"])
    z_cl = stage(z0, generic)
    g0 = grad_buffer(z_cl, torch.float32)
    partial = torch.empty(ops.entropy_partials_items(z_cl), dtype=torch.float64, device="cuda")
    loss0 = torch.empty(G, device="cuda")
    ops.entropy_loss_items(z_cl, g0, partial, loss0, softmax=softmax)
    torch.cuda.synchronize()
    g0, loss0 = ops.from_cl(g0).cpu(), loss0.cpu()
    gmax = g0.abs().max().item()
    print(f"vs entropy_loss_items: loss {((got['loss'] - loss0).abs() / loss0.abs()).max().item():.2e}, "
          f"gradient {(g[:, 0] - g0).abs().max().item() / gmax:.2e} of its maximum")
    assert ((got["loss"] - loss0).abs() <= 1e-6 * loss0.abs()).all(), (got["loss"], loss0)
    assert (g[:, 0] - g0).abs().max().item() <= 2e-6 * gmax


@pytest.mark.parametrize("softmax,R,generic,dtype", [(False, 3, False, torch.float32), (False, 3, False, torch.bfloat16),
                                                     (False, 3, True, torch.float32), (True, 4, False, torch.float32)])
def test_g_volumes_equal_g_single_volume_calls(softmax, R, generic, dtype):
    gen = torch.Generator().manual_seed(5)
    G, V = 3, 5
    z = torch.randn((G * V, R, 9, 8, 7), generator=gen) * 3.0
    both = run_loss(stage(z, generic), V, softmax, dtype, detach=False)
    for k in range(G):
        one = run_loss(stage(z[k * V:(k + 1) * V], generic), V, softmax, dtype, detach=False)
        for key in ("loss", "entropy", "consistency", "view_kl", "disagree"):
            assert torch.equal(one[key], both[key][k:k + 1]), key
        assert torch.equal(one["grad"], both["grad"][k * V:(k + 1) * V])


# ----------------------------------------------------------------------------- the plugin against the restatement
def modcons_cfg(model_cfg, steps=3, lr=None, block=None, **method):
    """``lr=None``: the configured learning rate (the reference's)."""
    from multimodal_tta_amd.config import compose
    cfg = root_cfg(model_cfg, steps=steps, lr=1e-3 if lr is None else lr, **method)
    if lr is None:
        cfg["training"]["optimizers"]["adam"]["lr"] = compose(overrides=["task=brats", "model=unet"])["training"]["optimizers"]["adam"]["lr"]
    cfg["method"]["name"] = "modcons_tta"
    cfg["method"]["modcons"] = dict({"subsets": "leave_one_out", "weight": 1.0, "entropy_weight": 1.0, "detach": True}, **(block or {}))
    return cfg


def check_against_reference(z_hip, res, out_ref, ref0, x, y, cfg, masks, softmax=False, bf16=False, **kw):
    """Tent's bounds, as check_against_reference of test_hip_memo.py applies them.  fp32, against a
    float64 run of the restatement: per-step loss 1e-4 relative, final logits within max(2e-3 of max|logits|, 3x the fp32
    restatement's own distance from that run), mask voxels differing only where the float64 logit (softmax head: the float64
    top-2 margin) lies within that bound of the threshold, Dice 1e-3.  bf16, against the fp32 restatement: loss 1e-2, logits
    3e-2 of max|logits|, masks 1e-2, Dice 2e-2, and the bf16 path must have been taken."""
    import oracle
    steps = len(out_ref["losses"])
    losses = res["losses"].cpu().reshape(-1).tolist()
    V = len(masks)
    assert res["view_kl"].shape == (steps, 1, V - 1) and res["disagree"].shape == (steps, 1, V - 1)
    assert res["disagree"].dtype == torch.int64 and res["view_kl"].dtype == torch.float32
    print("view_kl", res["view_kl"][:, 0].cpu().tolist(), "restatement", [k.tolist() for k in out_ref["view_kl"]])
    print("disagree", res["disagree"][:, 0].cpu().tolist(), "restatement", [k.tolist() for k in out_ref["disagree"]])

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
    o64 = modcons_reference(copy.deepcopy(ref0).double(), x.double(), cfg["training"], steps, masks, softmax=softmax, **kw)
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
    assert e_hip <= bound, f"HIP vs fp64 restatement {e_hip:.3e}; fp32 restatement vs fp64 {e_ref:.3e}"
    m_hip, m_ref, m64 = masks_of(z_hip), masks_of(z_ref), masks_of(z64)
    if softmax:
        top2 = z64.topk(2, dim=1).values
        near = ((top2[:, 0] - top2[:, 1]) <= bound * scale).unsqueeze(1)
    else:
        near = z64.abs() <= bound * scale
    assert not torch.any((m_hip != m64) & ~near), "a mask voxel differs away from the threshold"
    d64 = dice(m64)
    dd_hip, dd_ref = (dice(m_hip) - d64).abs().max().item(), (dice(m_ref) - d64).abs().max().item()
    print(f"Dice {dd_hip:.2e} (fp32 restatement {dd_ref:.2e}), mask voxels differing {(m_hip != m64).float().mean().item():.2e}")
    assert dd_hip <= 1e-3, (dd_hip, dd_ref)


def check_records(res):
    """The records hang together: L = w_e H + lambda C (both 1 here) and C = the mean of view_kl, to fp32 rounding."""
    loss, h, c = res["losses"].double().cpu(), res["entropy"].double().cpu(), res["consistency"].double().cpu()
    assert ((loss - (h + c)).abs() <= 1e-6 * loss.abs()).all()
    kl = res["view_kl"].double().cpu().mean(-1).reshape(c.shape)
    assert ((kl - c).abs() <= 1e-6 * c.abs()).all() and (res["view_kl"] >= 0).all() and (res["disagree"] >= 0).all()


# ----------------------------------------------------------------------------- 4. one step, stage by stage
def test_one_modcons_step_matches_torch_stage_by_stage(monkeypatch):
    """One eager step of the plugin read at every stage against torch on the same weights: the V = 5 leave-one-out views'
    logits (5e-4 of their maximum), the loss (1e-5 relative) and every parameter's gradient summed over the views (2e-3 of
    its tensor's maximum) - the whole-network bounds of DESIGN.md section 6."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_plugin
    cfg = modcons_cfg(SMALL, steps=1, lr=1e-3, group=1, use_graph=False)
    ref, hip = build_pair(SMALL)
    x, _ = volume(0)
    plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
    masks = plug.keep_masks
    assert plug.views == 5 and masks == [15, 14, 13, 11, 7] and not plug.rt.fused_layers
    rec = {}
    loss_items, step = ops.modcons_loss_items, plug.optimizer_step

    def spy_loss(logits, dlogits, views, partial, loss, *rest, **kw):
        loss_items(logits, dlogits, views, partial, loss, *rest, **kw)
        rec["z"], rec["loss"], rec["views"], rec["kw"] = ops.from_cl(logits).cpu(), loss.cpu().clone(), views, kw

    def spy_step(volumes=1, fused=False):
        ar = plug.rt.arena
        rec["g"], rec["volumes"] = ar.grads_all[0, :ar.n_train].cpu(), volumes
        step(volumes, fused=fused)

    monkeypatch.setattr(ops, "modcons_loss_items", spy_loss)
    monkeypatch.setattr(plug, "optimizer_step", spy_step)
    res = plug.adapt_volume(x.cuda())
    assert rec["views"] == 5 and rec["volumes"] == 1 and rec["kw"]["detach"] is True and rec["kw"]["weight"] == 1.0
    check_records(res)
    ref.train()
    z = ref(masked_views(x, masks))
    loss = modcons_loss(z, 5, False)[0][0]
    loss.backward()
    print(f"logits {(rec['z'] - z.detach()).abs().max().item() / z.abs().max().item():.2e} of their maximum; "
          f"loss {rec['loss'].item()} vs {loss.item()}")
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


# ----------------------------------------------------------------------------- 5. S steps against the restatement
@pytest.mark.parametrize("detach", [True, False], ids=["teacher", "both-sides"])
def test_modcons_leave_one_out_matches_the_restatement(detach):
    from multimodal_tta_amd.registry import get_plugin
    cfg = modcons_cfg(SMALL, steps=3, group=1, block={"detach": detach})
    ref, hip = build_pair(SMALL)
    ref0 = copy.deepcopy(ref)
    x, y = volume(0)
    plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
    assert plug.views == 5
    out_ref = modcons_reference(ref, x, cfg["training"], 3, plug.keep_masks, detach=detach)
    res = plug.adapt_volume(x.cuda())
    assert res["losses"].shape == (3,) and res["entropy"].shape == (3,) and res["consistency"].shape == (3,)
    check_records(res)
    check_against_reference(plug.logits(res).cpu(), res, out_ref, ref0, x, y, cfg, plug.keep_masks, detach=detach)


def test_modcons_hecktor_shaped_model_with_single_modality_views():
    """One region, two modalities (PET / CT), a ragged-aspect volume, ``single``: V = 3."""
    from multimodal_tta_amd.registry import get_plugin
    mcfg = dict(SMALL, in_channels=2, num_classes=1)
    cfg = modcons_cfg(mcfg, steps=3, group=1, block={"subsets": "single"})
    ref, hip = build_pair(mcfg, seed=7)
    ref0 = copy.deepcopy(ref)
    x, y = volume(2, shape=(16, 48, 48), C=2, R=1)
    plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
    assert plug.views == 3 and plug.keep_masks == [3, 1, 2]
    out_ref = modcons_reference(ref, x, cfg["training"], 3, plug.keep_masks)
    res = plug.adapt_volume(x.cuda())
    check_records(res)
    check_against_reference(plug.logits(res).cpu(), res, out_ref, ref0, x, y, cfg, plug.keep_masks)


def test_modcons_softmax_head_matches_the_restatement():
    from multimodal_tta_amd.registry import get_plugin
    mcfg = dict(SMALL, num_classes=4)
    cfg = modcons_cfg(mcfg, steps=3, group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    ref, hip = build_pair(mcfg)
    ref0 = copy.deepcopy(ref)
    x, y = volume(1, R=4)
    plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
    assert plug.softmax and plug.views == 5
    out_ref = modcons_reference(ref, x, cfg["training"], 3, plug.keep_masks, softmax=True)
    res = plug.adapt_volume(x.cuda())
    check_records(res)
    check_against_reference(plug.logits(res).cpu(), res, out_ref, ref0, x, y, cfg, plug.keep_masks, softmax=True)


def test_modcons_with_a_missing_modality():
    """``missing_modalities: [1]``: view 0 is the volume without channel 1, the three views leave one of the others out."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = modcons_cfg(SMALL, steps=3, group=1, missing_modalities=[1])
    ref, hip = build_pair(SMALL)
    ref0 = copy.deepcopy(ref)
    x, y = volume(3)
    plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
    assert plug.views == 4 and plug.keep_masks == [0b1101, 0b1100, 0b1001, 0b0101]
    out_ref = modcons_reference(ref, x, cfg["training"], 3, plug.keep_masks)
    res = plug.adapt_volume(x.cuda())
    check_records(res)
    check_against_reference(plug.logits(res).cpu(), res, out_ref, ref0, x, y, cfg, plug.keep_masks)


def test_modcons_bf16_tracks_the_restatement():
    from multimodal_tta_amd.registry import get_plugin
    cfg = modcons_cfg(SMALL, steps=3, group=1, precision="bf16")
    ref, hip = build_pair(SMALL)
    x, y = volume(5)
    plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
    out_ref = modcons_reference(ref, x, cfg["training"], 3, plug.keep_masks)
    res = plug.adapt_volume(x.cuda())
    check_records(res)
    check_against_reference(plug.logits(res).cpu(), res, out_ref, None, x, y, cfg, plug.keep_masks, bf16=True)


# ----------------------------------------------------------------------------- 6. bit for bit
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_weight_zero_is_bitwise_entmin(precision):
    """``weight: 0``: the plugin runs entmin_tta's own step - one view, its loss kernel, its fused update."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_groups import WIDE
    model_cfg = SMALL if precision == "fp32" else WIDE          # (wide enough for the fused weight update)
    for G in (1, 3):
        xs = torch.cat([volume(i)[0] for i in range(G)]).cuda()
        out = {}
        for name in ("entmin_tta", "modcons_tta"):
            cfg = modcons_cfg(model_cfg, steps=3, lr=1e-3, block={"weight": 0.0}, group=G, tune_volumes=4, precision=precision)
            cfg["method"]["name"] = name
            _, hip = build_pair(model_cfg)
            plug = get_plugin(name)(cfg).setup(hip, "cuda")
            assert plug.views == 1 and hip.views == 1
            res = plug.adapt_volume(xs)
            out[name] = (plug.logits(res).cpu(), res["losses"].cpu(), len(plug.rt.fused_layers))
            if name == "modcons_tta":
                assert torch.equal(res["entropy"], res["losses"]) and (res["consistency"] == 0).all()
                assert res["view_kl"].shape == (3, G, 0) and res["disagree"].shape == (3, G, 0)
        assert out["entmin_tta"][2] == out["modcons_tta"][2], "the fused update was not kept"
        if precision == "bf16":
            assert out["modcons_tta"][2] > 0
        for a, b in zip(out["entmin_tta"][:2], out["modcons_tta"][:2]):
            assert torch.equal(a, b)


def test_modcons_group_equals_one_volume_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    G = 2
    keys = ("losses", "entropy", "consistency", "view_kl", "disagree")
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = modcons_cfg(SMALL, steps=3, lr=1e-3, group=group, tune_volumes=4, use_graph=use_graph, block={"detach": False})
        _, hip = build_pair(SMALL)
        plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
        assert plug.group == group and plug.views == 5
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            assert r["losses"].shape == (3, G) and r["view_kl"].shape == (3, G, 4) and r["disagree"].shape == (3, G, 4)
            runs[(group, use_graph)] = [plug.logits(r).cpu()] + [r[k].cpu() for k in keys]
        else:
            rs, zs = [], []
            for v in vols:
                r = plug.adapt_volume(v.cuda())
                zs.append(plug.logits(r).cpu())          # (the logits live in a pool buffer the next call writes again)
                rs.append({k: r[k].cpu().clone() for k in keys})
            runs[(group, use_graph)] = [torch.cat(zs)] + [torch.stack([r[k].cpu() for r in rs], 1) for k in keys[:3]] + \
                                       [torch.cat([r[k].cpu() for r in rs], 1) for k in keys[3:]]
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


@pytest.mark.parametrize("group", [1, 2])
def test_returned_logits_are_the_plain_eval_forward_of_the_adapted_replica(group):
    """... on the base-masked volume (``missing_modalities: [1]``), and the views do not stick to the runtime or the model."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = modcons_cfg(SMALL, steps=2, lr=1e-3, group=group, missing_modalities=[1])
    _, hip = build_pair(SMALL)
    plug = get_plugin("modcons_tta")(cfg).setup(hip, "cuda")
    assert plug.views == 4 and hip.views == 4
    xs = torch.cat([volume(i)[0] for i in range(group)]).cuda()
    z = plug.logits(plug.adapt_volume(xs)).clone()
    rt = plug.rt
    assert rt.views == 1 and not rt.use_sets
    source = rt.arena.source.clone()
    assert not torch.equal(rt.arena.params_all[0], source), "nothing adapted"
    keep = torch.tensor([1.0, 0.0, 1.0, 1.0], device="cuda").view(1, 4, 1, 1, 1)
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
            want = twin(xs[g:g + 1] * keep)
        assert torch.equal(z[g:g + 1], want)
    # the model takes one item per volume again under entmin_tta
    cfg = modcons_cfg(SMALL, steps=1, lr=1e-3, group=group)
    cfg["method"]["name"] = "entmin_tta"
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    assert hip.views == 1 and plug.rt.views == 1
    assert plug.adapt_volume(xs)["losses"].shape == ((1,) if group == 1 else (1, group))


def test_modcons_refuses_running_statistics_and_too_many_volumes():
    from multimodal_tta_amd.registry import get_plugin
    batch = dict(SMALL, norm="BATCH")
    _, hip = build_pair(batch)
    with pytest.raises(NotImplementedError, match="running"):
        get_plugin("modcons_tta")(modcons_cfg(batch, steps=1, group=1)).setup(hip, "cuda")
    _, hip = build_pair(SMALL)
    plug = get_plugin("modcons_tta")(modcons_cfg(SMALL, steps=1, group=1)).setup(hip, "cuda")
    with pytest.raises(NotImplementedError, match="method.group = 1"):
        plug.adapt_volume(torch.cat([volume(0)[0], volume(1)[0]]).cuda())


# ----------------------------------------------------------------------------- 7. end to end
def test_seg_tta_eval_with_tta_modcons():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_modcons", "method.steps=2"])
    cfg["model"] = dict(SMALL)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    _, hip = build_pair(SMALL)
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "ModalityConsistencyTTA" and strat.plugin.views == 5
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "loss"} <= set(m)
    assert 0.0 <= m["avg_dc"] <= 1.0
